"""The fast parse of values above 16382 bytes (PMC_LEVEL_FAST_ALL, include/pmc_codec.h "compression
level"), stated in plain Python on tests/dict_model.py: the value is cut into segments of G bytes, and each
segment is parsed as dict_model parses a value behind a dictionary -- the dictionary being the H bytes that
precede the segment in the same value (fewer for a segment that starts before H; none for the first).
csrc/pmc_deflate_fast_large.hip (lv_fast_parse_kernel) computes the same token sequence on the GPU;
tests/test_gpu_fast_large.py compares the two token by token.

So a match never extends past its segment's end (the table's cap is the bytes left in the staged range), a
distance reaches at most G + H - 1, and a segment's tokens depend on the G + H bytes around it only.

Tokens are in the form tests/deflate_dissect.py returns: an int for a literal byte, (len, dist) for a match.
"""
from dict_model import dict_tokens, replay_with
from fast_model import FAST_MAX

G = 2048  # segment bytes   (csrc/pmc_deflate_fast_large.hip kFlSeg)
H = 2048  # history bytes   (kFlHist)
assert G + H <= FAST_MAX


def segments(v):
    """[(history, segment)] of a value, in order."""
    v = bytes(v)
    return [(v[s0 - min(s0, H):s0], v[s0:s0 + G]) for s0 in range(0, len(v), G)]


def fast_large_segment_tokens(v):
    """The token list of every segment."""
    return [dict_tokens(h, s) for h, s in segments(v)]


def fast_large_tokens(v):
    return [t for toks in fast_large_segment_tokens(v) for t in toks]


def replay_segments(v, seg_tokens):
    """The bytes the per-segment token lists stand for, each decoded behind its history of `v`."""
    return b"".join(replay_with(h, toks) for (h, _), toks in zip(segments(v), seg_tokens))

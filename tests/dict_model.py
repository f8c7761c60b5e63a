"""The fast level's parse behind a preset dictionary (include/pmc_codec.h "preset dictionary"), stated in
plain Python on tests/fast_model.py's functions: the match table over dictionary || value, walked from the
value's first byte.  csrc/pmc_deflate_fast.hip (deflate_front_fast_dict_kernel) computes the same token
sequence on the GPU; tests/test_gpu_dict.py compares the two token by token.

Tokens are in the form tests/deflate_dissect.py returns: an int for a literal byte, (len, dist) for a match;
a distance may exceed the bytes of the value before the match, by at most the dictionary's length.
"""
from fast_model import CAPT, FAST_MAX, LAZY, MAX_MATCH, match_table


def dict_tokens(dictionary, value):
    d, v = bytes(dictionary), bytes(value)
    D = len(d)
    c = d + v
    n = len(c)
    assert n <= FAST_MAX
    # (position 0 of the concatenation -- the dictionary's first byte -- is never a candidate; for a
    # position of the value, the table's cap min(CAPT, n - p) is the bytes left in the value)
    ml, mq = match_table(c)
    toks = []
    p = D
    while p < n:
        m = ml[p]
        if m >= 3 and not (LAZY and p + 1 < n and ml[p + 1] > m):
            q = mq[p]
            if m == CAPT:
                lim = min(MAX_MATCH, n - p)
                while m < lim and c[q + m] == c[p + m]:
                    m += 1
            toks.append((m, p - q))
            p += m
        else:
            toks.append(c[p])
            p += 1
    return toks


def replay_with(dictionary, toks):
    """The bytes a token sequence stands for, decoded behind `dictionary`."""
    out = bytearray(dictionary)
    D = len(out)
    for t in toks:
        if isinstance(t, tuple):
            ln, dist = t
            assert dist <= len(out)
            for _ in range(ln):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out[D:])

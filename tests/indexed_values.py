"""Values shared by the tests of indexed members (tests/test_indexed_model.py, tests/test_gpu_indexed.py):
the smallest shapes where a chunk edge, a 1-3 byte tail chunk, a cut match or a stored block can go wrong."""
import numpy as np

from fast_large_model import G, H
from fast_large_values import BIG_NAME, big_value
from fast_values import alnum, json_slices
from indexed_model import C

# C: the longest value the switch leaves alone; C + 1 .. 2 C + 3: a last chunk of 1, 0 (none), 1, 2 and 3 bytes
# (no / one hashable position); 3 C - 1: one byte short of three chunks; C + G, C + G + 1: a second chunk of
# one segment, and of one segment and a byte; 100000, 4 C: several chunks (and 16383-symbol blocks)
JSON_SIZES = [C, C + 1, 2 * C, 2 * C + 1, 2 * C + 2, 2 * C + 3, 3 * C - 1, C + G, C + G + 1, 100000, 4 * C]
PERIOD = H + 904  # the copy lies further back than the history
RANDOM_NAME = "random70000"
LAST_MATCH_NAME, LAST_MATCH_TEXT = "last_match", 16757  # (the length found by the model: 16383 tokens)


def across_value(rng) -> bytes:
    """A 300-byte string at C - 1174 and again across offset C: the first 150 bytes of the copy match their
    source 1024 bytes back (within the history) (cut at the chunk's end); the second 150 must not be found from before C."""
    rep = alnum(rng, 300)
    v = bytearray(alnum(rng, C + G + 500))
    v[C - 1174:C - 874] = rep
    v[C - 150:C + 150] = rep
    return bytes(v)


def last_match_value(tiled: bytes) -> bytes:
    """C bytes of JSON, then a last chunk of exactly 16383 tokens whose last one is a match (random text, and
    40 bytes of it again from 300 bytes back): the 16383rd symbol of a block is the value's last token, and it
    must end the final block -- no empty block after it."""
    text = alnum(np.random.default_rng(20263), LAST_MATCH_TEXT)
    return json_slices(tiled, C, 1, 3100)[0] + text + text[-300:-260]


def indexed_values(corpus: bytes):
    """[(name, value)], the 1 MiB value last."""
    rng = np.random.default_rng(20262)
    assert len(corpus) > G + H
    tiled = corpus * 3  # (the corpus is 82 KB; the tiling's period is beyond the parse's reach)
    vals = [(f"json{n}", json_slices(tiled, n, 1, 3000 + k)[0]) for k, n in enumerate(JSON_SIZES)]
    vals.append(("a_run", b"a" * (2 * C + 5000)))
    period = alnum(rng, PERIOD)
    vals.append(("period", (period * ((2 * C + 5000) // PERIOD + 1))[:2 * C + 5000]))
    vals.append(("across", across_value(rng)))
    vals.append((RANDOM_NAME, rng.integers(0, 256, size=70000, dtype=np.uint8).tobytes()))
    vals.append((LAST_MATCH_NAME, last_match_value(tiled)))
    vals.append((BIG_NAME, big_value(corpus, rng)))
    return vals

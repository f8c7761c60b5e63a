"""Values shared by the tests of the fast level for large values (tests/test_fast_large_model.py,
tests/test_gpu_fast_large.py): every size follows the model's segment and history lengths."""
import numpy as np

from fast_large_model import G, H
from fast_model import FAST_MAX
from fast_values import alnum, json_slices

# M segments are the fewest that make a large value (M * G > 16382)
M = FAST_MAX // G + 1
# 16383: the first length of the large path; around two segments: a last segment of 0 (none), 1, 2 and 3
# bytes (no / one hashable position of its own); one byte short of three segments; G + H: the second segment
# is exactly the history's length; 40000 / 65536 / 100000: several 16383-symbol blocks.  Where 2 G is at
# most 16382 those lengths take the small path (plain fast members), so the same edges follow around M
# segments, on the large path.
STATED_SIZES = [16383, 2 * G, 2 * G + 1, 2 * G + 2, 2 * G + 3, 3 * G - 1, G + H, 40000, 65536, 100000]
JSON_SIZES = list(dict.fromkeys(STATED_SIZES + [M * G, M * G + 1, M * G + 2, M * G + 3, (M + 1) * G - 1]))
BIG_NAME = "json_mix_1MiB"  # round trip only: no model comparison

BASELINE_SIZE, BASELINE_COUNT = 65536, 24

STRADDLE_AT, STRADDLE_BACK = M * G, min(3000, H // 2)


def straddle_value(rng) -> bytes:
    """A 300-byte string whose second copy lies across a segment boundary (STRADDLE_AT), STRADDLE_BACK
    bytes behind the first: its match is cut at the boundary, and the rest is found again from the next
    segment (its source in the history)."""
    rep = alnum(rng, 300)
    v = bytearray(alnum(rng, STRADDLE_AT + G + 500))
    v[STRADDLE_AT - STRADDLE_BACK - 150:STRADDLE_AT - STRADDLE_BACK + 150] = rep
    v[STRADDLE_AT - 150:STRADDLE_AT + 150] = rep
    return bytes(v)


def big_value(corpus: bytes, rng) -> bytes:
    """1 MiB of repeated, shuffled JSON slices."""
    pool = json_slices(corpus, 4096, 32, 77)
    order = rng.integers(0, len(pool), size=(1 << 20) // 4096)
    return b"".join(pool[int(k)] for k in order)


def large_values(corpus: bytes):
    """[(name, value)], the 1 MiB value last."""
    rng = np.random.default_rng(20261)
    # (the corpus is 82 KB: the longest slice comes from the corpus tiled, as tests/large_values.py's do; the
    # tiling's period is beyond the parse's reach)
    assert len(corpus) > G + H
    vals = [(f"json{n}", json_slices(corpus * 3, n, 1, 2000 + k)[0]) for k, n in enumerate(JSON_SIZES)]
    vals.append(("a50000", b"a" * 50000))
    period = alnum(rng, H + 904)
    vals.append(("period", (period * (50000 // len(period) + 1))[:50000]))
    vals.append(("straddle", straddle_value(rng)))
    vals.append(("random40000", rng.integers(0, 256, size=40000, dtype=np.uint8).tobytes()))
    vals.append((BIG_NAME, big_value(corpus, rng)))
    return vals

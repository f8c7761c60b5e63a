"""Values shared by the fast level's tests (tests/test_fast_model.py, tests/test_gpu_fast.py): the edge
list of the fast parse and the two seeded JSON-slice sets of tests/golden/fast_baseline.json."""
import numpy as np

# sizes by what they exercise: no / one hashable position; the lane boundary; the 258-byte match boundary;
# the back's header class; the front's size-class instances; the packed chain-count class (12-bit sorted
# positions from 3073 on); the last fast size
EDGE_SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 511, 512, 513, 1023, 1024, 1025, 3072, 3073,
              4095, 4096, 4097, 16382]
PATTERN_SIZES = [1, 2, 3, 4, 5, 64, 65, 258, 259, 260, 513, 1024, 1025, 3073, 4096, 4097, 16382]
ALNUM = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)


def json_slices(corpus: bytes, size: int, count: int, seed: int):
    """`count` slices of `size` bytes at numpy default_rng(seed) offsets."""
    offs = np.random.default_rng(seed).integers(0, len(corpus) - size + 1, size=count)
    return [corpus[int(o):int(o) + size] for o in offs]


def alnum(rng, n: int) -> bytes:
    return ALNUM[rng.integers(0, len(ALNUM), size=n)].tobytes()


def collision_value(rng, units: int = 60) -> bytes:
    """Trigrams b"\\x00xy" and b"\\x20xy" share the 15-bit hash (bit 15 of b0 << 10 is masked off), so the
    occurrences of one use up the candidate slots of the other."""
    out = bytearray(b"#")
    for _ in range(units):
        out += (b"\x00xy", b"\x20xy")[int(rng.integers(0, 2))] + b"QRSTUV" + alnum(rng, 5)
    return bytes(out)


def pos0_value(rng) -> bytes:
    """The only earlier occurrence of b"abc" is at position 0 (never a candidate); b"bcdefgh" at 1 is one."""
    return b"abcdefgh" + alnum(rng, 40).replace(b"a", b"A").replace(b"b", b"B") + b"abcdefgh" + b"!?"


def too_far_value(rng) -> bytes:
    """b"#$%" repeats 4190 bytes apart (a length-3 match beyond 4096: dropped), b"&*(" 4090 apart (kept)."""
    v = bytearray(alnum(rng, 4400))
    v[10:13], v[4200:4203] = b"#$%", b"#$%"
    v[100:103], v[4190:4193] = b"&*(", b"&*("
    return bytes(v)


LAZY_VALUE = b"_abcdefghij" + b"!@#$%^&*()" + b"Zab?" + b"[]{}<>;:,." + b"Zabcdefghij~"


def edge_values(corpus: bytes):
    """[(name, value)]: every edge size as a JSON slice, then the patterns."""
    rng = np.random.default_rng(20260)
    vals = []
    for k, n in enumerate(EDGE_SIZES):
        vals.append((f"json{n}", json_slices(corpus, n, 1, 1000 + k)[0]))
    for n in PATTERN_SIZES:
        vals.append((f"zero{n}", bytes(n)))
        vals.append((f"ab{n}", (b"ab" * (n // 2 + 1))[:n]))
        vals.append((f"abc{n}", (b"abc" * (n // 3 + 1))[:n]))
    for n in (64, 513, 1024, 4096, 16382):
        vals.append((f"alnum{n}", alnum(rng, n)))
    vals.append(("collide", collision_value(rng)))
    vals.append(("collide_long", collision_value(rng, 300)))
    vals.append(("pos0", pos0_value(rng)))
    vals.append(("too_far", too_far_value(rng)))
    vals.append(("lazy", LAZY_VALUE))
    return vals


BASELINE_SETS = {"1k": (1024, 300), "4k": (4096, 100)}

"""Inputs of the compress boundary tests (test infrastructure): stream windows and the route table.

A value is a window T[a : a + len] of a stream T of 1 MiB and is handed to the kernels where it lies: `src` holds
the streams and src_off[i] points into one.  So the bytes before and behind every value continue it -- a matcher
that runs a match one byte past the value, or finds a candidate before its first byte, then writes a different
member, which it would not with the zero padding of pmc_codec.device.pack.  Every window keeps 32768 + 64 bytes of
its stream before it and 258 + 64 behind it, so no kernel, right or wrong, is steered outside the buffer.

Shared by tests/test_boundary_model.py (CPU: the routes, how many windows are sensitive, the reference's members),
tests/test_gpu_compress_bounds.py and tests/golden/make_boundary_golden.py, so all three speak of the same bytes.
"""
import hashlib
import json
import os

import numpy as np

import deflate_dissect

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

STREAM_LEN = 1 << 20
LEFT = 32768 + 64    # bytes of its stream every window keeps before it (the window size and a staging's slack)
RIGHT = 258 + 64     # ... and behind it (the longest match and the 16/32-byte steps of the match loops)
STREAM_NAMES = ("p1", "p2", "p259", "p4099", "json")

EXACT, FAST, FAST_ALL = 9, 1, 2

# the edge lengths, by the route that admits them
EDGE_4K = [1, 2, 3, 4, 5, 257, 258, 259, 260, 261, 2047, 2048, 2049, 4095, 4096]
EDGE_16K = [4097, 16381, 16382]
EDGE_BIG = [16383, 16384, 16385]
EDGE_LV = [32505, 32506, 32507, 32767, 32768, 32769, 65535, 65536, 65537, 100001]
BIG_MAX = 31808      # deflate_big_limit() of this build: the longest value of the split pipeline's large pass
BIG_RANDOM = 20000   # random bytes: two stored blocks, so the large pass hands the value to the gated HBM kernel
DICT_LEN = 4096
DICT_EDGE = 16382 - DICT_LEN  # 12286: the longest value that becomes a dictionary member
EDGE_DICT = [DICT_EDGE - 1, DICT_EDGE, DICT_EDGE + 1] + EDGE_16K + EDGE_4K


def corpus():
    d = os.path.join(GOLDEN, "data")
    return b"".join(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".json"))


_STREAMS = None


def streams():
    """{name: 1 MiB of bytes}, NUL-free (the reference's Compress takes C strings)."""
    global _STREAMS
    if _STREAMS is None:
        rng = np.random.default_rng(0xB0DA)
        tile = lambda unit: (unit * (STREAM_LEN // len(unit) + 1))[:STREAM_LEN]  # noqa: E731
        _STREAMS = {
            "p1": tile(b"a"),
            "p2": tile(b"ab"),
            # 259 random bytes: a 258-byte match at distance 259 is on offer at every position
            "p259": tile(bytes(rng.integers(1, 256, 259, dtype=np.uint8))),
            # 4099 symbols of a 4-letter alphabet: the period lies just past TOO_FAR (4096)
            "p4099": tile(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 4099))),
            "json": tile(corpus()),
        }
    return _STREAMS


def stream_base(name):
    """Where stream `name` starts in source_bytes()."""
    return STREAM_NAMES.index(name) * STREAM_LEN


def source_bytes():
    """The five streams back to back: the `src` buffer of every call."""
    s = streams()
    return b"".join(s[n] for n in STREAM_NAMES)


class Window:
    """T[a : a + n] of stream `name`; `random`: the bytes are not the stream's but seeded random ones, which
    the tests write over a copy of the stream at that place (the large pass's multi-block value)."""

    def __init__(self, name, a, n, random=False):
        assert a >= LEFT and a + n + RIGHT <= STREAM_LEN, (name, a, n)
        self.name, self.a, self.n, self.random = name, a, n, random

    @property
    def off(self):
        return stream_base(self.name) + self.a

    def __repr__(self):
        return f"{self.name}[{self.a}:+{self.n}]"


# a % 16 of window k: every residue, and every a % 4 within four consecutive windows
RESIDUES = [0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 15, 14, 9, 4]


def _windows(lens, seed, names=STREAM_NAMES):
    out = []
    for k, n in enumerate(lens):
        span = STREAM_LEN - LEFT - RIGHT - n - 32
        a = LEFT + 16 + (k * 7919 + seed * 104729) % span
        a = a - a % 16 + RESIDUES[(k + k // 16) % 16]
        out.append(Window(names[k % len(names)], a, n))
    return out


def _fill(lens, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return lens + [int(x) for x in rng.integers(lo, hi + 1, n - len(lens))]


def _times5(edges):
    return [n for n in edges for _ in range(5)]  # (each edge length once per stream)


def shape(name):
    """The windows of one batch shape."""
    if name == "mono":       # 192 values of <= 4096 bytes
        return _windows(_fill(_times5(EDGE_4K), 192, 6, 4096, 1), 1)
    if name == "split-s12":  # 1100 values of <= 4096 bytes (the fill stays short: the CPU model dissects them all)
        return _windows(_fill(_times5(EDGE_4K), 1100, 6, 1200, 2), 2)
    if name == "split":      # 96 values of <= 16382 bytes
        return _windows(_fill(_times5(EDGE_16K + EDGE_4K), 96, 4097, 16382, 3), 3)
    if name == "big":        # 6 values of 16383 .. 31808 bytes, one of them random
        w = _windows(EDGE_BIG + [BIG_RANDOM, BIG_MAX - 2, BIG_MAX], 4, ("p259", "json", "p4099", "p2", "p2", "p1"))
        # (the random bytes are written over the stream: far from every other window, so none of them sees them)
        w[3] = Window("p2", 900003, BIG_RANDOM, random=True)
        return w
    if name == "lv":         # 12 values of 32505 .. 100001 bytes and 4 small ones
        return _windows(EDGE_LV + [49153, 81923] + [5, 260, 2049, 16382], 5)
    if name == "lv-json":    # 4 large JSON windows, each found right- and left-sensitive (tests/test_boundary_model.py
        # holds them to it): tiled JSON stitches, so none of them may reach the stitch's fallback
        return [Window("json", a, n) for a, n in ((132837, 32507), (232842, 49153), (332843, 65537), (432848, 100001))]
    if name == "fast-dict":  # 111 values on both sides of 12286: every edge length up to 16382 on every stream
        return _windows(_fill(_times5(EDGE_DICT), 111, 6, 16382, 6), 6)
    if name == "fast-all":   # 14 values of 16383 .. 100001 bytes: every edge length of that range
        return _windows(EDGE_BIG + EDGE_LV + [49154], 7)
    if name == "fast-idx":   # 8 values of 32769 .. 100001 bytes (K >= 2 chunks of 32768)
        return _windows([32769, 65535, 65536, 65537, 98304, 98305, 100001, 49154], 8)
    raise KeyError(name)


# id -> level, environment switch, context switches, the shapes of its batches
ROWS = {
    "mono": dict(level=EXACT, shapes=["mono"]),
    "split-s12": dict(level=EXACT, shapes=["split-s12"]),
    "split": dict(level=EXACT, shapes=["split"]),
    "big": dict(level=EXACT, shapes=["big"]),
    "lv": dict(level=EXACT, shapes=["lv", "lv-json"]),
    "v1": dict(level=EXACT, env="PMC_DEFLATE_V1", shapes=["mono", "split", "lv"]),
    "mono-env": dict(level=EXACT, env="PMC_DEFLATE_MONO", shapes=["split"]),
    "fast": dict(level=FAST, shapes=["split"]),
    "fast-dict": dict(level=FAST, dict=True, shapes=["fast-dict"]),
    "fast-all": dict(level=FAST_ALL, shapes=["fast-all"]),
    "fast-idx": dict(level=FAST_ALL, index=True, shapes=["fast-idx"]),
    "fast-idx-crc": dict(level=FAST_ALL, index=True, index_crc=True, shapes=["fast-idx"]),
}
LEVEL9_SHAPES = ["mono", "split-s12", "split", "big", "lv", "lv-json"]


def random_bytes(w):
    """The bytes of a `random` window (NUL-free)."""
    return bytes(np.random.default_rng(w.a).integers(1, 256, w.n, dtype=np.uint8))


def stream_of(w):
    """The stream window w lies in, as the kernels see it (with a random window's bytes written in)."""
    T = streams()[w.name]
    return T[:w.a] + random_bytes(w) + T[w.a + w.n:] if w.random else T


def source_for(windows):
    """source_bytes() with the random windows' bytes written in (numpy uint8, writable)."""
    buf = np.frombuffer(source_bytes(), dtype=np.uint8).copy()
    for w in windows:
        if w.random:
            buf[w.off:w.off + w.n] = np.frombuffer(random_bytes(w), dtype=np.uint8)
    return buf


def value(w):
    return stream_of(w)[w.a:w.a + w.n]


def dictionary():
    """The fast-dict row's dictionary: the 4096 bytes of the JSON stream just before the first JSON window."""
    w = next(w for w in shape("fast-dict") if w.name == "json")
    return streams()["json"][w.a - DICT_LEN:w.a]


# ---- sensitivity -------------------------------------------------------------------------------------------
def right_sensitive(w, member):
    """The member's last token is a match of length < 258 at distance d, and the byte behind the value equals
    the one d before it: a matcher that read one byte past the value's end would lengthen that match."""
    blocks = deflate_dissect.dissect(member)
    toks = blocks[-1].get("tokens") or []
    if not toks or not isinstance(toks[-1], tuple):
        return False
    ln, d = toks[-1]
    T, end = stream_of(w), w.a + w.n
    return ln < 258 and T[end] == T[end - d]


def left_sensitive(w):
    """The value's first 3 bytes occur in the 32768 bytes before it: a matcher that looked before the value's
    first byte would find a candidate for its position 0."""
    T = stream_of(w)
    return w.n >= 3 and T[w.a:w.a + 3] in T[w.a - 32768:w.a]


# ---- the reference's members ---------------------------------------------------------------------------------
def sha(b):
    return hashlib.sha256(b).hexdigest()


class BoundaryGolden:
    """tests/golden/boundary_golden.json (tests/golden/make_boundary_golden.py): the reference's member of every
    level-9 value, as SHA-256 + length, keyed by the value's SHA-256."""

    def __init__(self):
        with open(os.path.join(GOLDEN, "boundary_golden.json")) as f:
            self.vectors = json.load(f)["vectors"]

    def mismatches(self, values, members):
        """Indices whose member is not the reference's (or whose value has no vector)."""
        bad = []
        for k, (v, m) in enumerate(zip(values, members)):
            want = self.vectors.get(sha(v))
            if want is None or len(m) != want["gz_len"] or sha(m) != want["gz_sha256"]:
                bad.append(k)
        return bad

"""Dictionaries and values shared by the preset dictionary's tests (tests/test_dict_model.py,
tests/test_gpu_dict.py): the edge list of the fast parse behind a dictionary, and the dictionary and the two
seeded JSON-slice sets of tests/golden/dict_baseline.json."""
import zlib

import numpy as np

from fast_values import alnum, json_slices

SPAN = 16382  # a dictionary of D bytes is used for values of D + len <= SPAN

# dictionary lengths: the shortest (no, one hashable position of its own), the lane boundary, the packed-ml
# class (D + n <= 1024), 2 KiB (the baseline's), the longest
DICT_SIZES = [1, 2, 3, 63, 64, 65, 1024, 2048, 8192]
# value lengths: no / one hashable position of their own, a window of the walk, the 258-byte match boundary,
# 1 KiB; then SPAN - D (the last dictionary member) and SPAN - D + 1 (a plain fast member)
VALUE_SIZES = [1, 2, 3, 64, 258, 259, 1024]

DISTINCT = bytes(range(0x30, 0x58))  # 40 different bytes: no trigram twice
FILL1, FILL2 = bytes(range(0x64, 0x74)), bytes(range(0x74, 0x84))  # 16 + 16 more, none of them in a pattern's text


def edge_pairs(corpus: bytes):
    """[(name, dictionary, value)]: every dictionary size with every value size (JSON slices of one corpus, so
    the value finds its keys in the dictionary), then the patterns."""
    out = []
    for i, D in enumerate(DICT_SIZES):
        d = json_slices(corpus, D, 1, 3000 + i)[0]
        for j, n in enumerate(VALUE_SIZES + [SPAN - D, SPAN - D + 1]):
            out.append((f"d{D}_v{n}", d, json_slices(corpus, n, 1, 4000 + 16 * i + j)[0]))
    out += list(patterns(corpus).values())
    return out


def uses_dictionary(dictionary: bytes, value: bytes) -> bool:
    return 1 <= len(value) and len(dictionary) + len(value) <= SPAN


def patterns(corpus: bytes):
    """{name: (name, dictionary, value)}, each built for one rule of the parse."""
    rng = np.random.default_rng(20261)
    P = {}

    def add(name, d, v):
        P[name] = (name, bytes(d), bytes(v))

    j1k, j2k = json_slices(corpus, 1024, 1, 77)[0], json_slices(corpus, 2048, 1, 78)[0]
    add("tail", j1k, j1k[-200:])            # the value is the dictionary's tail
    add("whole", j2k, j2k)                  # the value is the whole dictionary
    # a periodic value: the match source starts in the dictionary and runs across the boundary into the value
    add("periodic", b"abc" * 20, (b"abc" * 40)[:100])
    add("periodic_long", b"abc" * 100, (b"abc" * 200)[:600])
    # the trigrams at D - 2 and D - 1 straddle the boundary: b"XYZ" and b"YZQ" exist nowhere else before
    # their repeats in the value
    # (fillers below 0x90: 8-bit codes in a fixed block, so these short members are never smaller stored and
    # their tokens stay visible to tests/test_gpu_dict.py)
    add("straddle", DISTINCT + b"XY", b"ZQR" + FILL1 + b"XYZQR" + FILL2)
    # b"abc" occurs only at the dictionary's position 0, which is never a candidate: all literals
    add("pos0", b"abc" + DISTINCT, FILL1 + b"abc" + FILL2)
    # ... while one byte in front of it makes it one
    add("pos1", b"#abc" + DISTINCT, FILL1 + b"abc" + FILL2)
    # the lazy rule decides at p = D: ml(D) = 3 (b"Zab"), ml(D + 1) = 10
    add("lazy", b"_abcdefghij" + b"!@#$%^&*()" + b"Zab?" + b"[]{}<>;:,.", b"Zabcdefghij~")
    # TOO_FAR: b"#$%" 4100 back into an 8192-byte dictionary is dropped, b"&*(" 4090 back is kept
    d = bytearray(alnum(rng, 8192))
    v = b"!@^_+#$%=~`|&*(;:,.?"
    d[8192 + 5 - 4100:8192 + 5 - 4100 + 3] = b"#$%"
    d[8192 + 12 - 4090:8192 + 12 - 4090 + 3] = b"&*("
    add("too_far", d, v)
    # a capped match (32) extended to 258 from a dictionary candidate
    d = alnum(rng, 1000)
    add("extend", d, d[200:500] + b"!")
    # hash collisions: b"\x20xy" twice uses up both candidate slots of b"\x00xy" with dictionary positions,
    # so b"\x00xyQRSTUV" goes unmatched at its first byte
    add("collide", b"#\x00xyQRSTUV" + b"0123" + b"\x20xy" + b"4567" + b"\x20xy" + b"89", b"\x00xyQRSTUV!")
    return P


# tests/golden/dict_baseline.json: a 2 KiB dictionary of eight 256-byte slices; 200 x 256 B and 100 x 1 KiB
BASELINE_DICT = (2048, 99)  # bytes, seed
BASELINE_SEED = 7
BASELINE_SETS = {"256": (256, 200), "1k": (1024, 100)}
FRAMING = 18  # gzip header and trailer bytes per member


def baseline_dictionary(corpus: bytes) -> bytes:
    size, seed = BASELINE_DICT
    return b"".join(json_slices(corpus, 256, size // 256, seed))


def baseline_values(corpus: bytes, name: str):
    size, count = BASELINE_SETS[name]
    return json_slices(corpus, size, count, BASELINE_SEED)


def crc0_bytes():
    """Four bytes whose CRC-32 is 0: the register must end at 0xFFFFFFFF, and the top byte of each register
    names the table entry of the step before it."""
    tab = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = 0xEDB88320 ^ (c >> 1) if c & 1 else c >> 1
        tab.append(c)
    want, idx = 0xFFFFFFFF, []
    for _ in range(4):
        k = next(n for n in range(256) if tab[n] >> 24 == want >> 24)
        idx.append(k)
        want = ((want ^ tab[k]) << 8) & 0xFFFFFFFF
    reg, out = 0xFFFFFFFF, bytearray()
    for k in reversed(idx):
        out.append((reg ^ k) & 0xFF)
        reg = tab[k] ^ (reg >> 8)
    assert zlib.crc32(bytes(out)) == 0
    return bytes(out)

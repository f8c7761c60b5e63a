"""The corpus of dictionary training (tests/dict_train_model.py): cases in which every rule of the algorithm
decides a byte of the result.  tests/test_dict_train_model.py asserts, from the model's own trace, that each case
does what its comment says; tests/test_host_dict_train.py and tests/test_gpu_dict_train.py compare the C++ check and
the kernels with the model on all of them.

A case is (name, src, offs, lens, D): sample k is src[offs[k]:offs[k] + lens[k]], as the C-ABI takes them."""
import numpy as np

from dict_train_model import SPAN, hash8
from fast_values import json_slices

SEEDED = (256, 2048, 12345)  # size, count, seed: the issue's sample set, JSON slices of the golden corpus
# CRC-32 of the model's dictionary for the seeded set, by D (the figures of the issue's prototype)
SEEDED_CRC = {64: 18057732, 2048: 1400053701, 8192: 1667123899}


class Case:
    def __init__(self, name, src, offs, lens, D):
        self.name, self.src, self.offs, self.lens, self.D = name, bytes(src), list(offs), list(lens), D

    @property
    def samples(self):
        return [self.src[o:o + n] for o, n in zip(self.offs, self.lens)]


def packed(name, samples, D, lead=0):
    """Samples back to back (so they abut, at whatever alignment their lengths give) behind `lead` filler bytes."""
    offs, at = [], lead
    for v in samples:
        offs.append(at)
        at += len(v)
    return Case(name, b"\xa5" * lead + b"".join(samples), offs, [len(v) for v in samples], D)


def noise(rng, n: int) -> bytes:
    """Random bytes: no 8 bytes twice (at these sizes), so every hashed position is worth its own count."""
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def distinct_noise(rng, n: int) -> bytes:
    """Random bytes whose hashed positions all fall into different slots (16375 positions among 2^20 slots would
    share some by chance): a byte that would land its position in a used slot is drawn again."""
    out, used = bytearray(noise(rng, 7)), set()
    while len(out) < n:
        out.append(int(rng.integers(0, 256)))
        h = hash8(out, len(out) - 8)
        if h in used:
            out.pop()
        else:
            used.add(h)
    return bytes(out)


def colliding_pair(rng):
    """Two different 8-byte strings with the same hash, by a birthday search over the 2^F slots."""
    seen = {}
    while True:
        x = noise(rng, 8)
        h = hash8(x, 0)
        if h in seen and seen[h] != x:
            return seen[h], x
        seen[h] = x


def seeded_samples(corpus: bytes):
    size, count, seed = SEEDED
    return json_slices(corpus, size, count, seed)


def small_cases():
    """{name: Case}, each built for one rule; what each must do is asserted in tests/test_dict_train_model.py."""
    rng = np.random.default_rng(20262)
    C = {}

    def add(case):
        assert case.name not in C
        C[case.name] = case

    T, R = noise(rng, 64), noise(rng, 64)
    # ---- sample lengths
    # 0 and 7 bytes hash nothing; the 8-byte sample's one position lifts T (58) over R (57), which comes first
    add(packed("len_0_7_8", [b"", R[:7], T[20:28], R, T], 64))
    # a 63-byte sample counts (56 positions of T) but is no candidate
    add(packed("len_63_counts", [R, T, T[:63]], 64))
    add(packed("len_63_only", [T[:63]] * 64, 2048))
    # 64 bytes: one candidate; 65 bytes: two, and the second one wins here (its 57 positions lie in the helper too)
    S65 = noise(rng, 65)
    add(packed("len_64_one", [T], 64))
    add(packed("len_65_second", [S65, S65[1:]], 64))
    # 16383 bytes: the last position (8 bytes from 16375) and the last start (16319) lie behind the span.  Five copies
    # of those 8 bytes would make that start the best; as the sample is cut, every start scores 57 and start 0 wins
    big = distinct_noise(rng, SPAN + 1)
    add(packed("len_16383_cut", [big] + [big[-8:]] * 5, 64))
    # ... and one byte shorter the same content counts
    add(packed("len_16382_whole", [big[1:]] + [big[-8:]] * 5, 64))
    # ---- the last start
    V = noise(rng, 200)
    add(packed("last_start", [V, V[-64:]], 64))
    # ---- window dedupe
    # period 2: two hash values, 29 + 28 times; each counts once (57), so the rival (57 + 10) wins; every position
    # counted, the periodic sample would score 29 * 29 + 28 * 28
    add(packed("period_2", [b"ab" * 32, R, R[:17]], 64))
    # period 56: position 56 repeats position 0, at the largest distance the window holds: it counts once (57), and
    # the rival (58) wins; counted twice it would score 59
    P56 = noise(rng, 56)
    add(packed("period_56", [P56 + P56[:8], R, R[8:16]], 64))
    # period 57: positions 0 and 57 never share a window; both starts score 58
    P57 = noise(rng, 57)
    add(packed("period_57", [R, P57 + P57[:8]], 64))
    # ---- ties
    add(packed("tie_samples", [T, T], 64))
    add(packed("tie_starts", [S65], 64))
    # ---- zeroing
    # epoch 1's sample holds T, the raw best, which epoch 0 took: it settles for the first start clear of T's slots
    U = noise(rng, 64)
    add(packed("zero_overlap", [T, T + U], 128))
    # the same 256 bytes 64 times over: 193 starts, but the slots run out after 6 segments
    X = noise(rng, 256)
    add(packed("zero_identical", [X] * 64, 2048))
    # epoch 1's only sample is what epoch 0 took: best score 0, nothing selected
    add(packed("zero_score", [T, T], 128))
    # ---- table collision: A holds X8, the three 8-byte samples are Y8 != X8 in X8's slot; that lifts A (60) over B
    # (57 + 2)
    X8, Y8 = colliding_pair(rng)
    A = X8 + noise(rng, 56)
    add(packed("collision", [R, R[30:38], R[40:48], A, Y8, Y8, Y8], 64))
    # ---- epoch partition: empty epochs (n < E), one sample each (n == E), uneven (7 over 4)
    Z = [noise(rng, 100) for _ in range(7)]
    add(packed("epochs_n_lt_E", Z[:3], 512))
    add(packed("epochs_n_eq_E", Z[:4], 256))
    add(packed("epochs_uneven",
               [Z[0], Z[1] + Z[0][10:90], Z[2], Z[3] + Z[2][:70], Z[4], Z[5], Z[6] + Z[4][20:95]], 256))
    # ---- offsets
    # the same samples at each alignment of the first byte
    for lead in range(4):
        add(packed(f"align_{lead}", [V, S65, V[-64:], T[:63], R], 128, lead=lead))
    # overlapping and abutting samples of one buffer, in an order that is not the buffer's
    add(Case("overlap", V + U, [50, 0, 100, 200, 136], [100, 100, 100, 64, 64], 128))
    # bytes outside a sample: each 63-byte sample T[:63] is followed by T[63]: reading one byte too many would make
    # it a candidate of score 57 * 5; as it is, R is the only candidate
    add(Case("outside", T * 5 + R, [0, 64, 128, 192, 256, 320], [63] * 5 + [64], 64))
    return C


def all_cases(corpus: bytes):
    """The small cases, then the seeded set at D = 64, 2048 and 8192."""
    out = list(small_cases().values())
    S = seeded_samples(corpus)
    for D in SEEDED_CRC:
        out.append(packed(f"seeded_{D}", S, D))
    return out


def case_file(cases) -> bytes:
    """The cases in the form tests/host/dict_train_check.cpp reads."""
    out = [np.uint32(len(cases)).tobytes()]
    for c in cases:
        out.append(np.array([len(c.lens), c.D], dtype="<u4").tobytes())
        out.append(np.array(c.lens, dtype="<u4").tobytes())
        out.append(b"".join(c.samples))
    return b"".join(out)

"""CPU: the model of dictionary training (tests/dict_train_model.py) on the corpus of tests/dict_train_values.py.
Every case is asserted from the model's own trace to do what it was built for, so that the C++ check and the kernels,
which are compared with the model on the same cases, are held to every rule."""
import json
import os
import zlib

import numpy as np
import pytest

import dict_train_model as M
from dict_train_values import SEEDED_CRC, all_cases, noise, packed, seeded_samples, small_cases
from dict_values import BASELINE_SETS, FRAMING, baseline_values

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    return small_cases()


@pytest.fixture(scope="module")
def traced(cases):
    return {name: M.train_trace(c.samples, c.D) for name, c in cases.items()}


@pytest.fixture(scope="module")
def seeded(golden):
    S = seeded_samples(golden.corpus)
    return S, {D: M.train(S, D) for D in SEEDED_CRC}


def raw_table(samples):
    freq = {}
    for v in samples:
        for x in M.hashes(v[:M.SPAN]):
            freq[x] = freq.get(x, 0) + 1
    return freq


def test_the_three_forms_of_the_score_agree(cases):
    """The definition, the per-position form the kernels use and the sliding form the model runs."""
    for name in ("period_2", "period_56", "period_57", "last_start", "collision", "epochs_uneven"):
        S = cases[name].samples
        freq = raw_table(S)
        for v in S:
            if len(v) < 64:
                continue
            h = M.hashes(v)
            nq = len(v) - 63
            direct = [M.score_direct(freq, h, q) for q in range(nq)]
            assert direct == [M.score_by_dist(freq, h, q) for q in range(nq)] == M.scores(freq, h, nq), name


def test_sample_lengths(cases, traced):
    S = cases["len_0_7_8"].samples
    assert [len(v) for v in S[:3]] == [0, 7, 8]
    assert traced["len_0_7_8"] == (S[4], [(58, 4, 0)])  # R, which comes first, has 57
    S = cases["len_63_counts"].samples
    assert traced["len_63_counts"] == (S[1], [(57 + 56, 1, 0)])
    assert traced["len_63_only"] == (b"", [None] * 32)
    assert traced["len_64_one"][1] == [(57, 0, 0)]
    S = cases["len_65_second"].samples
    assert traced["len_65_second"] == (S[0][1:], [(114, 0, 1)])
    # the cut: without it start 16319 would score 57 + 5, as it does in the sample that is one byte shorter
    S = cases["len_16383_cut"].samples
    assert len(S[0]) == 16383 and traced["len_16383_cut"] == (S[0][:64], [(57, 0, 0)])
    S = cases["len_16382_whole"].samples
    assert len(S[0]) == 16382 and traced["len_16382_whole"] == (S[0][-64:], [(62, 0, 16382 - 64)])


def test_last_start(cases, traced):
    S = cases["last_start"].samples
    assert traced["last_start"] == (S[0][-64:], [(114, 0, len(S[0]) - 64)])


def test_window_dedupe(cases, traced):
    def every_position(name, i):  # the score with every position counted
        S = cases[name].samples
        freq = raw_table(S)
        return sum(freq[x] for x in M.hashes(S[i])[:M.W])

    assert traced["period_2"][1] == [(67, 1, 0)] and every_position("period_2", 0) == 29 * 29 + 28 * 28 > 67
    assert traced["period_56"][1] == [(58, 1, 0)] and every_position("period_56", 0) == 59 > 58
    assert traced["period_57"][1] == [(58, 1, 0)]


def test_ties(cases, traced):
    assert traced["tie_samples"][1] == [(114, 0, 0)]
    S = cases["tie_starts"].samples
    assert traced["tie_starts"] == (S[0][:64], [(57, 0, 0)])
    freq = raw_table(S)
    assert M.scores(freq, M.hashes(S[0]), 2) == [57, 57]


def test_zeroing(cases, traced):
    S = cases["zero_overlap"].samples
    freq = raw_table(S)
    raw = M.scores(freq, M.hashes(S[1]), 65)
    assert raw.index(max(raw)) == 0 and raw[0] == 114       # the raw best is T, at start 0 ...
    d, tr = traced["zero_overlap"]
    assert tr == [(114, 0, 0), (57, 1, 57)]                 # ... and the pick is the first start clear of T's slots
    assert d == S[1][57:121] + S[0]
    d, tr = traced["zero_identical"]
    # 249 hashed positions, 57 zeroed per pick: starts 0, 57, 114, 171, then 192 for the last 21, then nothing
    assert len(d) == 320 and [t and t[2] for t in tr] == [0, 57, 114, 171, 192] + [None] * 27
    assert [t[0] for t in tr[:5]] == [64 * 57] * 4 + [64 * 21]
    assert traced["zero_score"] == (cases["zero_score"].samples[0], [(114, 0, 0), None])


def test_table_collision(cases, traced):
    S = cases["collision"].samples
    x, y = S[3][:8], S[4]
    assert x != y and M.hash8(x, 0) == M.hash8(y, 0)
    assert traced["collision"] == (S[3], [(60, 3, 0)])
    # with the three colliding samples replaced by bytes in other slots, R (59) wins
    other = packed("c", S[:4] + [bytes(8), bytes([1] * 8), bytes([2] * 8)], 64)
    assert M.train_trace(other.samples, 64)[1] == [(59, 0, 0)]


def test_epoch_partition(cases, traced):
    for name, n, E in (("epochs_n_lt_E", 3, 8), ("epochs_n_eq_E", 4, 4), ("epochs_uneven", 7, 4)):
        c = cases[name]
        d, tr = traced[name]
        assert (len(c.lens), c.D // 64, len(tr)) == (n, E, E)
        for e, t in enumerate(tr):
            lo, hi = e * n // E, (e + 1) * n // E
            assert (t is None) == (lo == hi), (name, e)
            assert t is None or lo <= t[1] < hi, (name, e)
    assert [t is not None for t in traced["epochs_n_lt_E"][1]] == [False, False, True, False, False, True, False, True]
    assert len(traced["epochs_n_lt_E"][0]) == 192
    # uneven: epochs of 1, 2, 2 and 2 samples, and the second sample of an epoch can win it
    assert [t[1] for t in traced["epochs_uneven"][1]] == [0, 2, 4, 5]


def test_offsets(cases, traced):
    assert {cases[f"align_{k}"].offs[0] % 4 for k in range(4)} == {0, 1, 2, 3}
    assert len({traced[f"align_{k}"][0] for k in range(4)}) == 1
    assert len(traced["align_0"][0]) == 128
    c = cases["overlap"]
    spans = sorted(zip(c.offs, c.lens))
    assert any(a + n > b for (a, n), (b, _) in zip(spans, spans[1:]))   # overlapping
    assert any(a + n == b for (a, n), (b, _) in zip(spans, spans[1:]))  # abutting
    assert c.offs != sorted(c.offs) and len(traced["overlap"][0]) == 128
    c = cases["outside"]
    assert traced["outside"] == (c.samples[5], [(57, 5, 0)])
    one_more = M.train_trace([c.src[o:o + 64] for o in c.offs], 64)   # what reading a byte too many would give
    assert one_more[1] == [(57 * 5, 0, 0)]


def test_seeded_set(seeded):
    S, dicts = seeded
    assert len(S) == 2048 and all(len(v) == 256 for v in S)
    for D, d in dicts.items():
        assert len(d) == D and zlib.crc32(d) == SEEDED_CRC[D], D
    assert len(M.train([S[0]] * 64, 2048)) == 384  # one JSON slice 64 times over: the zeroing ends it


def test_all_cases_are_valid_and_named_once(golden):
    cs = all_cases(golden.corpus)
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        assert M.valid(len(c.lens), c.D) and all(o + n <= len(c.src) for o, n in zip(c.offs, c.lens)), c.name
    assert {c.D for c in cs} >= {64, 2048, 8192}


def test_pure_function_and_permutation_within_an_epoch():
    """Twice the same; and samples reordered inside their epochs change the result only through the tie rule: with
    no ties the same segments are selected, with a tie the lower index wins."""
    rng = np.random.default_rng(5)
    b = [noise(rng, 90) for _ in range(8)]
    # (the copies are too short to be candidates: each epoch's best score belongs to one sample alone)
    S = [b[0], b[1], b[1][10:50], b[2], b[3], b[4][:30], b[4], b[5]]
    d, tr = M.train_trace(S, 128)  # two epochs of four samples
    assert M.train_trace(list(S), 128) == (d, tr)
    assert len({t[0] for t in tr}) == 2
    perm = [3, 1, 0, 2, 6, 7, 5, 4]
    d2, tr2 = M.train_trace([S[k] for k in perm], 128)
    assert d2 == d and [(s, perm[i], q) for s, i, q in tr2] == tr
    # a tie: the same sample twice in an epoch; whichever stands first is taken
    T = [S[1], S[0], S[1], S[3]]
    assert M.train_trace(T, 64)[1][0][1] == 0 and M.train_trace(T[::-1], 64)[1][0][1] == 1


def test_argument_bounds():
    assert M.valid(1, 64) and M.valid(M.MAX_SAMPLES, 8192)
    assert not any(M.valid(n, D) for n, D in ((0, 64), (M.MAX_SAMPLES + 1, 64), (1, 0), (1, 32), (1, 100), (1, 8256)))
    assert M.MAX_SAMPLES * M.SPAN < 1 << 32


def framed_total(vals, level, zdict):
    total = 0
    for v in vals:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict)
        total += len(c.compress(v) + c.flush()) + FRAMING
    return total


def test_trained_dictionary_beats_the_baseline_dictionary(golden, seeded):
    """Quality: zlib level 9 with the trained 2 KiB dictionary as zdict stores less on both baseline sets than with
    the baseline dictionary (15765 < 16460 and 22488 < 23119 when this was written), and the totals are the ones
    tests/golden/dict_train_baseline.json records."""
    d = seeded[1][2048]
    with open(os.path.join(GOLDEN, "dict_train_baseline.json")) as f:
        doc = json.load(f)
    with open(os.path.join(GOLDEN, "dict_baseline.json")) as f:
        base = json.load(f)
    assert (doc["dict_crc32"], doc["dict_len"], doc["dict_size"]) == (zlib.crc32(d), len(d), 2048)
    for name, (size, count) in BASELINE_SETS.items():
        assert (doc["sets"][name]["size"], doc["sets"][name]["count"]) == (size, count)
        assert doc["sets"][name]["level9_dict_total"] < base["sets"][name]["level9_dict_total"], name
    if zlib.ZLIB_RUNTIME_VERSION != "1.2.11":
        pytest.skip("the totals are zlib 1.2.11's")
    for name in BASELINE_SETS:
        vals = baseline_values(golden.corpus, name)
        for level in (1, 9):
            assert framed_total(vals, level, d) == doc["sets"][name][f"level{level}_dict_total"], (name, level)

"""CPU: the fast level's model (tests/fast_model.py) is a lossless parse on the whole edge list, the
level entry points refuse bad arguments without a device, and the recorded zlib baseline
(tests/golden/fast_baseline.json) is what zlib 1.2.11 produces."""
import ctypes
import importlib.util
import json
import os
import zlib

import pytest

import pmc_codec
from fast_model import CAPT, K, LAZY, fast_tokens, match_table, replay
from fast_values import LAZY_VALUE, edge_values

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_model_constants_match_the_kernel():
    src = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "poor-man-s-cache_amd", "csrc",
                            "pmc_deflate_fast.hip")).read()
    assert f"kFastK = {K}, kFastLazy = {LAZY}, kFastCap = {CAPT};" in src


def test_replay_rebuilds_every_edge_value(golden):
    vals = edge_values(golden.corpus)
    assert len({n for n, _ in vals}) == len(vals)
    for name, v in vals:
        toks = fast_tokens(v)
        assert replay(toks) == v, name
        for t in toks:
            if isinstance(t, tuple):
                assert 3 <= t[0] <= 258 and 1 <= t[1] <= 16382, (name, t)


def test_edge_values_hit_the_rules_they_are_built_for(golden):
    vals = dict(edge_values(golden.corpus))
    # lazy rule: at b"Z" ml = 3 (b"Zab"), at the next position ml = 10: literal, then the longer match
    toks = fast_tokens(LAZY_VALUE)
    at = len(LAZY_VALUE) - 12
    ml, _ = match_table(LAZY_VALUE)
    assert ml[at] == 3 and ml[at + 1] == 10
    assert toks[-3:] == [ord("Z"), (10, at), ord("~")]
    # TOO_FAR: the repeat 4190 back is dropped, the one 4090 back is kept
    v = vals["too_far"]
    ml, mq = match_table(v)
    assert ml[4200] == 0 and (ml[4190], 4190 - mq[4190]) == (3, 4090)
    # position 0 is not a candidate: b"abc" at 48 has none, b"bcdefgh" at 49 matches position 1
    ml, mq = match_table(vals["pos0"])
    assert ml[48] == 0 and (ml[49], mq[49]) == (7, 1)
    # capped matches are extended to 258 and chain
    assert fast_tokens(bytes(1024)) == [0, 0] + [(258, 1)] * 3 + [(248, 1)]
    # hash collisions use up candidate slots: some b"?xyQRSTUV" repeat goes unmatched
    c = vals["collide_long"]
    ml, _ = match_table(c)
    starts = [p for p in range(1, len(c) - 9) if c[p + 1:p + 9] == b"xyQRSTUV"]
    assert any(ml[p] >= 9 for p in starts[2:]) and any(ml[p] == 0 for p in starts[3:])
    # random [A-Za-z0-9] has (next to) no matches
    toks = fast_tokens(vals["alnum1024"])
    assert sum(isinstance(t, tuple) for t in toks) < 16


def test_level_calls_refuse_null_without_a_device():
    L = pmc_codec.lib()
    lvl = ctypes.c_int(77)
    assert L.pmc_ctx_set_level(None, pmc_codec.LEVEL_FAST) == pmc_codec.E_ARG
    assert L.pmc_ctx_set_level(None, pmc_codec.LEVEL_EXACT) == pmc_codec.E_ARG
    assert L.pmc_ctx_get_level(None, ctypes.byref(lvl)) == pmc_codec.E_ARG and lvl.value == 77
    assert L.pmc_group_set_level(None, pmc_codec.LEVEL_FAST) == pmc_codec.E_ARG
    assert (pmc_codec.LEVEL_EXACT, pmc_codec.LEVEL_FAST) == (9, 1)


def test_bad_pmc_level_fails_context_creation_before_any_device(monkeypatch):
    L = pmc_codec.lib()
    monkeypatch.setenv("PMC_LEVEL", "7")
    h = ctypes.c_void_p()
    assert L.pmc_ctx_create(0, ctypes.byref(h)) == pmc_codec.E_ARG and not h.value
    assert "PMC_LEVEL=7" in pmc_codec.last_error()


def test_recorded_baseline_is_what_zlib_1_2_11_gives():
    if zlib.ZLIB_RUNTIME_VERSION != "1.2.11":
        pytest.skip(f"zlib {zlib.ZLIB_RUNTIME_VERSION}: the baseline is stated for 1.2.11")
    spec = importlib.util.spec_from_file_location("make_fast_baseline", os.path.join(GOLDEN, "make_fast_baseline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "fast_baseline.json")) as f:
        doc = json.load(f)
    assert doc["zlib"] == "1.2.11"
    assert doc["sets"] == mod.totals(mod.corpus())
    for s in doc["sets"].values():
        assert s["level9_total"] < s["level1_total"]

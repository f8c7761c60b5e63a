"""CPU: the model of the fast level for large values (tests/fast_large_model.py) is a lossless parse of
every listed value, its matches stay inside their segments and within G + H - 1 bytes, its constants are
the kernel's, the new level is public and refused without a context, and the recorded zlib baseline
(tests/golden/fast_large_baseline.json) is what zlib 1.2.11 produces."""
import ctypes
import importlib.util
import json
import os
import zlib

import pytest

import pmc_codec
from fast_large_model import G, H, fast_large_segment_tokens, fast_large_tokens, replay_segments, segments
from fast_large_values import BIG_NAME, JSON_SIZES, M, STRADDLE_AT, STRADDLE_BACK, large_values
from fast_model import FAST_MAX, fast_tokens

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def values(golden):
    vals = large_values(golden.corpus)
    assert vals[-1][0] == BIG_NAME and len(vals[-1][1]) == 1 << 20
    assert len({n for n, _ in vals}) == len(vals)
    return vals[:-1]


def test_model_constants_match_the_kernel():
    src = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "poor-man-s-cache_amd", "csrc",
                            "pmc_deflate_fast_large.hip")).read()
    assert f"kFlSeg = {G}, kFlHist = {H};" in src
    assert G + H <= FAST_MAX


def test_value_list_is_the_one_the_level_is_stated_on(values):
    by = dict(values)
    assert [len(by[f"json{n}"]) for n in JSON_SIZES] == JSON_SIZES
    assert {16383, 2 * G, 2 * G + 1, 2 * G + 2, 2 * G + 3, 3 * G - 1, G + H, 40000, 65536, 100000} <= set(JSON_SIZES)
    # the same edges on the large path: around M segments, the fewest of a value above 16382 bytes
    assert (M - 1) * G <= FAST_MAX < M * G
    assert {M * G, M * G + 1, M * G + 2, M * G + 3, (M + 1) * G - 1} <= set(JSON_SIZES)
    assert by["a50000"] == b"a" * 50000
    p = by["period"]
    assert len(p) == 50000 and p[H + 904:] == p[:-(H + 904)]
    s = by["straddle"]
    at, back = STRADDLE_AT, STRADDLE_BACK
    assert at % G == 0 and back + 150 <= H and len(s) > FAST_MAX
    assert s[at - 150:at + 150] == s[at - back - 150:at - back + 150]
    assert len(by["random40000"]) == 40000
    # (lengths of at most 16382 bytes -- G + H always -- give plain fast members at the level)
    assert f"json{G + H}" in by and all(len(v) > FAST_MAX or n.startswith("json") for n, v in by.items())


def test_replay_rebuilds_every_value_and_matches_stay_in_their_segments(values):
    for name, v in values:
        seg_toks = fast_large_segment_tokens(v)
        assert len(seg_toks) == (len(v) + G - 1) // G, name
        assert replay_segments(v, seg_toks) == v, name
        for k, toks in enumerate(seg_toks):
            p = k * G
            for t in toks:
                if isinstance(t, tuple):
                    ln, dist = t
                    assert 3 <= ln <= 258 and 1 <= dist <= min(p, G + H - 1), (name, p, t)
                    assert (p + ln - 1) // G == k, (name, p, t)  # no match crosses a multiple of G
                    p += ln
                else:
                    p += 1
            assert p == min(len(v), (k + 1) * G), name


def test_values_hit_the_rules_they_are_built_for(values):
    by = dict(values)
    # 258-byte matches cut at the segment ends; from the second segment on the sources lie in the history
    segs = fast_large_segment_tokens(by["a50000"])
    assert (G - 2) % 258 >= 3 and G % 258 >= 3
    assert segs[0] == [97, 97] + [(258, 1)] * ((G - 2) // 258) + [((G - 2) % 258, 1)]
    assert segs[1] == [(258, 1)] * (G // 258) + [(G % 258, 1)]
    # a one-byte last segment is a literal; a three-byte one has one hashable position behind its history
    v = by[f"json{M * G + 1}"]
    assert fast_large_segment_tokens(v)[-1] == [v[-1]]
    # the repeat across the boundary: cut there, found again in the next segment
    s = by["straddle"]
    t0, t1 = fast_large_segment_tokens(s)[M - 1:M + 1]
    assert t0[-1] == (150, STRADDLE_BACK) and t1[0] == (150, STRADDLE_BACK)
    # a period of H + 904 bytes: the copy lies further back than the history, so only the positions from
    # 904 on in a segment reach it
    p = fast_large_segment_tokens(by["period"])
    dists = {t[1] for toks in p for t in toks if isinstance(t, tuple) and t[0] >= 32}
    assert dists == {H + 904}
    pos, long_at = 0, []
    for toks in p:
        for t in toks:
            if isinstance(t, tuple) and t[0] >= 32:
                long_at.append(pos)
            pos += t[0] if isinstance(t, tuple) else 1
    assert long_at[0] == H + 904 + 1  # (the copy's first byte would match position 0, never a candidate)
    assert all(x % G >= 904 for x in long_at)


def test_up_to_one_segment_the_parse_is_the_fast_level_s(golden):
    for n in (1, 2, 3, 1000, G - 1, G):
        v = golden.corpus[500:500 + n]
        assert segments(v) == [(b"", v)]
        assert fast_large_tokens(v) == fast_tokens(v), n


def test_the_level_is_public_and_refused_without_a_context():
    L = pmc_codec.lib()
    assert pmc_codec.LEVEL_FAST_ALL == 2
    assert L.pmc_ctx_set_level(None, 2) == pmc_codec.E_ARG
    assert L.pmc_group_set_level(None, 2) == pmc_codec.E_ARG
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "pmc_codec.h")).read()
    assert "#define PMC_LEVEL_FAST_ALL 2\n" in hdr


def test_pmc_level_names_the_new_level(monkeypatch):
    """PMC_LEVEL=fast-all / 2 are levels (a bad one is refused with the list); no device is touched."""
    L = pmc_codec.lib()
    monkeypatch.setenv("PMC_LEVEL", "fast-al")
    h = ctypes.c_void_p()
    assert L.pmc_ctx_create(0, ctypes.byref(h)) == pmc_codec.E_ARG and not h.value
    assert "fast-all, 2" in pmc_codec.last_error()


def test_recorded_baseline_is_what_zlib_1_2_11_gives():
    if zlib.ZLIB_RUNTIME_VERSION != "1.2.11":
        pytest.skip(f"zlib {zlib.ZLIB_RUNTIME_VERSION}: the baseline is stated for 1.2.11")
    spec = importlib.util.spec_from_file_location("make_fast_large_baseline",
                                                  os.path.join(GOLDEN, "make_fast_large_baseline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "fast_large_baseline.json")) as f:
        doc = json.load(f)
    assert doc["zlib"] == "1.2.11"
    assert doc["set"] == mod.totals(mod.corpus())
    assert doc["set"]["level9_total"] < doc["set"]["level1_total"]

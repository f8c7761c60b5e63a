"""CPU: the preset dictionary's model (tests/dict_model.py) is a lossless parse on the whole edge list and
is fast_model's without a dictionary, every pattern triggers the rule it is built for, the dictionary entry
points refuse bad arguments (and a bad PMC_DICT) without a device, and the recorded zlib baseline
(tests/golden/dict_baseline.json) is what zlib 1.2.11 produces."""
import ctypes
import importlib.util
import json
import os
import zlib

import pytest

import pmc_codec
from dict_model import dict_tokens, replay_with
from dict_values import DICT_SIZES, SPAN, VALUE_SIZES, crc0_bytes, edge_pairs, patterns, uses_dictionary
from fast_model import fast_tokens, match_table
from fast_values import edge_values

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reach(d, toks):
    """[(position in the value, token)] of the matches whose distance reaches into the dictionary."""
    out, p = [], 0
    for t in toks:
        if isinstance(t, tuple):
            if t[1] > p:
                out.append((p, t))
            p += t[0]
        else:
            p += 1
    return out


def test_replay_rebuilds_every_edge_value(golden):
    pairs = edge_pairs(golden.corpus)
    assert len({n for n, _, _ in pairs}) == len(pairs)
    assert len(pairs) == len(DICT_SIZES) * (len(VALUE_SIZES) + 2) + len(patterns(golden.corpus))
    used = 0
    for name, d, v in pairs:
        if not uses_dictionary(d, v):
            assert len(d) + len(v) == SPAN + 1, name
            continue
        toks = dict_tokens(d, v)
        assert replay_with(d, toks) == v, name
        p = 0
        for t in toks:
            if isinstance(t, tuple):
                assert 3 <= t[0] <= 258 and 1 <= t[1] <= p + len(d) - 1, (name, t)  # (never position 0)
                p += t[0]
            else:
                p += 1
        used += bool(reach(d, toks))
    # (a third of the dictionary sizes are 1..3 bytes, which a match can hardly reach, and one value per
    # dictionary is plain: the list is pointless unless at least a third of it reaches into its dictionary)
    assert used > len(pairs) // 3


def test_without_a_dictionary_it_is_the_fast_model(golden):
    for name, v in edge_values(golden.corpus):
        if len(v) <= 4097:
            assert dict_tokens(b"", v) == fast_tokens(v), name


def test_patterns_hit_the_rules_they_are_built_for(golden):
    P = patterns(golden.corpus)
    _, d, v = P["tail"]
    # (JSON repeats itself: the two nearest candidates may hide the copy 200 / 2048 back, but the first
    # token is a match into the dictionary either way)
    assert reach(d, dict_tokens(d, v))[0][0] == 0
    _, d, v = P["whole"]
    assert reach(d, dict_tokens(d, v))[0][0] == 0
    # the period-3 source starts in the dictionary and runs into the value
    _, d, v = P["periodic"]
    assert dict_tokens(d, v) == [(100, 3)]
    _, d, v = P["periodic_long"]
    assert dict_tokens(d, v) == [(258, 3), (258, 3), (84, 3)]
    # the straddling trigrams are the candidates: b"XYZQR" 19 bytes into the value matches position D - 2
    _, d, v = P["straddle"]
    D = len(d)
    ml, mq = match_table(d + v)
    assert (ml[D + 19], mq[D + 19]) == (5, D - 2) and (ml[D + 20], mq[D + 20]) == (4, D - 1)
    assert reach(d, dict_tokens(d, v)) == [(19, (5, 21))]
    # position 0 of the dictionary is no candidate; position 1 is
    _, d, v = P["pos0"]
    assert dict_tokens(d, v) == list(v)
    _, d, v = P["pos1"]
    assert reach(d, dict_tokens(d, v)) == [(16, (3, len(d) - 1 + 16))]
    # the lazy rule at p = D
    _, d, v = P["lazy"]
    D = len(d)
    ml, _ = match_table(d + v)
    assert ml[D] == 3 and ml[D + 1] == 10
    assert dict_tokens(d, v) == [ord("Z"), (10, D + 1 - 1), ord("~")]
    # TOO_FAR into the dictionary
    _, d, v = P["too_far"]
    D = len(d)
    ml, mq = match_table(d + v)
    assert ml[D + 5] == 0 and (ml[D + 12], D + 12 - mq[D + 12]) == (3, 4090)
    assert (12, (3, 4090)) in reach(d, dict_tokens(d, v))
    # a capped match extended to 258 from a dictionary candidate
    _, d, v = P["extend"]
    assert dict_tokens(d, v)[0] == (258, 800)
    # both candidate slots used up by colliding dictionary positions
    _, d, v = P["collide"]
    toks = dict_tokens(d, v)
    assert toks[0] == 0 and toks[1][0] == 8 and toks[1][1] > 1
    assert dict_tokens(d.replace(b"\x20xy", b"_xy"), v)[0][0] == 9  # (without the collisions: all of b"\x00xyQRSTUV")


def test_dictionary_calls_refuse_bad_arguments_without_a_device():
    L = pmc_codec.lib()
    i = ctypes.c_uint32(77)
    assert L.pmc_ctx_set_dictionary(None, b"abc", 3) == pmc_codec.E_ARG
    assert L.pmc_ctx_set_dictionary(None, None, 0) == pmc_codec.E_ARG
    assert L.pmc_ctx_get_dictionary_id(None, ctypes.byref(i)) == pmc_codec.E_ARG and i.value == 77
    assert L.pmc_group_set_dictionary(None, b"abc", 3) == pmc_codec.E_ARG
    assert pmc_codec.DICT_MAX == 8192


@pytest.mark.parametrize("case", ["missing", "empty", "oversized", "crc0"])
def test_bad_pmc_dict_fails_context_creation_before_any_device(monkeypatch, tmp_path, case):
    L = pmc_codec.lib()
    path = tmp_path / "dict.bin"
    if case == "empty":
        path.write_bytes(b"")
    elif case == "oversized":
        path.write_bytes(bytes(range(256)) * 32 + b"x")
    elif case == "crc0":
        path.write_bytes(crc0_bytes())
    monkeypatch.setenv("PMC_DICT", str(path))
    h = ctypes.c_void_p()
    assert L.pmc_ctx_create(0, ctypes.byref(h)) == pmc_codec.E_ARG and not h.value
    assert "PMC_DICT=" in pmc_codec.last_error()


def test_recorded_baseline_is_what_zlib_1_2_11_gives():
    if zlib.ZLIB_RUNTIME_VERSION != "1.2.11":
        pytest.skip(f"zlib {zlib.ZLIB_RUNTIME_VERSION}: the baseline is stated for 1.2.11")
    spec = importlib.util.spec_from_file_location("make_dict_baseline", os.path.join(GOLDEN, "make_dict_baseline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "dict_baseline.json")) as f:
        doc = json.load(f)
    assert doc["zlib"] == "1.2.11"
    want = mod.totals(mod.corpus())
    assert {k: doc[k] for k in want} == want
    for s in doc["sets"].values():
        assert s["level9_dict_total"] < s["level1_dict_total"] < s["level9_total"]

"""CPU: what tests/test_gpu_compress_bounds.py relies on, checked without a GPU.

Routes: every batch shape of tests/boundary_values.py goes through tests/host/plan_check's `route` mode and must
give the Route its GPU test means to reach (kind, passes, lv, gated) -- a shape that no longer reaches its route
fails here instead of passing on another route there.

Sensitivity: the windows are only worth their trouble where the neighbouring bytes could change a member.  In
every level-9 batch at least one third of the values must be right-sensitive (the last token of the oracle's
member is a match of length < 258 whose distance also fits the byte behind the value) and at least two thirds
left-sensitive (the first 3 bytes occur in the 32768 bytes before the value).  Conditions on the inputs, not
measurements: where a batch falls short, its windows change, not the shares.

Reference members: the oracle, greedy walk and dynamic-programming walk alike, reproduces the reference's own
member of every level-9 value (tests/golden/boundary_golden.json)."""
import pytest

import boundary_values as BV
from test_host_plan import EXACT, FAST, FAST_ALL, plan_bin, routes, row  # noqa: F401  (plan_bin: a fixture)


def lens_of(shape):
    return [w.n for w in BV.shape(shape)]


def route_rows():
    """(row id, shape) -> the RouteIn of that batch as the device entry builds it: `small` for a batch of at most
    1,024 values of at most 4 KiB (pmc_gzip_compress_batch), max_len the longest value."""
    out = {}
    for rid, r in BV.ROWS.items():
        for shape in r["shapes"]:
            lens = lens_of(shape)
            n, max_len = len(lens), max(lens)
            out[(rid, shape)] = row(n, max_len, r["level"], dict_len=BV.DICT_LEN if r.get("dict") else 0,
                                    small=n <= 1024 and max_len <= 4096,
                                    force_v1=1 if r.get("env") == "PMC_DEFLATE_V1" else -1,
                                    mono_env=1 if r.get("env") == "PMC_DEFLATE_MONO" else -1)
    return out


def test_shapes_hold_the_lengths_their_rows_name():
    L = {s: lens_of(s) for s in ("mono", "split-s12", "split", "big", "lv", "fast-dict", "fast-all", "fast-idx")}
    assert len(L["mono"]) == 192 and max(L["mono"]) == 4096 and set(BV.EDGE_4K) <= set(L["mono"])
    assert len(L["split-s12"]) == 1100 and max(L["split-s12"]) == 4096 and set(BV.EDGE_4K) <= set(L["split-s12"])
    assert len(L["split"]) == 96 and max(L["split"]) == 16382 and set(BV.EDGE_16K + BV.EDGE_4K) <= set(L["split"])
    assert len(L["big"]) == 6 and min(L["big"]) == 16383 and max(L["big"]) == BV.BIG_MAX
    assert set(BV.EDGE_BIG) <= set(L["big"]) and BV.BIG_RANDOM in L["big"]
    big = [n for n in L["lv"] if n > 16382]
    assert len(big) == 12 and min(big) == 32505 and max(big) == 100001 and set(BV.EDGE_LV) <= set(big)
    assert len(L["lv"]) == 16 and max(n for n in L["lv"] if n <= 16382) == 16382
    assert len(L["fast-dict"]) == 111 and max(L["fast-dict"]) == 16382 and set(BV.EDGE_DICT) <= set(L["fast-dict"])
    assert {BV.DICT_EDGE - 1, BV.DICT_EDGE, BV.DICT_EDGE + 1} | set(BV.EDGE_16K + BV.EDGE_4K) == set(BV.EDGE_DICT)
    assert len(L["fast-all"]) == 14 and min(L["fast-all"]) == 16383 and max(L["fast-all"]) == 100001
    assert set(BV.EDGE_BIG + BV.EDGE_LV) <= set(L["fast-all"])
    for s in ("mono", "split-s12", "split", "fast-dict"):  # each edge length on each of the five streams
        ws = BV.shape(s)
        edges = BV.EDGE_DICT if s == "fast-dict" else BV.EDGE_16K + BV.EDGE_4K if s == "split" else BV.EDGE_4K
        assert all({w.name for w in ws if w.n == n} == set(BV.STREAM_NAMES) for n in edges), s
    assert len(L["fast-idx"]) == 8 and min(L["fast-idx"]) == 32769 and max(L["fast-idx"]) == 100001
    assert len(BV.dictionary()) == BV.DICT_LEN


@pytest.mark.parametrize("shape", ["mono", "split-s12", "split", "big", "lv", "lv-json", "fast-dict", "fast-all", "fast-idx"])
def test_windows_lie_inside_their_streams_at_every_alignment(shape):
    ws = BV.shape(shape)
    for w in ws:
        assert w.a >= 32768 + 64 and w.a + w.n + 258 + 64 <= len(BV.streams()[w.name]), w
        assert BV.value(w) == BV.stream_of(w)[w.a:w.a + w.n] and len(BV.value(w)) == w.n
    for r in (w for w in ws if w.random):  # the bytes written over the stream lie outside every other window's reach
        assert all(o is r or o.name != r.name or o.a + o.n + 258 + 64 <= r.a or r.a + r.n <= o.a - 32768 - 64 for o in ws)
    assert {w.a % 4 for w in ws} == {0, 1, 2, 3}
    if shape == "lv-json":  # (four hand-picked windows: the other alignments are the other shapes' business)
        return
    assert {w.off % 4 for w in ws} == {0, 1, 2, 3}  # (the streams are 4-byte aligned in the source buffer)
    assert len({w.a % 16 for w in ws}) >= min(len(ws), 8)
    assert {w.n % 4 for w in ws} == {0, 1, 2, 3}
    if len(ws) >= 10:
        assert {w.name for w in ws} == set(BV.STREAM_NAMES)


def test_every_row_reaches_its_route(plan_bin):  # noqa: F811
    rows = route_rows()
    got = dict(zip(rows, routes(plan_bin, list(rows.values()))))
    small_pass = [[0, 16382, 16382, 0, 0]]

    def check(key, kind, passes, lv, gated, **more):
        g = got[key]
        assert (g["kind"], g["passes"], g["lv"], g["gated"]) == (kind, passes, lv, gated), (key, g)
        for k, v in more.items():
            assert g[k] == v, (key, k, g)

    # the device one-kernel path (deflate_small_kernel), gated retry pass behind it
    check(("mono", "mono"), "mono", [], 0, 1, lds_cut=4096, rlist=1)
    # the split pipeline, working sets of the 4 KiB class
    check(("split-s12", "split-s12"), "split", [[0, 4096, 4096, 0, 0]], 0, 1)
    check(("split", "split"), "split", small_pass, 0, 1)
    # small pass and large pass; the HBM kernel gated (it redoes the large pass's multi-block value)
    check(("big", "big"), "split", small_pass + [[16382, BV.BIG_MAX, BV.BIG_MAX, 0, 0]], 0, 1, hbm_cut=BV.BIG_MAX, rlist=1)
    # the large-value rounds above 16382, the small pass below
    check(("lv", "lv"), "split", small_pass, 1, 1, hbm_cut=16382, rlist=1)
    check(("lv", "lv-json"), "split", small_pass, 1, 1, hbm_cut=16382, rlist=1)
    # PMC_DEFLATE_V1: deflate_kernel<false> up to its LDS limit, deflate_kernel<true> by length above it
    check(("v1", "mono"), "v1", [], 0, 1, lds_cut=4096)
    check(("v1", "split"), "v1", [], 0, 0, lds_cut=13647, hbm_cut=13647)
    check(("v1", "lv"), "v1", [], 0, 0, lds_cut=13647, hbm_cut=13647)
    # PMC_DEFLATE_MONO: the one-kernel path at full cap
    check(("mono-env", "split"), "mono", [], 0, 1, lds_cut=16382, cap=16382)
    # the fast front; with the dictionary a pass of its own up to 12286
    check(("fast", "split"), "split", [[0, 16382, 16382, 1, 0]], 0, 1, fast_all=0)
    check(("fast-dict", "fast-dict"), "split", [[0, BV.DICT_EDGE, 12288, 1, 1], [BV.DICT_EDGE, 16382, 16382, 1, 0]], 0, 1,
          dict_len=BV.DICT_LEN)
    # the fast level's large rounds (no small value in these batches, the small pass finds nothing)
    for rid in ("fast-all", "fast-idx", "fast-idx-crc"):
        check((rid, BV.ROWS[rid]["shapes"][0]), "split", [[0, 16382, 16382, 1, 0]], 1, 1, fast_all=1, hbm_cut=16382)
    assert len(rows) == 15


@pytest.fixture(scope="module")
def members():
    """{shape: [(window, value, the oracle's member)]} of the level-9 shapes, computed once."""
    from oracle import pyoracle as O
    return {s: [(w, BV.value(w), O.compress(BV.value(w))) for w in BV.shape(s)] for s in BV.LEVEL9_SHAPES}


@pytest.mark.parametrize("shape", BV.LEVEL9_SHAPES)
def test_level9_batches_are_sensitive_to_their_neighbours(members, shape):
    ms = members[shape]
    right = sum(BV.right_sensitive(w, m) for w, _, m in ms)
    left = sum(BV.left_sensitive(w) for w, _, _ in ms)
    print(f"{shape}: {len(ms)} values, right-sensitive {right} ({right / len(ms):.2f}), left-sensitive {left} "
          f"({left / len(ms):.2f})")
    assert 3 * right >= len(ms), (shape, right, len(ms))
    assert 3 * left >= 2 * len(ms), (shape, left, len(ms))
    if shape == "lv-json":  # every one: the GPU test reads a retry of any of them as a parse that left its value
        assert right == left == len(ms) == 4 and all(w.name == "json" and w.n > 32506 for w, _, _ in ms)


def test_sensitivity_is_about_the_neighbours():
    """The two predicates on hand-made cases: they look at the bytes outside the value, and only there."""
    from oracle import pyoracle as O
    assert BV.left_sensitive(next(w for w in BV.shape("mono") if w.name == "p1" and w.n == 261))
    short = next(w for w in BV.shape("mono") if w.name == "p1" and w.n == 2)
    assert not BV.left_sensitive(short) and not BV.right_sensitive(short, O.compress(BV.value(short)))
    w260 = next(w for w in BV.shape("mono") if w.name == "p1" and w.n == 260)
    assert not BV.right_sensitive(w260, O.compress(BV.value(w260)))  # (its last token is a match of 258 or a literal)
    w100 = BV.Window("p2", BV.LEFT + 7, 100)
    assert BV.right_sensitive(w100, O.compress(BV.value(w100)))  # ('a' 'b', then one match of 98 at distance 2)
    rnd = next(w for w in BV.shape("big") if w.random)
    assert not BV.right_sensitive(rnd, O.compress(BV.value(rnd)))  # (stored blocks: no token at all)


def test_oracle_reproduces_the_reference_members(members):
    from oracle import pyoracle as O
    G = BV.BoundaryGolden()
    for shape, ms in members.items():
        vals = [v for _, v, _ in ms]
        assert G.mismatches(vals, [m for _, _, m in ms]) == [], shape
        assert G.mismatches(vals, [O.compress(v, dp=True) for v in vals]) == [], (shape, "dp")

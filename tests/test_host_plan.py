"""CPU: the planning arithmetic of a compress and of a decompress call (csrc/pmc_plan.hpp), printed by
tests/host/plan_check.cpp, equals a restatement of the formulas the host code had before the planner existed:
the large-value rounds of both levels (counts, table and scratch offsets, filled tables, round splitting under
a budget), the split pipeline's chunk-array layout, the compress route (which path claims which lengths), and
the decompress plan (the wave-only route, which stages run, their grids, groups and scratch sizes).  The
restatement below is written from those formulas, not from pmc_plan.hpp."""
import itertools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from fast_large_model import G as FL_SEG  # the fast level's segment bytes (kFlSeg)

HERE = os.path.dirname(os.path.abspath(__file__))

LV_SEG, LV_OVERLAP, LV_CHUNK = 16384, 2048, 4096
SPLIT_ROWS, MERGE_ROWS, HDR_WORDS, ORDER_BINS = 336, 572, 76, 2048
BUDGET = 24 << 30
U32MAX = 4294967295

EXACT_LENS = [16383, 16386, 16387, 32767, 32768, 32769, 49151, 49152, 150001, 4 << 20]
FAST_LENS = [16383, 16384, 16385, 18432, 18433, 1 << 20]


@pytest.fixture(scope="module")
def plan_bin():
    d = tempfile.mkdtemp(prefix="pmc_plan_")
    exe = os.path.join(d, "plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "host", "plan_check.cpp")])
    return exe, d


def al(x):
    return (x + 255) & ~255


# ---- large-value rounds, restated -------------------------------------------------------------------------
class Exact:
    fast_seg = 0

    @staticmethod
    def nseg(n):
        return max(1, n // LV_SEG)

    @staticmethod
    def nch(n):
        return (n - 2 + LV_CHUNK - 1) // LV_CHUNK

    @staticmethod
    def caps(n):
        """token capacity of each segment of a value of n bytes"""
        ns = Exact.nseg(n)
        c = np.full(ns, LV_SEG + LV_OVERLAP + 2, dtype=np.uint64)
        c[ns - 1] = n - (ns - 1) * LV_SEG + 2
        return c

    @staticmethod
    def cost(n):
        ns = Exact.nseg(n)
        tok = (ns - 1) * (LV_SEG + LV_OVERLAP + 2) + (n - (ns - 1) * LV_SEG) + 2
        return 13 * (n - 2) + 4 * tok + ns * (2 * LV_OVERLAP * 4 + 16) + Exact.nch(n) * 1024 + 64


class Fast:
    fast_seg = FL_SEG

    @staticmethod
    def nseg(n):
        return (n + FL_SEG - 1) // FL_SEG

    @staticmethod
    def nch(n):
        return 0

    @staticmethod
    def caps(n):
        ns = Fast.nseg(n)
        c = np.full(ns, FL_SEG, dtype=np.uint64)
        c[ns - 1] = n - (ns - 1) * FL_SEG
        return c

    @staticmethod
    def cost(n):
        return 4 * n + Fast.nseg(n) * 32 + 64


def want_rounds(mode, vals, budget):
    """vals: sorted (index, length).  The rounds as lists of values: take while need + cost <= budget, the
    first always."""
    rounds, v0 = [], 0
    while v0 < len(vals):
        v1, need = v0, 0
        while v1 < len(vals) and (v1 == v0 or need + mode.cost(vals[v1][1]) <= budget):
            need += mode.cost(vals[v1][1])
            v1 += 1
        rounds.append(vals[v0:v1])
        v0 = v1
    return rounds


def want_round(mode, rv):
    """Counts, regions as (name, offset, bytes) and the tables of one round of values rv."""
    nv = len(rv)
    lens = [n for _, n in rv]
    nseg, nch = sum(mode.nseg(n) for n in lens), sum(mode.nch(n) for n in lens)
    caps = np.concatenate([mode.caps(n) for n in lens])
    tb = int(caps.sum(dtype=np.uint64))
    segs = np.array([mode.nseg(n) for n in lens], dtype=np.uint64)
    t = {"val": np.array([i for i, _ in rv], dtype=np.uint32),
         "seg0": np.concatenate([[0], np.cumsum(segs)]).astype(np.uint32),
         "seg_val": np.repeat(np.arange(nv, dtype=np.uint32), segs.astype(np.int64)),
         "seg_tok0": (np.cumsum(caps, dtype=np.uint64) - caps).astype(np.uint64)}
    if mode is Exact:
        P = sum(n - 2 for n in lens)
        chs = np.array([mode.nch(n) for n in lens], dtype=np.uint64)
        pos = np.array([n - 2 for n in lens], dtype=np.uint64)
        t["pbase"] = (np.cumsum(pos, dtype=np.uint64) - pos).astype(np.uint64)
        t["ch0"] = np.concatenate([[0], np.cumsum(chs)]).astype(np.uint32)
        t["ch_val"] = np.repeat(np.arange(nv, dtype=np.uint32), chs.astype(np.int64))
        o_val = 0
        o_pb = al(o_val + 4 * nv)
        o_seg0 = al(o_pb + 8 * nv)
        o_ch0 = al(o_seg0 + 4 * (nv + 1))
        o_sval = al(o_ch0 + 4 * (nv + 1))
        o_stok = al(o_sval + 4 * nseg)
        o_cval = al(o_stok + 8 * nseg)
        tab_bytes = al(o_cval + 4 * nch)
        tab = [("val", o_val, 4 * nv), ("pbase", o_pb, 8 * nv), ("seg0", o_seg0, 4 * (nv + 1)),
               ("ch0", o_ch0, 4 * (nv + 1)), ("seg_val", o_sval, 4 * nseg), ("seg_tok0", o_stok, 8 * nseg),
               ("ch_val", o_cval, 4 * nch)]
        b_tmp = 0
        b_S = al(b_tmp + 4 * P)
        b_R = al(b_S + 4 * P)
        b_HC = al(b_R + 4 * P)
        b_hist = al(b_HC + P)
        b_tok = al(b_hist + 1024 * nch)
        b_map = al(b_tok + 4 * tb)
        b_stok = al(b_map + 2 * LV_OVERLAP * 4 * nseg)
        b_fail = al(b_stok + 16 * nseg)
        scratch_bytes = al(b_fail + 4 * nv)
        scratch = [("tmp", b_tmp, 4 * P), ("S", b_S, 4 * P), ("R", b_R, 4 * P), ("HC", b_HC, P),
                   ("hist", b_hist, 1024 * nch), ("tok", b_tok, 4 * tb), ("map", b_map, 2 * LV_OVERLAP * 4 * nseg),
                   ("seg_tok", b_stok, 16 * nseg), ("fail", b_fail, 4 * nv)]
    else:
        P = 0
        o_val = 0
        o_seg0 = al(o_val + 4 * nv)
        o_sval = al(o_seg0 + 4 * (nv + 1))
        o_stok = al(o_sval + 4 * nseg)
        tab_bytes = al(o_stok + 8 * nseg)
        tab = [("val", o_val, 4 * nv), ("seg0", o_seg0, 4 * (nv + 1)), ("seg_val", o_sval, 4 * nseg),
               ("seg_tok0", o_stok, 8 * nseg)]
        b_tok = 0
        b_stok = al(b_tok + 4 * tb)
        b_fail = al(b_stok + 16 * nseg)
        scratch_bytes = al(b_fail + 4 * nv)
        scratch = [("tok", b_tok, 4 * tb), ("seg_tok", b_stok, 16 * nseg), ("fail", b_fail, 4 * nv)]
    return {"nv": nv, "nseg": nseg, "nch": nch, "P": P, "tb": tb, "maxlen": max(lens), "tab": tab,
            "tab_bytes": tab_bytes, "scratch": scratch, "scratch_bytes": scratch_bytes, "tables": t, "caps": caps}


TAB_NAMES = ["val", "pbase", "seg0", "ch0", "seg_val", "seg_tok0", "ch_val"]
SCRATCH_NAMES = ["tmp", "S", "R", "HC", "hist", "tok", "map", "seg_tok", "fail"]
TAB_DTYPE = {"val": "<u4", "pbase": "<u8", "seg0": "<u4", "ch0": "<u4", "seg_val": "<u4", "seg_tok0": "<u8", "ch_val": "<u4"}


def run_lv(plan_bin, mode, vals, budget, tag):
    exe, d = plan_bin
    prefix = os.path.join(d, tag + "_")
    out = subprocess.run([exe, "lv", str(mode.fast_seg), str(budget), prefix] + [f"{i}:{n}" for i, n in vals],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rounds = [json.loads(ln) for ln in out.stdout.splitlines()]
    return rounds, [np.fromfile(f"{prefix}{k}.bin", dtype=np.uint8) for k in range(len(rounds))]


def check_regions(regions, total):
    """256-aligned, in order, not overlapping, inside the total (regions of no bytes take no space)"""
    end = 0
    for name, off, size in regions:
        assert off % 256 == 0, (name, off)
        if size:
            assert off >= end, (name, off, end)
            end = off + size
    assert end <= total and total % 256 == 0


def check_lv(plan_bin, mode, vals, budget, tag):
    """Every round plan_check prints for vals under budget equals the restatement's; returns the rounds."""
    vals_sorted = sorted(vals)
    want = want_rounds(mode, vals_sorted, budget)
    got, images = run_lv(plan_bin, mode, vals, budget, tag)
    assert [(g["v0"], g["v1"]) for g in got] == [(sum(len(r) for r in want[:k]), sum(len(r) for r in want[:k + 1]))
                                                  for k in range(len(want))]
    for g, img, rv in zip(got, images, want):
        w = want_round(mode, rv)
        for key in ("nv", "nseg", "nch", "P", "tb", "maxlen", "tab_bytes", "scratch_bytes"):
            assert g[key] == w[key], (key, g[key], w[key])
        g_tab, g_scr = dict(zip(TAB_NAMES, g["tab"])), dict(zip(SCRATCH_NAMES, g["scratch"]))
        for name, off, size in w["tab"]:
            assert g_tab[name] == off, (name, g_tab[name], off)
        for name, off, size in w["scratch"]:
            assert g_scr[name] == off, (name, g_scr[name], off)
        # the plan's own regions (all of them, whatever the level) with the restatement's sizes
        sizes = {name: size for name, off, size in w["tab"] + w["scratch"]}
        check_regions([(nm, g_tab[nm], sizes.get(nm, 0)) for nm in TAB_NAMES], g["tab_bytes"])
        check_regions([(nm, g_scr[nm], sizes.get(nm, 0)) for nm in SCRATCH_NAMES], g["scratch_bytes"])
        assert len(img) == g["tab_bytes"]
        for name, off, size in w["tab"]:
            table = np.frombuffer(img[off:off + size].tobytes(), dtype=TAB_DTYPE[name])
            assert np.array_equal(table, w["tables"][name]), name
        t = w["tables"]
        stok = np.frombuffer(img[g_tab["seg_tok0"]:g_tab["seg_tok0"] + 8 * g["nseg"]].tobytes(), dtype="<u8")
        assert stok[0] == 0 and np.array_equal(np.diff(stok), w["caps"][:-1]) and (w["caps"] > 0).all()
        assert int(stok[-1] + w["caps"][-1]) == g["tb"]
        assert t["seg0"][-1] == g["nseg"]
        if mode is Exact:
            assert t["ch0"][-1] == g["nch"]
    return want


@pytest.mark.parametrize("mode,lens", [(Exact, EXACT_LENS), (Fast, FAST_LENS)], ids=["exact", "fast"])
def test_large_rounds_match_the_restated_formulas(plan_bin, mode, lens):
    for k, n in enumerate(lens):  # each edge length alone, then all of them in one call
        assert len(check_lv(plan_bin, mode, [(7 + k, n)], BUDGET, f"{mode.__name__}_one{k}")) == 1
    assert len(check_lv(plan_bin, mode, [(3 * k + 1, n) for k, n in enumerate(lens)], BUDGET, f"{mode.__name__}_all")) == 1


@pytest.mark.parametrize("mode", [Exact, Fast], ids=["exact", "fast"])
def test_large_round_of_the_longest_value(plan_bin, mode):
    """4294967295 bytes alone: the arithmetic is 64-bit (the exact level's cost is above the budget)"""
    (rv,) = check_lv(plan_bin, mode, [(123456, U32MAX)], BUDGET, f"{mode.__name__}_max")
    assert rv == [(123456, U32MAX)]
    if mode is Exact:
        assert mode.cost(U32MAX) > BUDGET


@pytest.mark.parametrize("mode,lens", [(Exact, EXACT_LENS), (Fast, FAST_LENS)], ids=["exact", "fast"])
def test_large_round_splitting(plan_bin, mode, lens):
    # three values of every length, batch indices interleaved so that the sorted order is not the given one
    vals = [((k * 7 + 5 * c) % 31 + 31 * c, n) for c in range(3) for k, n in enumerate(lens)]
    assert len({i for i, _ in vals}) == len(vals)
    costs = [mode.cost(n) for _, n in vals]
    total, biggest = sum(costs), max(costs)
    # (total - 1: everything but the last value fits the first round)
    for tag, budget, rounds in (("one", BUDGET, 1), ("two", total - 1, 2), ("many", biggest, None),
                                ("under", biggest - 1, None), ("each", 1, len(vals))):
        want = check_lv(plan_bin, mode, vals, budget, f"{mode.__name__}_split_{tag}")
        assert [v for r in want for v in r] == sorted(vals)
        assert all(len(r) >= 1 for r in want)
        assert all(len(r) == 1 or sum(mode.cost(n) for _, n in r) <= budget for r in want)
        if rounds is not None:
            assert len(want) == rounds, (tag, len(want))
        else:
            assert len(want) > 2
        if tag == "under":
            assert any(sum(mode.cost(n) for _, n in r) > budget for r in want)


# ---- split chunk layout, restated -------------------------------------------------------------------------
def want_carve(pcap, chunk):
    blocks, off, p = chunk // 64, {}, 0
    for name, size in (("cT", chunk * pcap * 4), ("cN", chunk * 4), ("cP", chunk * 4), ("cG", blocks * 64 * MERGE_ROWS * 4),
                       ("cH", blocks * 64 * SPLIT_ROWS * 2), ("cL", blocks * 64 * SPLIT_ROWS),
                       ("cB", blocks * 64 * HDR_WORDS * 4), ("cC", chunk * 4), ("cD", (chunk + 1) * 4), ("cZ", chunk * 4),
                       ("ord", chunk * 4), ("obins", ORDER_BINS * 4)):
        off[name] = p
        p += size
    off["cQ"] = p
    return off


def want_scratch_of(c, ch):
    blocks = ch // 64
    return (ch * c * 4 + ch * 4 + ch * 4 + blocks * 64 * SPLIT_ROWS * 3 + blocks * 64 * MERGE_ROWS * 4 +
            blocks * 64 * HDR_WORDS * 4 + ch * 4 + (ch + 1) * 4 + ch * 8 + ORDER_BINS * 4 + 64 + 1024)


def want_value_bytes(cap):
    return cap * 4 + 4 + SPLIT_ROWS * 2 + SPLIT_ROWS + 4 + MERGE_ROWS * 4 + 4 + 8


def want_chunk_of(n, budget, cap):
    ch = min(n, max(4096, budget // want_value_bytes(cap)))
    return (ch + 63) & ~63


@pytest.mark.parametrize("pcap", [64, 512, 1024, 4096, 16384])
@pytest.mark.parametrize("chunk", [64, 4096, (10_000_000 + 63) & ~63])
def test_split_chunk_layout(plan_bin, pcap, chunk):
    got = json.loads(subprocess.check_output([plan_bin[0], "layout", str(pcap), str(chunk)]))
    want = want_carve(pcap, chunk)
    assert {k: got[k] for k in want} == want
    assert got["bytes"] == want_scratch_of(pcap, chunk)
    assert got["cB"] % 16 == 0
    assert got["cQ"] + 8 <= got["bytes"]


def test_split_chunk_sizes(plan_bin):
    """values per chunk: the budget over split_value_bytes(cap), as tests/test_gpu_fullsize.py sizes its budgets"""
    for n, mb, cap in ((200_000, 400, 1024), (200_000, 200, 256), (200_000, 1000, 4096), (1_000_000, 1500, 1024),
                       (200_000, 16384, 1024), (10_000_000, 98304, 1024), (1000, 98304, 16382), (5000, 1, 16382), (1, 1, 64)):
        got = json.loads(subprocess.check_output([plan_bin[0], "chunk", str(n), str(mb << 20), str(cap)]))
        assert got == {"chunk": want_chunk_of(n, mb << 20, cap), "value_bytes": want_value_bytes(cap)}


# ---- the route, restated ----------------------------------------------------------------------------------
EXACT, FAST, FAST_ALL = 9, 1, 2
CUS = 256
SMALL_LIM, BIG_LIM = 16382, 31808
V1_LIM = 13647      # deflate_lds_limit() of this build: the general kernel's LDS working set within 160 KiB
SMALL_MAX = 16382   # kSmallMax
DICT_SPAN = 16382   # kDictSpan


def hbm_wb_of(max_len):
    """stands in for deflate_wave_bytes(true, max_len): ~21 bytes of HBM working set per byte of value"""
    return 21 * max_len + 16384


def want_route(n, max_len, level, lane_ok, dict_len, cus, latency, small, force_v1, mono_env, big_env,
               small_lim_in, big_lim_in, v1_lim, small_max, hbm_wb):
    fast = level in (FAST, FAST_ALL) and lane_ok and not force_v1
    fast_all = fast and level == FAST_ALL
    dD = dict_len if fast else 0
    mono = not fast and (mono_env or latency or small or not lane_ok)
    split = not force_v1 and not mono
    small_lim = 0 if force_v1 else small_lim_in
    big_lim = big_lim_in if split else small_lim
    lds_cut = min(v1_lim, max(max_len, 1)) if force_v1 else min(small_lim, max(max_len, 1))
    cap = min((lds_cut + 63) & ~63, v1_lim if force_v1 else small_lim)
    big_pick = big_env != 0 if big_env >= 0 else (n <= 2 * cus and max_len <= big_lim)
    big_pass = split and not fast_all and big_pick and max_len > small_lim and big_lim > small_lim
    big_hi = min(big_lim, max_len) if big_pass else 0
    big_cap = min((big_hi + 63) & ~63, big_lim) if big_pass else 0
    hbm_cut = big_hi if big_pass else lds_cut
    lv = not force_v1 and max_len > hbm_cut
    hbm_waves = 0
    gated = not (force_v1 and max_len > hbm_cut)
    if not gated or not latency:
        cap_waves = 64 if gated and max_len <= small_max else cus * 8
        hbm_waves = max(1, min(cap_waves, ((8 if gated else 32) << 30) // max(hbm_wb, 1)))
    hbm_waves = min(hbm_waves, n)
    passes = []
    if split:
        if dD:
            dict_hi = min(lds_cut, DICT_SPAN - dD)
            dict_cap = min(cap, (dict_hi + 63) & ~63)
            passes.append([0, dict_hi, dict_cap, 1, 1])
            if lds_cut > dict_hi:
                passes.append([dict_hi, lds_cut, cap, 1, 0])
        else:
            passes.append([0, lds_cut, cap, int(fast), 0])
        if big_pass:
            passes.append([small_lim, big_hi, big_cap, 0, 0])
    return {"kind": "split" if split else "v1" if force_v1 else "mono", "passes": passes, "lds_cut": lds_cut, "cap": cap,
            "dict_len": dD, "lv": int(lv), "fast_all": int(fast_all), "hbm_cut": hbm_cut, "gated": int(gated),
            "rlist": int(gated and hbm_waves > 0), "hbm_waves": hbm_waves}


def routes(plan_bin, rows):
    text = "".join(" ".join(str(int(x)) for x in row) + "\n" for row in rows)
    out = subprocess.run([plan_bin[0], "route"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def row(n, max_len, level, lane_ok=True, dict_len=0, latency=False, small=False, force_v1=-1, mono_env=-1, big_env=-1):
    # (PMC_DEFLATE_V1 / PMC_DEFLATE_MONO: unset (-1) and 0 are both "off")
    return (n, max_len, level, lane_ok, dict_len, CUS, latency, small, force_v1 == 1, mono_env == 1, big_env,
            SMALL_LIM, BIG_LIM, V1_LIM, SMALL_MAX, hbm_wb_of(max_len))


def claims(r, max_len):
    """the (lo, hi] intervals of lengths each path of route r claims"""
    c = [(lo, hi) for lo, hi, _, _, _ in r["passes"]]
    if r["kind"] != "split":
        c.append((0, r["lds_cut"]))
    if r["lv"]:
        c.append((r["hbm_cut"], max_len))
    if not r["gated"] and r["hbm_waves"]:
        c.append((r["hbm_cut"], max_len))
    return c


def test_route_claims_every_length_once(plan_bin):
    rows = [row(n, max_len, level, lane_ok, dict_len, latency, small, force_v1, mono_env, big_env)
            for level, dict_len, lane_ok, latency, small, force_v1, mono_env, big_env, n, max_len in itertools.product(
                (EXACT, FAST, FAST_ALL), (0, 2048, 8192), (True, False), (False, True), (False, True), (-1, 0, 1),
                (-1, 0, 1), (-1, 0, 1), (1, 1024, 2 * CUS, 2 * CUS + 1, 10_000_000),
                (1, 512, 1024, 4096, 16382, 16383, 31808, 31809, 65536, 4 << 20))]
    got = routes(plan_bin, rows)
    for rw, g in zip(rows, got):
        assert g == want_route(*rw), rw
        max_len = rw[1]
        at = 0
        for lo, hi in sorted(claims(g, max_len)):  # the claims tile (0, max_len]: no gap, no overlap
            assert lo == at and hi > lo, (rw, g)
            at = hi
        assert at == max_len, (rw, g)
        assert (g["kind"] == "split") == bool(g["passes"])


def test_route_rows_pinned(plan_bin):
    a, b, c, d = routes(plan_bin, [row(10_000_000, 1024, EXACT), row(1000, 16382, FAST, dict_len=2048),
                                   row(8, 30000, EXACT), row(8, 30000, FAST_ALL)])
    assert a["kind"] == "split" and a["passes"] == [[0, 1024, 1024, 0, 0]] and not a["lv"]
    assert a["gated"] and a["rlist"] and a["hbm_waves"] == 64
    assert b["passes"] == [[0, 14334, 14336, 1, 1], [14334, 16382, 16382, 1, 0]] and b["dict_len"] == 2048 and not b["lv"]
    assert c["passes"] == [[0, 16382, 16382, 0, 0], [16382, 30000, 30016, 0, 0]] and not c["lv"] and c["hbm_cut"] == 30000
    assert d["passes"] == [[0, 16382, 16382, 1, 0]] and d["lv"] and d["fast_all"] and d["hbm_cut"] == 16382


# ---- the decompress plan, restated ------------------------------------------------------------------------
# Written from the host code as it was before plan_inflate existed (decompress_batch_body, chunk_pass_decode,
# latency_decompress and host_batch's need_hbm expression in pmc_capi.hip), branch by branch, not from
# pmc_plan.hpp.
IDX_CHUNK, IDX_MAX_CHUNKS = 32768, 16382
REC_MAX, REC_OUT_MAX, SCAN_BLOCK, LDS_OUT_LIMIT = 2048, 4096, 1024, 48 * 1024
# stand-ins for what the runtime answers on the device: resident blocks per CU of inflate_rec_kernel<1024>,
# inflate_rec_kernel<4096> and inflate_chunk_kernel
REC_PER_CU_1K, REC_PER_CU_4K, CHUNK_PER_CU = 8, 5, 20


def gzip_bound(n):
    return n + (n >> 3) + 6 * (n // 16383 + 1) + 32


def want_inflate(n, max_len, cus, latency, need_hbm, dict_len, wave_only, no_order, no_rec, rec_1k, rec_4k, chunk_per_cu,
                 rec_max, rec_out_max, scan_block, out_limit):
    dD = dict_len
    chunk_pass = not wave_only and max_len > IDX_CHUNK
    retry_only = retried = order = rec = False
    # "if (chunk_pass && latency)": the wave-only route's chunk pass, every member looked at
    chunk_all = bool(chunk_pass and latency)
    crcx = chunk_all
    if chunk_all:
        retry_only = True
    # "if (!wave_only && !latency)": order, record kernel, lane passes, chunk pass, verify
    lane = not wave_only and not latency
    if lane:
        crcx = True
        order = not no_order and n >= 4096
        rec = not no_rec
        retry_only = retried = True
    ob = min((n + 1023) // 1024, cus * 4)
    lb = min((n + 63) // 64, cus * 16)
    rstride = min(rec_max, max(64, (max_len + 63) & ~63))
    out1k = max_len <= 1024
    slots = cus * (rec_1k if out1k else rec_4k)
    G = 1
    while G < 64 and (n + G - 1) // G > slots:
        G *= 2
    rb = min((n + G - 1) // G, slots)
    VG = 1
    while VG < 64 and (n + VG - 1) // VG > cus * 32:
        VG *= 2
    vb = min((n + 8 * VG - 1) // (8 * VG), cus * 4)
    # chunk_pass_decode
    nb = (n + scan_block - 1) // scan_block
    o_fail, o_pre = 4 * n, (8 * n + 7) & ~7
    o_bsum = o_pre + 8 * n
    mb = min((n + 255) // 256, cus * 8)
    cb = min(cus * chunk_per_cu, (n * IDX_MAX_CHUNKS + 63) // 64)
    # the wave kernels
    out_cap = (min(out_limit, max(max_len, 1)) + 63) & ~63
    lds_max_in = gzip_bound(out_cap) + 64
    dict_out = out_cap + ((dD + 15) & ~15)
    dict_in = gzip_bound(DICT_SPAN - dD) + 64 if dD else 0
    dict_second = bool(dD and need_hbm and (dict_out < DICT_SPAN or lds_max_in < dict_in))
    waves = min(cus * 4, n)
    return {"lane_route": int(lane), "chunk_pass": int(chunk_pass), "chunk_all": int(chunk_all), "order": int(order),
            "rec": int(rec), "multi_pass": int(max_len > 16383), "verify": int(crcx), "dict_second": int(dict_second),
            "hbm": int(need_hbm), "retry_only": int(retry_only), "count_retried": int(retried),
            "ob": ob, "lb": lb, "out1k": int(out1k), "rstride": rstride, "G": G, "rb": rb,
            "rec_max_out": 1024 if out1k else rec_out_max, "VG": VG, "vb": vb, "mb": mb, "cb": cb, "hbm_waves": waves,
            "hbm_blocks": (waves + 3) // 4,
            "crcx": n * 4, "order_bytes": ORDER_BINS * 4 + n * 4, "recs": rb * 64 * rstride * 4 + 256, "bigl": n * 4 + 256,
            "idx": {"cnt": 0, "fail": o_fail, "pre": o_pre, "bsum": o_bsum, "total": o_bsum + 8 * nb,
                    "bytes": o_bsum + 8 * (nb + 1)},
            "out_cap": out_cap, "lds_max_in": lds_max_in, "dict_out": dict_out,
            "second": {"lds_max_out": (DICT_SPAN + 63) & ~63, "lds_max_in": dict_in, "dict_out": (DICT_SPAN + 63) & ~63,
                       "first_img": dict_out, "first_in": lds_max_in}}


def want_latency(n, max_len, out_bytes, cus, lat_batch, lat_max_len, device_call, out_limit):
    lb, lm = 4 * lat_batch, lat_max_len
    max_out = max(lm, out_limit) if lm else 0                                        # latency_max_out()
    lat = n <= lb and max_len <= max_out and (max_len <= lm or out_bytes <= lb * lm)  # latency_decompress()
    return bool(lat or (device_call and lat_batch != 0 and n <= 4 * cus))            # pmc_gzip_decompress_batch


def want_need_hbm(latency, max_len, max_in, out_limit):
    lim = (min(out_limit, max(max_len, 1)) + 63) & ~63  # inflate_lds_limit_out(max_len)
    return bool(not latency or max_len > lim or max_in > gzip_bound(lim) + 64)


def plan_lines(plan_bin, mode, rows):
    text = "".join(" ".join(str(int(x)) for x in r) + "\n" for r in rows)
    out = subprocess.run([plan_bin[0], mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [json.loads(ln) for ln in out.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def irow(n, max_len, cus=CUS, latency=False, need_hbm=True, dict_len=0, wave_only=False, no_order=False, no_rec=False):
    return (n, max_len, cus, latency, need_hbm, dict_len, wave_only, no_order, no_rec, REC_PER_CU_1K, REC_PER_CU_4K,
            CHUNK_PER_CU, REC_MAX, REC_OUT_MAX, SCAN_BLOCK, LDS_OUT_LIMIT)


INFLATE_N = (1, 63, 64, 65, 4095, 4096, 4 * CUS, 4 * CUS + 1, 65536, 10_000_000)
INFLATE_LENS = (1, 64, 1024, 1025, 4096, 4097, 16383, 16384, 32768, 32769, 49152, 49153, 65536, 1 << 20, U32MAX)


def pow2_le_64(g):
    return 1 <= g <= 64 and g & (g - 1) == 0


def test_inflate_plan_matches_the_restated_formulas(plan_bin):
    rows = [irow(n, max_len, cus, latency, need_hbm, dict_len, wave_only, no_order, no_rec)
            for n, max_len, dict_len, latency, need_hbm, wave_only, no_order, no_rec, cus in itertools.product(
                INFLATE_N, INFLATE_LENS, (0, 1, 2048, 8192), (False, True), (False, True), (False, True), (False, True),
                (False, True), (8, 256))]
    got = plan_lines(plan_bin, "inflate", rows)
    for rw, g in zip(rows, got):
        assert g == want_inflate(*rw), rw
        n, max_len, cus, latency, need_hbm, dict_len, wave_only = rw[:7]
        rec_per_cu = REC_PER_CU_1K if g["out1k"] else REC_PER_CU_4K
        # every grid within [1, its residency cap]
        for key, cap in (("ob", cus * 4), ("lb", cus * 16), ("rb", cus * rec_per_cu), ("vb", cus * 4), ("mb", cus * 8),
                         ("cb", cus * CHUNK_PER_CU), ("hbm_blocks", cus), ("hbm_waves", cus * 4)):
            assert 1 <= g[key] <= cap, (key, rw, g)
        assert pow2_le_64(g["G"]) and pow2_le_64(g["VG"]), (rw, g)
        assert -(-n // g["G"]) <= cus * rec_per_cu or g["G"] == 64, (rw, g)
        assert -(-n // g["VG"]) <= cus * 32 or g["VG"] == 64, (rw, g)
        assert g["rstride"] % 64 == 0 and 64 <= g["rstride"] <= REC_MAX, (rw, g)
        # the idx rows: cnt u32[n] | fail u32[n] | pre u64[n] | bsum u64[nb] | total u64, none overlapping
        ix, nb = g["idx"], -(-n // SCAN_BLOCK)
        end = 0
        for name, size in (("cnt", 4 * n), ("fail", 4 * n), ("pre", 8 * n), ("bsum", 8 * nb), ("total", 8)):
            assert ix[name] >= end, (name, rw, g)
            end = ix[name] + size
        assert ix["pre"] % 8 == 0 and ix["bsum"] % 8 == 0 and ix["total"] % 8 == 0 and ix["bytes"] >= end, (rw, g)
        assert bool(g["chunk_pass"]) == (not wave_only and max_len > 32768), (rw, g)
        assert bool(g["retry_only"]) == bool(g["lane_route"] or g["chunk_pass"]), (rw, g)
        assert not g["dict_second"] or (dict_len != 0 and need_hbm), (rw, g)
        if dict_len:
            assert g["second"]["dict_out"] >= DICT_SPAN and g["second"]["lds_max_out"] >= DICT_SPAN, (rw, g)
            assert g["second"]["lds_max_in"] >= gzip_bound(DICT_SPAN - dict_len) + 64, (rw, g)
        assert bool(g["multi_pass"]) == (max_len > 16383), (rw, g)


def test_inflate_need_hbm_contract(plan_bin):
    """Where inflate_need_hbm says no, the LDS pass of that call's plan holds every member: image >= max_len and
    staged input >= max_in (else a host call would skip the HBM pass for a member the LDS pass cannot hold)."""
    cases = []
    for max_len in INFLATE_LENS:
        out_cap = (min(LDS_OUT_LIMIT, max(max_len, 1)) + 63) & ~63
        edge = gzip_bound(out_cap) + 64
        cases += [(latency, max_len, max_in) for latency in (True, False) for max_in in (1, edge - 1, edge, edge + 1)]
    got = plan_lines(plan_bin, "need_hbm", [(lat, ml, mi, LDS_OUT_LIMIT) for lat, ml, mi in cases])
    plans = plan_lines(plan_bin, "inflate", [irow(400, ml, latency=lat, need_hbm=bool(nh)) for (lat, ml, mi), nh in zip(cases, got)])
    said_no = 0
    for (lat, max_len, max_in), nh, p in zip(cases, got, plans):
        assert bool(nh) == want_need_hbm(lat, max_len, max_in, LDS_OUT_LIMIT), (lat, max_len, max_in)
        if not nh:
            said_no += 1
            assert lat and p["out_cap"] >= max_len and p["lds_max_in"] >= max_in and not p["hbm"], (max_len, max_in, p)
    assert said_no == 3 * sum(1 for ml in INFLATE_LENS if ml <= LDS_OUT_LIMIT)


def test_inflate_latency_matches_the_restated_rule(plan_bin):
    MiB16 = 16 << 20
    rows = []
    for cus, lat_batch, lat_max_len, device_call in itertools.product((8, 256, 2048), (1024, 0), (4096, 0), (False, True)):
        for n in (1, 4096, 4097, 4 * cus, 4 * cus + 1):
            for max_len in (1, 4096, 4097, 49152, 49153):
                for out_bytes in (n * max_len, MiB16, MiB16 + 1):
                    rows.append((n, max_len, out_bytes, cus, lat_batch, lat_max_len, device_call, LDS_OUT_LIMIT))
    got = plan_lines(plan_bin, "latency", rows)
    for rw, g in zip(rows, got):
        assert bool(g) == want_latency(*rw), rw
    lat = dict(zip(rows, got))
    # the clauses by name: 4,096 members of 4 KiB; a 48 KiB member within 16 MiB in all; 4 members per CU on
    # the device entry only; PMC_LATENCY_BATCH=0 and PMC_LATENCY_MAX_LEN=0 turn the route off
    assert lat[(4096, 4096, 4096 * 4096, 256, 1024, 4096, False, LDS_OUT_LIMIT)] == 1
    assert lat[(4097, 4096, 4097 * 4096, 256, 1024, 4096, False, LDS_OUT_LIMIT)] == 0
    assert lat[(1, 49152, MiB16, 256, 1024, 4096, False, LDS_OUT_LIMIT)] == 1
    assert lat[(1, 49152, MiB16 + 1, 256, 1024, 4096, False, LDS_OUT_LIMIT)] == 0
    assert lat[(1, 49153, 49153, 256, 1024, 4096, False, LDS_OUT_LIMIT)] == 0
    assert lat[(1, 49153, 49153, 256, 1024, 4096, True, LDS_OUT_LIMIT)] == 1
    assert lat[(1024, 49153, 1024 * 49153, 256, 1024, 4096, True, LDS_OUT_LIMIT)] == 1
    assert lat[(1025, 49153, 1025 * 49153, 256, 1024, 4096, True, LDS_OUT_LIMIT)] == 0
    assert lat[(8192, 49153, 8192 * 49153, 2048, 1024, 4096, True, LDS_OUT_LIMIT)] == 1
    assert lat[(8192, 49153, 8192 * 49153, 2048, 1024, 4096, False, LDS_OUT_LIMIT)] == 0
    assert not any(g for rw, g in zip(rows, got) if rw[4] == 0)
    assert not any(g for rw, g in zip(rows, got) if rw[5] == 0 and not (rw[6] and rw[0] <= 4 * rw[3]))


def test_inflate_rows_pinned(plan_bin):
    flat, host, wide, mid, dic = plan_lines(plan_bin, "inflate", [
        irow(10_000_000, 1024),                             # the flagship batch: record kernel, 1 KiB instance
        irow(400, 4096, latency=True, need_hbm=False),      # a host call of a server's GET batch
        irow(1000, 1 << 20, latency=True),                  # at most 4 members per CU: wave kernels after the chunk pass
        irow(40_000, 65536),                                # the pipeline with the multi-block pass and the chunk pass
        irow(5000, 1024, dict_len=2048)])                   # a dictionary context: two LDS passes
    stages = ("lane_route", "order", "rec", "multi_pass", "chunk_pass", "chunk_all", "verify", "dict_second", "hbm",
              "retry_only", "count_retried")
    on = lambda p: [s for s in stages if p[s]]
    assert on(flat) == ["lane_route", "order", "rec", "verify", "hbm", "retry_only", "count_retried"]
    assert (flat["ob"], flat["lb"], flat["out1k"], flat["rstride"], flat["G"], flat["rb"], flat["rec_max_out"]) == (
        1024, 4096, 1, 1024, 64, 2048, 1024)
    assert (flat["VG"], flat["vb"], flat["out_cap"], flat["lds_max_in"], flat["hbm_waves"], flat["hbm_blocks"]) == (
        64, 1024, 1024, 1254, 1024, 256)
    assert flat["recs"] == 2048 * 64 * 1024 * 4 + 256 and flat["crcx"] == 40_000_000
    assert on(host) == [] and (host["out_cap"], host["lds_max_in"], host["dict_out"]) == (4096, 4710, 4096)
    assert on(wide) == ["multi_pass", "chunk_pass", "chunk_all", "verify", "hbm", "retry_only"]
    assert (wide["mb"], wide["cb"], wide["VG"], wide["vb"], wide["out_cap"], wide["hbm_waves"]) == (4, 5120, 1, 125, 49152, 1000)
    assert wide["idx"] == {"cnt": 0, "fail": 4000, "pre": 8000, "bsum": 16000, "total": 16008, "bytes": 16016}
    assert on(mid) == ["lane_route", "order", "rec", "multi_pass", "chunk_pass", "verify", "hbm", "retry_only", "count_retried"]
    assert (mid["out1k"], mid["rstride"], mid["G"], mid["rb"], mid["rec_max_out"], mid["lb"]) == (0, 2048, 32, 1250, 4096, 625)
    assert on(dic) == ["lane_route", "order", "rec", "verify", "dict_second", "hbm", "retry_only", "count_retried"]
    assert (dic["out_cap"], dic["dict_out"], dic["lds_max_in"]) == (1024, 3072, 1254)
    assert dic["second"] == {"lds_max_out": 16384, "lds_max_in": 16227, "dict_out": 16384, "first_img": 3072, "first_in": 1254}

"""CPU: the plans of the host-memory calls (csrc/pmc_plan.hpp: HostStage, plan_host_batch, pinned_chunk_of,
plan_pinned_chunk, PinnedSlot), printed by tests/host/plan_check.cpp, equal a restatement of the arithmetic that
host_batch_locked and pinned_batch_run did inline before those plans existed: the two sums and the running
offset of the host call's staging, its route, and per pinned chunk the source range, the tiled-or-compacted
decision, the destination range and the slot's chain of arrays.  The restatement below is written from that
code, branch by branch, not from pmc_plan.hpp."""
import itertools

import pytest

from test_host_plan import CUS, EXACT, FAST, FAST_ALL, LDS_OUT_LIMIT, SCAN_BLOCK, U32MAX
from test_host_plan import check_regions, plan_bin, plan_lines, want_latency, want_need_hbm  # noqa: F401

MiB16 = 16 << 20
LAT_BATCH, LAT_MAX_LEN = 1024, 4096


def al(x):
    return (x + 255) & ~255


# ---- a host call, restated --------------------------------------------------------------------------------
# A batch is given as runs (count, src_len, dst_cap), so that 4,097 values stay one short line.
def want_host(compress, level, lane_ok, force, cus, lat_batch, lat_max, out_limit, runs):
    n = sum(c for c, _, _ in runs)
    # "for (i < n) in_bytes += src_len[i]; out_bytes += dst_cap[i]; max_len = ...; max_in = ..."
    in_bytes = sum(c * s for c, s, _ in runs)
    out_bytes = sum(c * d for c, _, d in runs)
    max_len = max(s if compress else d for _, s, d in runs)
    max_in = max(s for _, s, _ in runs)
    down = al(n * 8) * 2 + al(n * 4) * 2 + al(in_bytes + 16)
    up = al(n * 4) * 2 + al(out_bytes + 16)
    fast = bool(compress and level in (FAST, FAST_ALL) and lane_ok)
    if compress:
        latency = not force and (not fast and n <= lat_batch and max_len <= lat_max)
    else:
        latency = not force and want_latency(n, max_len, out_bytes, cus, lat_batch, lat_max, False, out_limit)
    path = (0 if latency else 2) + (0 if compress else 1)
    # run(): only a decompress call states it
    need_hbm = bool(not compress and want_need_hbm(latency, max_len, max_in, out_limit))
    # the second walk: "h_soff = hp + o; o += al(n * 8ull); ..."
    o, off = 0, {}
    for name, size in (("soff", n * 8), ("doff", n * 8), ("slen", n * 4), ("dcap", n * 4), ("src", in_bytes + 16),
                       ("dlen", n * 4), ("rc", n * 4), ("dst", out_bytes + 16)):
        off[name] = o
        o += al(size)
    # "h_soff[i] = so; so += src_len[i]; h_doff[i] = doff; doff += dst_cap[i]"
    flat = [(s, d) for c, s, d in runs for _ in range(min(c, 9))][:9]
    so = do = 0
    soff_v, doff_v = [], []
    for s, d in flat[:min(n, 8)]:
        soff_v.append(so)
        doff_v.append(do)
        so, do = so + s, do + d
    return dict(off, in_bytes=in_bytes, out_bytes=out_bytes, max_len=max_len, max_in=max_in, latency=int(latency),
                need_hbm=int(need_hbm), path=path, down=down, up=up, bytes=down + up, lens_copied=1, soff_v=soff_v,
                doff_v=doff_v, soff_last=in_bytes - runs[-1][1], doff_last=out_bytes - runs[-1][2])


def host_row(compress, runs, level=EXACT, lane_ok=True, force=False, cus=CUS, lat_batch=LAT_BATCH, lat_max=LAT_MAX_LEN):
    runs = [r for r in runs if r[0] > 0]
    return (compress, level, lane_ok, force, cus, lat_batch, lat_max, LDS_OUT_LIMIT, runs)


def host_plans(plan_bin, rows):
    got = plan_lines(plan_bin, "host", [r[:8] + tuple(x for run in r[8] for x in run) for r in rows])
    for rw, g in zip(rows, got):
        assert g == want_host(*rw), rw
    return got


HOST_REGIONS = ("soff", "doff", "slen", "dcap", "src", "dlen", "rc", "dst")


def check_host_layout(rw, g):
    n = sum(c for c, _, _ in rw[8])
    sizes = {"soff": 8 * n, "doff": 8 * n, "slen": 4 * n, "dcap": 4 * n, "src": g["in_bytes"] + 16, "dlen": 4 * n,
             "rc": 4 * n, "dst": g["out_bytes"] + 16}
    check_regions([(nm, g[nm], sizes[nm]) for nm in HOST_REGIONS], g["bytes"])
    assert [g[nm] for nm in HOST_REGIONS] == sorted(g[nm] for nm in HOST_REGIONS) and g["soff"] == 0
    # one H2D moves everything in front of dlen, one D2H everything from dlen on
    assert g["down"] == g["dlen"] and g["down"] + g["up"] == g["dst"] + al(g["out_bytes"] + 16) == g["bytes"]


def test_host_layout_matches_the_two_walks(plan_bin):
    """n where 8n and 4n cross a multiple of 256, byte totals where + 16 does: one value carries the bytes, every
    other one is zero-length"""
    rows = [host_row(compress, [(1, ib, ob), (n - 1, 0, 0)] if first else [(n - 1, 0, 0), (1, ib, ob)])
            for compress, n, ib, ob, first in itertools.product((True, False), (1, 32, 33, 64, 65, 1024, 1025, 4096, 4097),
                                                                (0, 239, 240, 241), (0, 239, 240, 241), (True, False))]
    src_room, dst_room = {}, {}
    for rw, g in zip(rows, host_plans(plan_bin, rows)):
        check_host_layout(rw, g)
        src_room.setdefault(g["in_bytes"], set()).add(g["dlen"] - g["src"])
        dst_room.setdefault(g["out_bytes"], set()).add(g["bytes"] - g["dst"])
    assert src_room == dst_room == {0: {256}, 239: {256}, 240: {256}, 241: {512}}


def test_host_layout_of_the_longest_values(plan_bin):
    """three values of 4294967295 bytes: the sums and the offsets are 64-bit"""
    for compress in (True, False):
        rw = host_row(compress, [(3, U32MAX, U32MAX)])
        (g,) = host_plans(plan_bin, [rw])
        check_host_layout(rw, g)
        assert g["in_bytes"] == g["out_bytes"] == 3 * U32MAX > 1 << 33 and g["max_len"] == g["max_in"] == U32MAX
        assert g["soff_v"] == g["doff_v"] == [0, U32MAX, 2 * U32MAX] and g["bytes"] > 1 << 34
        assert not g["latency"] and g["path"] == (2 if compress else 3)


def spread(n, max_len, total):
    """n lengths, the first max_len, none above it, `total` in all (None: there are none)"""
    if n == 1:
        return [(1, max_len)] if total == max_len else None
    rest, k = total - max_len, n - 1
    if rest < 0:
        return None
    base, rem = divmod(rest, k)
    if base + (1 if rem else 0) > max_len:
        return None
    return [(1, max_len), (rem, base + 1), (k - rem, base)]


def test_host_route_matches_the_restated_rule(plan_bin):
    rows = []
    for compress, level, lane_ok, force, lat_batch, lat_max, n, max_len, out, max_in in itertools.product(
            (True, False), (EXACT, FAST, FAST_ALL), (True, False), (False, True), (LAT_BATCH, 0), (LAT_MAX_LEN, 0),
            (1, 1024, 1025, 4096, 4097), (4096, 4097, 49152, 49153), (None, MiB16, MiB16 + 1), (100, 70000)):
        lens = spread(n, max_len, n * max_len if out is None else out)
        if lens is None:
            continue
        if compress:   # the lengths are the sources', the capacities roomy
            runs = [(c, ln, ln + 64) for c, ln in lens]
        else:          # the lengths are the capacities; max_in: the longest member
            runs = [(c, max_in if k == 0 else 100, ln) for k, (c, ln) in enumerate(lens)]
        rows.append(host_row(compress, runs, level, lane_ok, force, CUS, lat_batch, lat_max))
    got = host_plans(plan_bin, rows)
    seen = set()
    for rw, g in zip(rows, got):
        compress, level, lane_ok, force, _, lat_batch, lat_max = rw[:7]
        assert g["path"] == (0 if g["latency"] else 2) + (0 if compress else 1), rw
        assert not (g["latency"] and (force or lat_batch == 0 or lat_max == 0)), rw
        assert not (compress and g["latency"] and level != EXACT and lane_ok), rw
        assert compress or g["need_hbm"] or g["latency"], rw
        seen.add((compress, g["latency"], g["need_hbm"]))
    assert seen == {(True, 0, 0), (True, 1, 0), (False, 0, 1), (False, 1, 0), (False, 1, 1)}
    # a 48 KiB member stays on the latency route up to 16 MiB of capacities in all, and not one byte beyond
    by = {(rw[0], rw[1], rw[2], rw[3], rw[5], rw[6], g["out_bytes"], g["max_len"], g["max_in"], sum(c for c, _, _ in rw[8])): g
          for rw, g in zip(rows, got)}
    assert by[(False, EXACT, True, False, LAT_BATCH, LAT_MAX_LEN, MiB16, 49152, 100, 1024)]["latency"] == 1
    assert by[(False, EXACT, True, False, LAT_BATCH, LAT_MAX_LEN, MiB16 + 1, 49152, 100, 1024)]["latency"] == 0
    assert by[(False, EXACT, True, False, LAT_BATCH, LAT_MAX_LEN, MiB16, 49153, 100, 1024)]["latency"] == 0


def test_host_route_rows_pinned(plan_bin):
    """the rows INTEGRATION.md quotes"""
    k4 = 4096
    a, b, c, d, e = host_plans(plan_bin, [
        host_row(True, [(1024, k4, k4 + 600)]),                 # 1,024 x 4 KiB compress: latency
        host_row(True, [(1025, k4, k4 + 600)]),                 # 1,025: pipeline
        host_row(True, [(8, k4, k4 + 600)], level=FAST),        # any fast level: pipeline
        host_row(True, [(8, k4, k4 + 600)], level=FAST_ALL),
        host_row(False, [(400, 1500, k4)])])                    # 400 x 4 KiB decompress: latency, no HBM pass
    assert (a["latency"], a["path"]) == (1, 0)
    assert (b["latency"], b["path"]) == (0, 2)
    assert (c["latency"], c["path"]) == (0, 2) and (d["latency"], d["path"]) == (0, 2)
    assert (e["latency"], e["need_hbm"], e["path"]) == (1, 0, 1)
    assert (e["in_bytes"], e["out_bytes"], e["max_len"], e["max_in"]) == (400 * 1500, 400 * k4, k4, 1500)


# ---- a pinned call's chunks, restated -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65536, 65537, 16 * 65536 + 1])
@pytest.mark.parametrize("chunk", [0, 1, 7])
def test_pinned_chunk_of(plan_bin, n, chunk):
    (g,) = plan_lines(plan_bin, "pinned", [(n, chunk)])
    want = chunk if chunk else max(65536, (n + 15) // 16)   # "if (chunk == 0) chunk = max(65536, (n + 15) / 16)"
    assert g == {"chunk": want, "nchunks": (n + want - 1) // want}
    assert (g["nchunks"] - 1) * g["chunk"] < n <= g["nchunks"] * g["chunk"]


def want_pinned(packed, a, m, vals):
    """vals: (src_off, src_len, dst_off, dst_cap) of every value of the batch; the chunk is vals[a : a + m]"""
    ch = vals[a:a + m]
    sb = min(so for so, _, _, _ in ch)
    se = max(so + sl for so, sl, _, _ in ch)
    compact = bool(packed)
    db, de = 2 ** 64 - 1, 0
    if not packed:
        for (_, _, d0, c0), (_, _, d1, _) in zip(ch, ch[1:]):
            compact = compact or d1 != d0 + c0
        db = ch[0][2]
        de = ch[-1][2] + ch[-1][3]
    if compact:
        db = 0
        de = sum(c for _, _, _, c in ch)
    nb = (m + SCAN_BLOCK - 1) // SCAN_BLOCK
    meta = al(m * 8) * 3 + al(m * 4) * 4 + al((nb + 1) * 8)
    need = meta + al(se - sb + 16) + al(de - db + 16) * (2 if compact else 1)
    # "d_doff = d_soff + al(m * 8ull) / 8, ..."
    soff = 0
    doff = soff + al(m * 8)
    poff = doff + al(m * 8)
    slen = poff + al(m * 8)
    dcap = slen + al(m * 4)
    dlen = dcap + al(m * 4)
    rc = dlen + al(m * 4)
    bsum = rc + al(m * 4)
    src = meta
    dst = src + al(se - sb + 16)
    pk = dst + al(de - db + 16)
    return {"sb": sb, "se": se, "db": db, "de": de, "compact": int(compact), "nb": nb, "soff": soff, "doff": doff,
            "poff": poff, "slen": slen, "dcap": dcap, "dlen": dlen, "rc": rc, "bsum": bsum, "meta": meta, "src": src,
            "dst": dst, "packed": pk, "need": need}


def values(n, lens=None, caps=None, base=5, gaps=None, order=None, soffs=None):
    """n values: sources back to back from 11 (soffs: given), slots tiled from `base` in `order` with gaps[k] bytes
    in front of the k-th slot"""
    lens = lens or [1 + (37 * i) % 200 for i in range(n)]
    caps = caps or [ln + 40 for ln in lens]
    order = list(order) if order is not None else list(range(n))
    doff, at = [0] * n, base
    for k, i in enumerate(order):
        at += gaps.get(k, 0) if gaps else 0
        doff[i] = at
        at += caps[i]
    so, at = [], 11
    for ln in lens:
        so.append(at)
        at += ln
    if soffs is not None:
        so = soffs
    return list(zip(so, lens, doff, caps))


PINNED_CASES = {
    # name: (packed, a, m, values, compact)
    "tiled": (0, 0, 8, values(8), 0),
    "tiled-inner": (0, 8, 8, values(24), 0),
    # a gap in front of the chunk's first slot or behind its last one leaves it tiled
    "gaps-outside": (0, 8, 8, values(24, gaps={8: 3, 16: 9}), 0),
    "gap": (0, 8, 8, values(24, gaps={12: 1}), 1),
    "gap-at-the-last-slot": (0, 8, 8, values(24, gaps={15: 7}), 1),
    "permuted": (0, 0, 8, values(8, order=[3, 0, 7, 1, 6, 2, 5, 4]), 1),
    "overlapping-slots": (0, 0, 2, [(11, 5, 100, 50), (16, 5, 120, 50)], 1),
    "packed": (1, 0, 8, values(8), 1),
    "packed-inner": (1, 8, 8, values(24), 1),
    "m1-slot-mode": (0, 3, 1, values(8, order=[3, 0, 7, 1, 6, 2, 5, 4]), 0),
    "m1-packed": (1, 3, 1, values(8), 1),
    "shared-source": (0, 0, 4, values(4, lens=[100] * 4, soffs=[700, 11, 700, 650]), 0),
    "zero-length": (0, 0, 6, values(6, lens=[0, 7, 0, 0, 9, 0], caps=[0, 30, 0, 8, 30, 0]), 0),
    "all-zero": (0, 0, 3, values(3, lens=[0, 0, 0], caps=[0, 0, 0]), 0),
    "zero-length-compacted": (0, 0, 6, values(6, lens=[0, 7, 0, 0, 9, 0], caps=[0, 30, 0, 8, 30, 0], gaps={2: 4}), 1),
    "m1024": (0, 0, 1024, values(1025), 0),
    "m1025": (0, 0, 1025, values(1025), 0),
    "m1024-compacted": (0, 1, 1024, values(1025, gaps={500: 2}), 1),
    "m1025-packed": (1, 0, 1025, values(1025), 1),
    "m2049-long": (0, 0, 2049, values(2049, lens=[U32MAX] * 2049, caps=[U32MAX] * 2049), 0),
}


@pytest.mark.parametrize("case", list(PINNED_CASES))
def test_pinned_chunk_plan(plan_bin, case):
    packed, a, m, vals, compact = PINNED_CASES[case]
    (g,) = plan_lines(plan_bin, "pinned", [(packed, a, m) + tuple(x for v in vals for x in v)])
    w = want_pinned(packed, a, m, vals)
    assert g == w, case
    assert g["compact"] == compact and g["nb"] == -(-m // 1024), case
    src_bytes, dst_bytes = g["se"] - g["sb"] + 16, g["de"] - g["db"] + 16
    sizes = [("soff", 8 * m), ("doff", 8 * m), ("poff", 8 * m), ("slen", 4 * m), ("dcap", 4 * m), ("dlen", 4 * m),
             ("rc", 4 * m), ("bsum", 8 * (g["nb"] + 1)), ("src", src_bytes), ("dst", dst_bytes),
             ("packed", dst_bytes if compact else 0)]
    check_regions([(nm, g[nm], sz) for nm, sz in sizes], g["need"])
    assert g["meta"] == g["src"] == 3 * al(8 * m) + 4 * al(4 * m) + al(8 * (g["nb"] + 1)), case
    # the compacted bytes: as large as the slots, and there only for a compacted chunk
    assert g["need"] - g["packed"] == (al(dst_bytes) if compact else 0), case
    assert g["need"] == g["meta"] + al(src_bytes) + al(dst_bytes) * (2 if compact else 1), case
    ch = vals[a:a + m]
    assert all(g["sb"] <= so and so + sl <= g["se"] for so, sl, _, _ in ch), case
    if compact:
        assert (g["db"], g["de"]) == (0, sum(c for _, _, _, c in ch)), case
    else:
        assert (g["db"], g["de"]) == (ch[0][2], ch[-1][2] + ch[-1][3]), case


def test_pinned_cases_cover_the_steps():
    ms = {m for _, _, m, _, _ in PINNED_CASES.values()}
    assert {1, 1024, 1025} <= ms
    assert {(p, c) for p, _, _, _, c in PINNED_CASES.values()} == {(0, 0), (0, 1), (1, 1)}

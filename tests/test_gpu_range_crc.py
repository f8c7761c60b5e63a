"""GPU: chunk CRCs of indexed members, and ranged reads that verify their bytes (include/pmc_codec.h "member
index", chunk CRCs, and "ranged reads", INTEGRITY).

With the level at PMC_LEVEL_FAST_ALL, the index switch and the index_crc switch on, a value above C bytes
becomes the indexed member of the index switch alone with a second FEXTRA subfield that holds every chunk's
CRC-32 and every offset shifted by its length -- the stream bytes are the same; every other value gives the bytes
it gives with the switch off.  Full reads do not look at the subfield.  A ranged read checks every chunk it
decoded against its entry (pmc_ctx_range_verify_counts proves it): a bit flip in a chunk's stream that keeps
the structure and changes the bytes -- which a ranged read of a plain indexed member answers PMC_OK with wrong
bytes -- is answered PMC_E_NO_INDEX by every request that covers the chunk and by no other.  In "require" mode
members without chunk CRCs are declined at the scan."""
import ctypes
import zlib

import numpy as np
import pytest

from indexed_crc_model import (assemble_crc, chunk_crcs, crc_defects, header_crc, parse_chunk_crcs, plan,
                               read_range_verified)
from indexed_model import C, assemble, parse_index
from indexed_values import indexed_values
from range_model import chunk_bytes, chunk_span, range_of, ranges_for, read_range
from test_gpu_foreign import PIPELINE_N, Case, check_route, cus
from test_gpu_indexed import split_blocks
from test_gpu_range import device_compress, ranged_call, repeat_extents, untouched

pytestmark = pytest.mark.gpu

RANDOM = "random_2C+3"
FLIP_SEED = 7     # np.random.default_rng(FLIP_SEED): per chunk 0, 1, 2 in turn, 200 x (byte of the span, bit)
FLIPS = 200


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    c.level = pmc_codec.LEVEL_FAST_ALL
    c.index = True
    assert c.index_crc is False and c.range_verify == 0
    c.index_crc = True
    assert c.index_crc is True
    for bad in (2, -1):
        with pytest.raises(ValueError):
            c.index_crc = bad
        with pytest.raises(ValueError):
            c.range_verify = bad
    assert c.index_crc is True and c.range_verify == 0
    yield c
    c.close()


@pytest.fixture(scope="module")
def vals(golden):
    by = dict(indexed_values(golden.corpus))
    out = [(f"json{n}", by[f"json{n}"]) for n in (C + 1, 2 * C, 2 * C + 3, 100000)]
    assert [len(v) for _, v in out] == [C + 1, 2 * C, 2 * C + 3, 100000]
    out.append((RANDOM, np.random.default_rng(20265).integers(0, 256, 2 * C + 3, dtype=np.uint8).tobytes()))
    return out


@pytest.fixture(scope="module")
def members(ctx, vals):
    """The values as one device batch with chunk CRCs (computed once, never changed)."""
    return device_compress(ctx, [v for _, v in vals])


@pytest.fixture(scope="module")
def plain(ctx, vals, members):
    """The same batch with the index_crc switch off."""
    ctx.index_crc = False
    try:
        return device_compress(ctx, [v for _, v in vals])
    finally:
        ctx.index_crc = True


def counts(ctx):
    a, b = ctx.range_counts(), ctx.range_verify_counts()
    return np.array([a["served"], a["declined"], a["chunks"], b["matched"], b["mismatched"]], dtype=np.int64)


def counted(ctx, fn):
    """fn(), and the growth of (served, declined, chunks, matched, mismatched) over it."""
    a = counts(ctx)
    res = fn()
    return res, tuple(int(x) for x in counts(ctx) - a)


def put(m, at, b):
    return m[:at] + bytes(b) + m[at + len(b):]


def test_written_members(ctx, golden, vals, members, plain):
    import torch
    import pmc_codec
    from pmc_codec import device as D
    L = pmc_codec.lib()
    for (name, v), m, p in zip(vals, members, plain):
        k = -(-len(v) // C)
        crcs = chunk_crcs(v)
        assert pmc_codec.index_info(p) == (C, k) and pmc_codec.index_crc_info(p) is None, name
        assert zlib.decompress(m, 31) == v and len(m) <= pmc_codec.gzip_bound(len(v)), name
        assert pmc_codec.index_crc_info(m) == crcs == parse_chunk_crcs(m), name
        _, _, offs, hdr = parse_index(m)
        _, _, poffs, phdr = parse_index(p)
        assert hdr == phdr + 8 + 4 * k == plan(len(v))[2] and offs == [o + 8 + 4 * k for o in poffs], name
        assert m[:hdr] == header_crc(len(v), offs, crcs) and m[hdr:] == p[phdr:], name
        assert m[8] == p[8] == 4 and m[4:8] == p[4:8] == bytes(4) and m[:10] == p[:10] and m[12:20] == p[12:20], name
        assert len(m) == len(p) + 8 + 4 * k, name
    values = [v for _, v in vals]
    n = len(values)
    # the same member alone, in another batch order, and through every entry point
    for v, m in zip(values, members):
        assert device_compress(ctx, [v]) == [m]
    perm = [3, 1, 4, 0, 2, 3]
    assert device_compress(ctx, [values[i] for i in perm]) == [members[i] for i in perm]
    assert ctx.compress_many(values) == [(0, m) for m in members]
    for v, m in list(zip(values, members))[::2]:
        out = ctypes.create_string_buffer(pmc_codec.gzip_bound(len(v)))
        olen = ctypes.c_size_t(0)
        assert L.pmc_gzip_compress(ctx.handle, v, len(v), out, len(out), ctypes.byref(olen)) == 0
        assert out.raw[:olen.value] == m
    st = pmc_codec.Store(ctx, 16 << 20)
    try:
        ext, rc = st.put(values)
        assert rc == [0] * n and st.members(ext, n) == members
        assert st.get(ext, n) == [(0, v) for v in values]
    finally:
        st.close()
    slab = pmc_codec.Slab(ctx, 8, max(len(v) for v in values))
    try:
        b = D.pack(values)
        slots = torch.from_numpy(np.array([5, 0, 7, 2, 3], dtype=np.int32)).cuda()
        src_rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        slab.set(b.data, b.off, b.len, slots, src_rc, D.stream_handle())
        torch.cuda.synchronize()
        assert int((src_rc != 0).sum()) == 0
        lens_t = torch.zeros(8, dtype=torch.int32, device="cuda")
        data_t = torch.zeros(slab.stride * 8, dtype=torch.uint8, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")
        for t, ptr, nb in ((lens_t, slab.lengths_ptr(), 4 * 8), (data_t, slab.data_ptr(), slab.stride * 8)):
            assert hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(nb), 3) == 0
        ln, data = lens_t.cpu().numpy(), data_t.cpu().numpy().tobytes()
        assert [data[s * slab.stride:s * slab.stride + int(ln[s])] for s in (5, 0, 7, 2, 3)] == members
    finally:
        slab.close()
    # where the switch does not act, the bytes are those with it off: values of <= C bytes, level 9, level fast,
    # and the index switch off
    small = [(golden.corpus * 2)[300:300 + k] for k in (1, 1000, 16383, 20000, C - 1, C)]
    try:
        on = {"small": device_compress(ctx, small)}
        for lvl in (pmc_codec.LEVEL_EXACT, pmc_codec.LEVEL_FAST):
            ctx.level = lvl
            on[lvl] = device_compress(ctx, values[:3] + small[-2:])
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index = False
        on["noindex"] = device_compress(ctx, values)
        ctx.index_crc = False
        assert device_compress(ctx, values) == on["noindex"] and all(m[3] == 0 for m in on["noindex"])
        ctx.index = True
        assert device_compress(ctx, small) == on["small"] and all(m[3] == 0 for m in on["small"])
        for lvl in (pmc_codec.LEVEL_EXACT, pmc_codec.LEVEL_FAST):
            ctx.level = lvl
            assert device_compress(ctx, values[:3] + small[-2:]) == on[lvl], lvl
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index = True
        ctx.index_crc = True


def test_read_back(ctx, vals, members, plain):
    import pmc_codec
    cases = [Case(n, m, len(v)) for (n, v), m in zip(vals, members)]
    assert all(c.rc == 0 and c.out == v for c, (_, v) in zip(cases, vals))
    # full reads: the wave-only route and the record / lane pipeline; the chunk pass completes every JSON member
    # and hands the one with stored blocks over, as without CRCs
    for pad_to in (0, max(PIPELINE_N, 4 * cus() + 8)):
        a = ctx.index_counts()
        check_route(ctx, cases, max(c.cap for c in cases), pad_to)
        b = ctx.index_counts()
        assert (b["completed"] - a["completed"], b["handed_over"] - a["handed_over"]) == (len(cases) - 1, 1)
    assert ctx.decompress_many(members) == [(0, v) for _, v in vals]
    # ranged reads: the model's bytes and the write bound, every decoded chunk verified -- and none for the same
    # values without CRCs.  The incompressible value's full chunks hold stored blocks, which the lane decoder
    # declines as ever (its 3-byte tail chunk is a block of literals and is served)
    for ms, verified in ((members, True), (plain, False)):
        reqs, want, chunks, good = [], [], 0, 0
        for (name, v), m in zip(vals, ms):
            stored = [any(b["type"] == 0 for b in c) for c in split_blocks(m, parse_index(m)[3])[0]]
            assert stored[:2] == [True, True] if name == RANDOM else not any(stored), (name, stored)
            for off, ln in ranges_for(len(v), C):
                assert read_range_verified(m, off, ln) == v[off:off + ln]
                _, L, k0, items = range_of(len(v), 15, off, ln)
                reqs.append((m, off, ln))
                want.append(None if any(stored[k0:k0 + items]) else v[off:off + ln])
                chunks += items
                good += items - sum(stored[k0:k0 + items])
        (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
        bad = [(k, int(rc[k]), int(dlen[k])) for k, w in enumerate(want)
               if (rc[k], dlen[k], slots[k]) != ((0, len(w), w) if w is not None else (pmc_codec.E_NO_INDEX, 0, slots[k]))]
        assert not bad, (len(bad), bad[:8])
        declined = sum(1 for w in want if w is None)
        assert declined >= 5 and got == (len(reqs) - declined, declined, chunks, good if verified else 0, 0), (got, chunks, good)
    # capacity: nothing written, nothing verified
    v, m = vals[3][1], members[3]
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, [(m, 0, 100), (m, C - 1, 2)], caps=[99, 1]))
    assert list(rc) == [pmc_codec.E_CAPACITY] * 2 and list(dlen) == [100, 2] and all(untouched(s) for s in slots)
    assert got == (0, 0, 0, 0, 0), got


def flips_of(m, rng):
    """[(chunk, damaged member)]: FLIPS seeded single-bit flips inside each chunk's compressed span that keep the
    chunk's structure (range_model.chunk_bytes) and change its bytes; and how many there were per chunk."""
    k = parse_index(m)[1]
    out, per = [], []
    for j in range(k):
        s, e, _, _ = chunk_span(m, j)
        good = chunk_bytes(m, j)
        assert good is not None
        found = 0
        for _ in range(FLIPS):
            at, bit = int(rng.integers(s, e)), int(rng.integers(0, 8))
            b = put(m, at, [m[at] ^ (1 << bit)])
            got = chunk_bytes(b, j)
            if got is not None and got != good:
                out.append((j, b))
                found += 1
        per.append(found)
    return out, per


def check_flips(ctx, v, m, flips, fixed):
    """Every flip: a request inside the damaged chunk and one over the whole value are declined, a request in
    each other chunk is served, and the mismatch is counted.  fixed: the member's blocks are fixed ones, where the
    lane decoder's structural test and range_model.chunk_bytes take the same streams, so every flip reaches the
    CRC check; a flip in a dynamic block's tables may also be declined by the decoder before it."""
    import pmc_codec
    k = parse_index(m)[1]
    reqs, want = [], []
    for j, b in flips:
        for q in range(k):
            off = q * C + (7 if len(v) - q * C > 60 else 0)
            ln = min(50, len(v) - off)
            reqs.append((b, off, ln))
            want.append(None if q == j else v[off:off + ln])
        reqs.append((b, 0, len(v)))
        want.append(None)
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
    bad = [(i, int(rc[i]), int(dlen[i])) for i, w in enumerate(want)
           if (w is None and (rc[i] != pmc_codec.E_NO_INDEX or dlen[i] != 0)) or
           (w is not None and (rc[i] != 0 or dlen[i] != len(w) or slots[i] != w))]
    assert not bad, (len(bad), len(reqs), bad[:8])
    # per flip: the damaged chunk is decoded and mismatches twice (its own request and the whole value's)
    print("flips:", len(flips), "(served, declined, chunks, matched, mismatched):", got)
    assert got[1] == 2 * len(flips) and got[0] == len(reqs) - got[1], got
    if fixed:
        assert got[4] == 2 * len(flips) and got[3] == got[2] - got[4], got
    else:
        assert 1 <= got[4] <= 2 * len(flips), got


def test_flips_that_keep_the_structure_are_declined(ctx, golden, vals, members):
    """The test that fails without chunk CRCs.  On the parent a ranged read of these members (it reads a member
    with the subfield as a plain indexed one) answers PMC_OK with other bytes for every flip counted here.
    Measured on the CPU for the assembled member with default_rng(7): 103, 88 and 99 of 200 flips in chunks 0, 1
    and 2 keep the structure and change the bytes."""
    v = (golden.corpus * 4)[100:100 + 2 * C + 3]
    m = assemble_crc(v)
    assert parse_index(m)[1] == 3 and zlib.decompress(m, 31) == v
    rng = np.random.default_rng(FLIP_SEED)
    flips, per = flips_of(m, rng)
    print("assembled member: flips per chunk that keep the structure and change the bytes:", per, "of", FLIPS)
    assert all(x >= 50 for x in per), per
    for j, b in flips:  # (the plain model serves them: this is the gap)
        assert read_range(b, j * C, 1) is not None and read_range_verified(b, j * C, 1) is None
    check_flips(ctx, v, m, flips, True)
    # the same on a member the library wrote (dynamic blocks)
    name, v = vals[2]
    m = members[2]
    assert len(v) == 2 * C + 3
    flips, per = flips_of(m, np.random.default_rng(FLIP_SEED))
    print("written member: flips per chunk that keep the structure and change the bytes:", per, "of", FLIPS)
    assert len(flips) >= 1, per
    check_flips(ctx, v, m, flips, False)


def test_a_damaged_crc_entry(ctx, vals, members):
    import pmc_codec
    name, v = vals[3]
    m = members[3]
    k = parse_index(m)[1]
    at = plan(len(v))[4]
    assert k == 4 and at == 16 + 4 * k + 8
    st = pmc_codec.Store(ctx, 8 << 20)
    try:
        for j in range(k):
            b = put(m, at + 4 * j + (j & 3), [m[at + 4 * j + (j & 3)] ^ 0x40])
            assert zlib.decompress(b, 31) == v and parse_chunk_crcs(b)[j] != chunk_crcs(v)[j]
            reqs = [(b, off, ln) for off, ln in ranges_for(len(v), C)] + [(b, q * C + 9, 20) for q in range(k)]
            want = [read_range_verified(b, off, ln) for _, off, ln in reqs]
            assert sum(1 for w in want if w is None) >= 3 and sum(1 for w in want if w) >= 3
            rc, dlen, slots = ranged_call(ctx, reqs)
            for i, w in enumerate(want):
                r = range_of(len(v), 15, reqs[i][1], reqs[i][2])
                touches = r[1] > 0 and r[2] <= j < r[2] + r[3]
                assert (w is None) == touches
                if w is None:
                    assert (rc[i], dlen[i]) == (pmc_codec.E_NO_INDEX, 0), (j, i)
                else:
                    assert (rc[i], dlen[i], slots[i]) == (0, len(w), w) and w == v[reqs[i][1]:reqs[i][1] + reqs[i][2]], (j, i)
            # the full read does not look at the subfield
            assert ctx.decompress_many([b]) == [(0, v)]
            c = Case(f"entry{j}", b, len(v))
            assert (c.rc, c.out) == (0, v)
            a = ctx.index_counts()
            check_route(ctx, [c], len(v))
            assert ctx.index_counts()["completed"] >= a["completed"] + 1
        # the store returns every range, through its whole read where the ranged call declines: the entry of
        # chunk 1 is damaged inside the heap
        ext, rc = st.put([v])
        assert rc == [0] and st.members(ext, 1) == [m]
        hip = ctypes.CDLL("libamdhip64.so")
        byte = bytes([m[at + 4] ^ 1])
        assert hip.hipMemcpy(ctypes.c_void_p(st.data_ptr() + ext[0].off + at + 4), byte, ctypes.c_size_t(1), 1) == 0
        dam = st.members(ext, 1)[0]
        assert dam == put(m, at + 4, byte) and parse_chunk_crcs(dam)[1] != chunk_crcs(v)[1]
        pairs = ranges_for(len(v), C)
        (res, got) = counted(ctx, lambda: st.get_range(repeat_extents(ext, [0] * len(pairs)), pairs))
        assert res == [(0, v[off:off + ln]) for off, ln in pairs]
        touching = sum(1 for off, ln in pairs if read_range_verified(dam, off, ln) is None)
        assert touching >= 3 and got[1] == touching and got[4] == touching, (got, touching)
        assert st.get(ext, 1) == [(0, v)]
    finally:
        st.close()


def test_damaged_subfield_and_require(ctx, golden, vals, members, plain):
    import pmc_codec
    v = (golden.corpus * 4)[100:100 + 2 * C + 3]
    defects = {name: assemble_crc(v, sub=sub) for name, sub in crc_defects(v).items()}
    good = assemble_crc(v)
    rs = [(5, 100), (C - 3, 9), (len(v) - 50, 50), (0, len(v)), (len(v), 4), (C, 0)]
    reqs = [(m, off, ln) for m in defects.values() for off, ln in rs]
    want = [v[off:off + ln] for _ in defects for off, ln in rs]
    live = sum(1 for w in want if w)
    assert all(parse_index(m) is not None and parse_chunk_crcs(m) is None for m in defects.values())
    # mode 0: served unverified, as a plain indexed member is
    assert ctx.range_verify == 0
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
    assert not rc.any() and [int(x) for x in dlen] == [len(w) for w in want] and slots == want
    assert got[0] == len(reqs) and got[2] > 0 and got[3:] == (0, 0), got
    try:
        ctx.range_verify = 1
        assert ctx.range_verify == 1
        # mode 1: declined at the scan -- empty ranges and capacity verdicts included -- and nothing is decoded
        (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
        assert list(rc) == [pmc_codec.E_NO_INDEX] * len(reqs) and not dlen.any() and all(untouched(s) for s in slots)
        assert got == (0, len(reqs), 0, 0, 0), got
        (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, [(plain[2], 0, 100), (assemble(v), 0, 100)], caps=[99, 99]))
        assert list(rc) == [pmc_codec.E_NO_INDEX] * 2 and got == (0, 2, 0, 0, 0), got
        # members with CRCs keep every verdict in its order
        reqs2 = [(good, off, ln) for off, ln in rs] + [(members[2], off, ln) for off, ln in rs]
        want2 = [v[off:off + ln] for off, ln in rs] + [vals[2][1][off:off + ln] for off, ln in rs]
        (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs2))
        assert not rc.any() and slots == want2 and got[3] == got[2] > 0 and got[4] == 0, got
        rc, dlen, slots = ranged_call(ctx, [(good, 0, 100)], caps=[99])
        assert (int(rc[0]), int(dlen[0])) == (pmc_codec.E_CAPACITY, 100)
        # the store on a "require" context: right bytes for plain indexed, CRC-indexed, level-9 and small extents
        values = [vals[3][1], vals[0][1], b"x" * 5000, b"tiny"]
        st = pmc_codec.Store(ctx, 16 << 20)
        try:
            exts = []
            for crc, lvl in ((True, pmc_codec.LEVEL_FAST_ALL), (False, pmc_codec.LEVEL_FAST_ALL), (True, pmc_codec.LEVEL_EXACT)):
                ctx.index_crc, ctx.level = crc, lvl
                ext, prc = st.put(values)
                assert prc == [0] * len(values)
                exts.append(ext)
            ms = [st.members(e, len(values)) for e in exts]
            assert pmc_codec.index_crc_info(ms[0][0]) and pmc_codec.index_info(ms[1][0]) and not pmc_codec.index_crc_info(ms[1][0])
            assert ms[2][0][3] == 0 and ms[2][0][8] == 2
            for e, (served, verified) in zip(exts, ((True, True), (False, False), (False, False))):
                pairs = [(i, off, ln) for i, x in enumerate(values) for off, ln in ranges_for(max(len(x), 8), C)]
                a = counts(ctx)
                res = st.get_range(repeat_extents(e, [i for i, _, _ in pairs]), [(off, ln) for _, off, ln in pairs])
                d = counts(ctx) - a
                bad = [(i, off, ln, r[0]) for (i, off, ln), r in zip(pairs, res) if r != (0, values[i][off:off + ln])]
                assert not bad, bad[:8]
                assert (d[0] > 0) == served and (d[3] > 0) == verified and d[4] == 0, d
                assert served or d[2] == 0, d
        finally:
            st.close()
    finally:
        ctx.range_verify = 0
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index_crc = True


def test_more_items_than_one_grid_pass_with_crcs(ctx, vals, members):
    """100,000 requests of 16 bytes on members with chunk CRCs: every item is an edge chunk whose row the lane
    reuses in its next round, so the check must have read it before (csrc/pmc_plan.hpp plan_range: more requests
    than rows).  One member carries a wrong entry for chunk 1: exactly the requests that touch it are declined."""
    import pmc_codec
    pick = [(v, m) for (name, v), m in zip(vals, members) if name != RANDOM]
    v3, m3 = pick[3]
    at = plan(len(v3))[4] + 4
    pick.append((v3, put(m3, at, [m3[at] ^ 0x80])))
    rng = np.random.default_rng(20266)
    n = 100000
    which = rng.integers(0, len(pick), n)
    offs = np.array([int(rng.integers(0, len(pick[w][0]) - 16)) for w in which], dtype=np.int64)
    for k in range(64):  # (across an edge: two items)
        if len(pick[which[k]][0]) >= C + 8:
            offs[k] = C - 8
    reqs = [(pick[w][1], int(o), 16) for w, o in zip(which, offs)]
    base = np.concatenate([[0], np.cumsum([len(v) for v, _ in pick])[:-1]])
    flat = np.frombuffer(b"".join(v for v, _ in pick), dtype=np.uint8)
    want = flat[(base[which] + offs)[:, None] + np.arange(16)[None, :]]
    k0, k1 = offs >> 15, (offs + 15) >> 15
    chunks = int((k1 - k0 + 1).sum())
    hit = (which == len(pick) - 1) & (k0 <= 1) & (k1 >= 1)
    mism = int(hit.sum())
    assert chunks > n and 1000 < mism < n // 4
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
    assert (rc[hit] == pmc_codec.E_NO_INDEX).all() and not dlen[hit].any()
    assert not rc[~hit].any() and (dlen[~hit] == 16).all()
    out = np.frombuffer(b"".join(slots), dtype=np.uint8).reshape(n, 16)
    assert (out[~hit] == want[~hit]).all()
    assert got == (n - mism, mism, chunks, chunks - mism, mism), (got, chunks, mism)


def test_group_sets_all_or_none(ctx):
    import pmc_codec
    L = pmc_codec.lib()
    g = ctypes.c_void_p()
    assert L.pmc_group_create((ctypes.c_int * 2)(0, 0), 2, ctypes.byref(g)) == 0
    try:
        v = bytes(range(256)) * 300
        k = -(-len(v) // C)
        kh = np.array([L.pmc_key_hash(b"key%d" % i, len(b"key%d" % i)) for i in range(8)], dtype=np.uint64)

        def compress():
            n = 8
            lens = np.full(n, len(v), dtype=np.uint32)
            caps = np.full(n, pmc_codec.gzip_bound(len(v)), dtype=np.uint32)
            soff = (np.arange(n) * len(v)).astype(np.uint64)
            doff = (np.arange(n) * int(caps[0])).astype(np.uint64)
            out = ctypes.create_string_buffer(int(caps.sum()) + 64)
            glen, grc = np.zeros(n, dtype=np.uint32), np.full(n, 7, dtype=np.int32)
            assert L.pmc_group_compress_batch(g, v * n, soff.ctypes.data, lens.ctypes.data, kh.ctypes.data, 128, n, out,
                                              doff.ctypes.data, caps.ctypes.data, glen.ctypes.data, grc.ctypes.data,
                                              len(v)) == 0
            assert (grc == 0).all()
            return {out.raw[int(doff[i]):int(doff[i]) + int(glen[i])] for i in range(n)}

        assert L.pmc_group_set_level(g, pmc_codec.LEVEL_FAST_ALL) == 0 and L.pmc_group_set_index(g, 1) == 0
        off = compress()
        assert len(off) == 1 and pmc_codec.index_info(next(iter(off))) == (C, k) and not pmc_codec.index_crc_info(next(iter(off)))
        for bad in (2, -1):  # a bad value leaves every member context as it was
            assert L.pmc_group_set_index_crc(g, bad) == pmc_codec.E_ARG
        assert compress() == off
        assert L.pmc_group_set_index_crc(g, 1) == 0
        on = compress()  # (both member contexts: the keys route to each of them)
        assert len(on) == 1 and pmc_codec.index_crc_info(next(iter(on))) == chunk_crcs(v)
        assert L.pmc_group_set_index_crc(g, 2) == pmc_codec.E_ARG and compress() == on
        assert L.pmc_group_set_index_crc(g, 0) == 0 and compress() == off
    finally:
        L.pmc_group_destroy(g)

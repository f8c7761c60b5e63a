"""GPU: the preset dictionary (include/pmc_codec.h "preset dictionary").

At the fast level a value of D + len <= 16382 becomes a dictionary member whose tokens are
tests/dict_model.py's; zlib's raw inflate with the same zdict reads it, and so does the library through every
entry point; members without the mark, foreign ones included, decode as ever in the same batch; a wrong or
missing dictionary, a distance before the dictionary's start and an oversized ISIZE give PMC_Z_DATA_ERROR;
the no-dictionary paths are untouched; and on two seeded JSON-slice sets the members are no larger in total
than zlib level 1's with the same dictionary and at most 0.75 of zlib level 9's without one
(tests/golden/dict_baseline.json)."""
import ctypes
import json
import os
import struct
import zlib

import numpy as np
import pytest

from deflate_dissect import dissect
from dict_model import dict_tokens
from dict_values import (BASELINE_SETS, SPAN, baseline_dictionary, baseline_values, crc0_bytes, edge_pairs,
                         uses_dictionary)
from fast_model import fast_tokens
from fast_values import alnum, edge_values, json_slices

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIPELINE_N = 4200  # more members than the wave-kernel-only route of a device batch takes (4,096)


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    c.level = pmc_codec.LEVEL_FAST
    assert c.dictionary_id == 0
    yield c
    c.close()


def device_compress(ctx, values):
    import torch
    from pmc_codec import device as D
    out, rc = D.compress(ctx, D.pack(values))
    torch.cuda.synchronize()
    assert int((rc != 0).sum()) == 0, rc
    return out.host_items()


def gz(v, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(v) + c.flush()


def device_decompress(ctx, members, caps, pipeline, max_len=None):
    """[(rc, bytes)] through the device-resident call: the wave kernel alone (a small batch), or -- padded
    with copies of a plain member to PIPELINE_N -- the record / lane kernels with the wave kernels behind.
    max_len: the call's bound on the decompressed sizes (default: the largest capacity)."""
    import torch
    from pmc_codec import device as D
    n = len(members)
    pad = gz(b"padding " * 8)
    if pipeline:
        members = list(members) + [pad] * (PIPELINE_N - n)
        caps = list(caps) + [64] * (PIPELINE_N - n)
    if max_len is None:
        back, rc = D.decompress(ctx, D.pack(members), caps)
    else:
        b = D.pack(members)
        dst, doff, dcap = D.slots_for(caps)
        dlen = torch.zeros(b.n, dtype=torch.int32, device="cuda")
        rc = torch.full((b.n,), 7, dtype=torch.int32, device="cuda")
        ctx.decompress_device(b.data, b.off, b.len, dst, doff, dcap, dlen, rc, max_len, D.stream_handle())
        back = D.Batch(dst, doff, dlen, b.n, max(caps))
    torch.cuda.synchronize()
    rcs, items = rc.cpu().numpy().tolist(), back.host_items()
    if pipeline:
        assert rcs[n:] == [0] * (PIPELINE_N - n) and set(items[n:]) == {b"padding " * 8}
    return list(zip(rcs[:n], items[:n]))


@pytest.fixture(scope="module")
def edge(golden):
    return edge_pairs(golden.corpus)


@pytest.fixture(scope="module")
def no_dict_members(ctx, golden):
    """Fast members of fast_values' edge list before any dictionary was set on the context."""
    assert ctx.dictionary_id == 0
    return device_compress(ctx, [v for _, v in edge_values(golden.corpus)])


@pytest.fixture(scope="module")
def edge_members(ctx, edge, no_dict_members):
    """{name: member}: the pairs of each dictionary as one ragged device batch (computed once)."""
    out = {}
    by_dict = {}
    for name, d, v in edge:
        by_dict.setdefault(d, []).append((name, v))
    for d, items in by_dict.items():
        ctx.set_dictionary(d)
        assert ctx.dictionary_id == zlib.crc32(d)
        for (name, _), m in zip(items, device_compress(ctx, [v for _, v in items])):
            out[name] = m
    ctx.set_dictionary(None)
    return out


@pytest.fixture(scope="module")
def base(ctx, golden, edge_members):
    """The baseline dictionary, its two value sets and their dictionary members."""
    d = baseline_dictionary(golden.corpus)
    ctx.set_dictionary(d)
    sets = {name: baseline_values(golden.corpus, name) for name in BASELINE_SETS}
    mem = {name: device_compress(ctx, vals) for name, vals in sets.items()}
    ctx.set_dictionary(None)
    return d, sets, mem


def frame(raw, value, mtime, xfl=4):
    return b"\x1f\x8b\x08\x00" + struct.pack("<I", mtime) + bytes([xfl, 3]) + raw + struct.pack(
        "<II", zlib.crc32(value), len(value))


def test_spec_parity(ctx, edge, edge_members):
    import pmc_codec
    stored = marked = 0
    for name, d, v in edge:
        m = edge_members[name]
        assert len(m) <= pmc_codec.gzip_bound(len(v)), name
        assert m[:4] == b"\x1f\x8b\x08\x00" and m[8] == 4, name
        assert m[-8:] == struct.pack("<II", zlib.crc32(v), len(v)), name
        blocks = dissect(m)
        assert len(blocks) == 1, name
        if uses_dictionary(d, v):
            marked += 1
            assert m[4:8] == struct.pack("<I", zlib.crc32(d)), name
            assert zlib.decompressobj(-15, zdict=d).decompress(m[10:-8]) == v, name
            want = dict_tokens(d, v)
        else:  # D + len = 16383: a plain fast member
            assert len(d) + len(v) == SPAN + 1 and m[4:8] == bytes(4), name
            assert zlib.decompress(m, 31) == v, name
            want = fast_tokens(v)
        if blocks[0]["type"] == 0:
            # (a stored block has no tokens to compare; the patterns, each built for one rule, are never stored)
            assert name.startswith("d") and name[1].isdigit(), name
            stored += 1
            continue
        got = blocks[0]["tokens"]
        if got != want:
            k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
            raise AssertionError(f"{name}: tokens differ at #{k}: {got[k:k + 3]} vs {want[k:k + 3]}")
    assert marked == len(edge) - 9 and stored < len(edge) // 2  # (a stored block has no tokens to compare)
    assert ctx.guard_counts()["sort"] == 0


def test_own_round_trip_and_identical_members_from_every_entry_point(ctx, golden, edge, edge_members, base):
    import torch
    import pmc_codec
    from pmc_codec import device as D
    L = pmc_codec.lib()
    d, sets, mem = base
    ctx.set_dictionary(d)
    try:
        # the edge values of the 2 KiB dictionary size (their dictionary is another slice: new members), the
        # patterns' values and a few of each baseline set
        vals = [v for n, _, v in edge if n.startswith("d2048_") or not n.startswith("d")]
        vals += sets["256"][:8] + sets["1k"][:4]
        want = device_compress(ctx, vals)
        n = len(vals)
        assert want[-12:] == mem["256"][:8] + mem["1k"][:4]  # (batch and position do not matter)
        marks = [m[4:8] == struct.pack("<I", zlib.crc32(d)) for m in want]
        assert sum(marks) == n - 1 and not marks[[len(v) for v in vals].index(SPAN - 2048 + 1)]
        caps = [len(v) for v in vals]
        # device: the wave kernel alone, and behind the record / lane kernels
        for pipeline in (False, True):
            assert device_decompress(ctx, want, caps, pipeline) == [(0, v) for v in vals], pipeline
        # host batch; one value at a time (the latency path)
        assert ctx.compress_many(vals) == [(0, m) for m in want]
        assert ctx.decompress_many(want) == [(0, v) for v in vals]
        before = ctx.path_counts()["latency_decompress"]
        for v, m in list(zip(vals, want))[::3]:
            out = ctypes.create_string_buffer(pmc_codec.gzip_bound(len(v)))
            olen = ctypes.c_size_t(0)
            assert L.pmc_gzip_compress(ctx.handle, v, len(v), out, len(out), ctypes.byref(olen)) == 0
            assert out.raw[:olen.value] == m
            assert ctx.decompress_many([m]) == [(0, v)]
        assert ctx.path_counts()["latency_decompress"] > before
        # pinned, pipelined in chunks of 7
        lens = np.array([len(v) for v in vals], dtype=np.int64)
        bnd = np.array([pmc_codec.gzip_bound(int(x)) for x in lens], dtype=np.int64)
        soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
        doff = np.concatenate([[0], np.cumsum(bnd)[:-1]])
        pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
        src = torch.frombuffer(bytearray(b"".join(vals) + bytes(64)), dtype=torch.uint8).pin_memory()
        dst = torch.zeros(int(bnd.sum()) + 64, dtype=torch.uint8).pin_memory()
        dlen, rc = torch.zeros(n, dtype=torch.int32).pin_memory(), torch.full((n,), 7, dtype=torch.int32).pin_memory()
        ctx.compress_pinned(src, pin(soff, np.int64), pin(lens, np.int32), dst, pin(doff, np.int64), pin(bnd, np.int32),
                            dlen, rc, int(lens.max()), 7)
        assert (rc.numpy() == 0).all()
        raw = dst.numpy().tobytes()
        assert [raw[int(doff[k]):int(doff[k]) + int(dlen[k])] for k in range(n)] == want
        mlen = np.array([len(m) for m in want], dtype=np.int64)
        moff = np.concatenate([[0], np.cumsum(mlen)[:-1]])
        msrc = torch.frombuffer(bytearray(b"".join(want) + bytes(64)), dtype=torch.uint8).pin_memory()
        back = torch.zeros(int(lens.sum()) + 64, dtype=torch.uint8).pin_memory()
        blen, brc = torch.zeros(n, dtype=torch.int32).pin_memory(), torch.full((n,), 7, dtype=torch.int32).pin_memory()
        ctx.decompress_pinned(msrc, pin(moff, np.int64), pin(mlen, np.int32), back, pin(soff, np.int64),
                              pin(lens, np.int32), blen, brc, int(lens.max()), 7)
        assert (brc.numpy() == 0).all()
        raw = back.numpy().tobytes()
        assert [raw[int(soff[k]):int(soff[k]) + int(blen[k])] for k in range(n)] == vals
        # store, all three frames
        st = pmc_codec.Store(ctx, 16 << 20)
        ext, src_rc = st.put(vals)
        assert src_rc == [0] * n
        assert st.members(ext, n) == want
        assert st.get(ext, n) == [(0, v) for v in vals]
        assert st.get(ext, n, pmc_codec.FRAME_CUSTOM) == [(0, v + b"\x1f") for v in vals]
        assert st.get(ext, n, pmc_codec.FRAME_RESP) == [(0, b"$%d\r\n" % len(v) + v + b"\r\n") for v in vals]
        st.close()
        # slab
        slab = pmc_codec.Slab(ctx, 64, 16382)
        b = D.pack(vals)
        slots = torch.from_numpy(np.random.default_rng(9).permutation(64)[:n].astype(np.int32)).cuda()
        rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        slab.set(b.data, b.off, b.len, slots, rc, D.stream_handle())
        torch.cuda.synchronize()
        assert int((rc != 0).sum()) == 0
        lens_t = torch.zeros(64, dtype=torch.int32, device="cuda")
        data_t = torch.zeros(slab.stride * 64, dtype=torch.uint8, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")
        for t, p, nb in ((lens_t, slab.lengths_ptr(), 4 * 64), (data_t, slab.data_ptr(), slab.stride * 64)):
            assert hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(nb), 3) == 0
        sl, ln, data = slots.cpu().numpy(), lens_t.cpu().numpy(), data_t.cpu().numpy().tobytes()
        assert [data[int(s) * slab.stride:int(s) * slab.stride + int(ln[s])] for s in sl] == want
        dst2, doff_t, dcap = D.slots_for([len(v) for v in vals])
        dlen2 = torch.zeros(n, dtype=torch.int32, device="cuda")
        grc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        slab.get(slots, dst2, doff_t, dcap, dlen2, grc, D.stream_handle())
        torch.cuda.synchronize()
        assert int((grc != 0).sum()) == 0
        assert D.Batch(dst2, doff_t, dlen2, n, 0).host_items() == vals
        slab.close()
        # a group of two contexts on device 0
        g = ctypes.c_void_p()
        assert L.pmc_group_create((ctypes.c_int * 2)(0, 0), 2, ctypes.byref(g)) == 0
        try:
            assert L.pmc_group_set_dictionary(g, bytes(8193), 8193) == pmc_codec.E_ARG
            assert L.pmc_group_set_level(g, pmc_codec.LEVEL_FAST) == 0
            assert L.pmc_group_set_dictionary(g, d, len(d)) == 0
            kh = np.array([L.pmc_key_hash(b"key%d" % i, len(b"key%d" % i)) for i in range(n)], dtype=np.uint64)
            out = ctypes.create_string_buffer(int(bnd.sum()) + 64)
            glen, grc2 = np.zeros(n, dtype=np.uint32), np.full(n, 7, dtype=np.int32)
            u = lambda a, dt: np.ascontiguousarray(a).astype(dt)  # noqa: E731
            u_soff, u_len, u_cap, u_doff = u(soff, np.uint64), u(lens, np.uint32), u(bnd, np.uint32), u(doff, np.uint64)
            assert L.pmc_group_compress_batch(g, b"".join(vals), u_soff.ctypes.data, u_len.ctypes.data, kh.ctypes.data,
                                              128, n, out, u_doff.ctypes.data, u_cap.ctypes.data, glen.ctypes.data,
                                              grc2.ctypes.data, int(lens.max())) == 0
            assert (grc2 == 0).all()
            assert [out.raw[int(doff[k]):int(doff[k]) + int(glen[k])] for k in range(n)] == want
        finally:
            L.pmc_group_destroy(g)
    finally:
        ctx.set_dictionary(None)


@pytest.fixture(scope="module")
def mixed(ctx, golden, base, no_dict_members):
    """[(member, value, needs the dictionary)]: dictionary members, plain fast members, level-9 members and
    foreign members with a nonzero MTIME and XFL 4."""
    import pmc_codec
    d, sets, mem = base
    out = [(m, v, True) for name in sets for m, v in zip(mem[name], sets[name])]
    ev = [v for _, v in edge_values(golden.corpus)]
    out += [(m, v, False) for m, v in zip(no_dict_members, ev) if len(v) <= 4097][:60]
    out += [(g, r, False) for r, g in golden.pairs()[:60] if 0 < len(r) <= 16384]
    for k, v in enumerate(sets["1k"][:20]):
        c = zlib.compressobj(1, zlib.DEFLATED, 31)
        f = bytearray(c.compress(v) + c.flush())
        f[4:8] = struct.pack("<I", 1700000000 + k)
        assert f[3] == 0 and f[8] == 4
        out.append((bytes(f), v, False))
    # one foreign member whose MTIME happens to be the id but whose XFL is not 4, one with FLG.FNAME
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    raw = c.compress(sets["1k"][0]) + c.flush()
    out.append((frame(raw, sets["1k"][0], zlib.crc32(d), xfl=2), sets["1k"][0], False))
    named = b"\x1f\x8b\x08\x08" + struct.pack("<I", zlib.crc32(d)) + b"\x04\x03" + b"n\x00" + raw + struct.pack(
        "<II", zlib.crc32(sets["1k"][0]), 1024)
    assert zlib.decompress(named, 31) == sets["1k"][0]
    out.append((named, sets["1k"][0], False))
    order = np.random.default_rng(3).permutation(len(out))
    return [out[i] for i in order]


@pytest.mark.parametrize("pipeline", [False, True])
def test_mixed_batch(ctx, base, mixed, pipeline):
    d = base[0]
    ctx.set_dictionary(d)
    try:
        got = device_decompress(ctx, [m for m, _, _ in mixed], [len(v) for _, v, _ in mixed], pipeline)
        assert got == [(0, v) for _, v, _ in mixed]
        if not pipeline:  # the host call's latency route: the same kernel, the same answers
            few = mixed[:48]
            assert ctx.decompress_many([m for m, _, _ in few]) == [(0, v) for _, v, _ in few]
    finally:
        ctx.set_dictionary(None)


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("other", [None, b"another dictionary altogether, of a few dozen bytes"])
def test_wrong_or_missing_dictionary(ctx, mixed, other, pipeline):
    import pmc_codec
    ctx.set_dictionary(other)
    try:
        got = device_decompress(ctx, [m for m, _, _ in mixed], [len(v) for _, v, _ in mixed], pipeline)
        errors = 0
        for (rc, b), (_, v, needs) in zip(got, mixed):
            if needs:
                assert rc == pmc_codec.Z_DATA_ERROR or (rc, b) == (0, v)
                errors += rc != 0
            else:
                assert (rc, b) == (0, v)  # (members around a failing one are unaffected)
        # (the size condition -- a quarter saved against level 9 -- cannot hold unless most of the 300
        # members reach into their dictionary)
        assert errors > 150
    finally:
        ctx.set_dictionary(None)


@pytest.mark.parametrize("pipeline", [False, True])
def test_bad_dictionary_members(ctx, golden, pipeline):
    """A distance that reaches before the dictionary's first byte, and a marked member whose ISIZE exceeds
    16382 - D: PMC_Z_DATA_ERROR, the members around them unaffected."""
    import pmc_codec
    rng = np.random.default_rng(11)
    useful = json_slices(golden.corpus, 1024, 1, 501)[0]
    d4k = useful + alnum(rng, 3072)  # what helps lies 3 KiB and more before the value
    d1k = alnum(rng, 1024)
    v = useful[100:700]
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, d4k)
    raw = c.compress(v) + c.flush()
    assert len(raw) < 40  # (it is one long match into the 4 KiB dictionary)
    ident = zlib.crc32(d1k)
    before_start = frame(raw, v, ident)
    # a correct dictionary member of the 1 KiB dictionary, as zlib writes it; then its ISIZE overstated
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, d1k)
    good_v = d1k[10:300] + b"tail"
    good = frame(c.compress(good_v) + c.flush(), good_v, ident)
    big = bytearray(good)
    big[-4:] = struct.pack("<I", SPAN - 1024 + 1)
    plain = gz(v)
    members = [plain, before_start, good, bytes(big), plain]
    caps = [len(v), len(v), len(good_v), SPAN - 1024 + 1, len(v)]
    ctx.set_dictionary(d1k)
    try:
        got = device_decompress(ctx, members, caps, pipeline)
        assert [rc for rc, _ in got] == [0, pmc_codec.Z_DATA_ERROR, 0, pmc_codec.Z_DATA_ERROR, 0]
        assert [b for _, b in got] == [v, b"", good_v, b"", v]
        # the same member behind its own 4 KiB dictionary decodes
        ctx.set_dictionary(d4k)
        assert device_decompress(ctx, [frame(raw, v, zlib.crc32(d4k))], [len(v)], pipeline) == [(0, v)]
    finally:
        ctx.set_dictionary(None)


@pytest.mark.parametrize("pipeline", [False, True])
def test_capacity_and_isize_above_the_calls_max_len(ctx, golden, base, pipeline):
    """max_len bounds the decompressed sizes, not the capacities (a slab passes its own): dictionary members
    whose capacity and ISIZE lie above it, one of them longer than the input the call's first pass stages,
    still decode, or get a clean verdict, and the members beside them in the same workgroup are unaffected."""
    import pmc_codec
    d, sets, mem = base
    ctx.set_dictionary(d)
    try:
        big = [json_slices(golden.corpus, 3000, 1, 611)[0], (d[:1500] * 2), json_slices(golden.corpus, SPAN - 2048, 1, 612)[0]]
        big_m = device_compress(ctx, big)
        assert all(m[4:8] == struct.pack("<I", zlib.crc32(d)) for m in big_m)
        # (the first pass of a max_len = 256 call stages members of up to gzip_bound(256) + 64 bytes)
        assert len(big_m[2]) > pmc_codec.gzip_bound(256) + 64 > len(big_m[1])
        overstated = bytearray(big_m[1])  # ISIZE says 256: the stream runs past the image it was routed by
        overstated[-4:] = struct.pack("<I", 256)
        small = list(zip(mem["256"][:40], sets["256"][:40]))
        plain = [(gz(v), v) for v in sets["256"][40:60]]
        items = []
        for k, (m, v) in enumerate(small + plain):
            items.append((m, v, 256, 0))
            if k % 12 == 5:
                j = (k // 12) % 3
                items.append((big_m[j], big[j], 4096 if j < 2 else SPAN - 2048, 0))
            if k % 12 == 11:
                items.append((bytes(overstated), b"", 4096, pmc_codec.Z_DATA_ERROR))
                items.append((big_m[0], b"", 2000, pmc_codec.E_CAPACITY))
        got = device_decompress(ctx, [m for m, _, _, _ in items], [c for _, _, c, _ in items], pipeline, max_len=256)
        assert [rc for rc, _ in got] == [rc for _, _, _, rc in items]
        # (a PMC_E_CAPACITY answer carries the size needed, not bytes)
        assert [b for (rc, b) in got if rc != pmc_codec.E_CAPACITY] == [v for _, v, _, rc in items if rc != pmc_codec.E_CAPACITY]
    finally:
        ctx.set_dictionary(None)


def test_no_regression_without_a_dictionary(ctx, golden, no_dict_members, edge_members):
    import pmc_codec
    vals = [v for _, v in edge_values(golden.corpus)]
    assert ctx.dictionary_id == 0  # (edge_members set and cleared several)
    assert device_compress(ctx, vals) == no_dict_members
    # at level 9 a dictionary has no effect on compress
    pairs = [(r, g) for r, g in golden.pairs() if r][:100]
    d = baseline_dictionary(golden.corpus)
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        ctx.set_dictionary(d)
        assert ctx.level == pmc_codec.LEVEL_EXACT and ctx.dictionary_id == zlib.crc32(d)
        assert device_compress(ctx, [r for r, _ in pairs]) == [g for _, g in pairs]
        with pytest.raises(ValueError):
            ctx.set_dictionary(bytes(pmc_codec.DICT_MAX + 1))
        with pytest.raises(ValueError):  # (CRC-32 0 stands for "no dictionary")
            ctx.set_dictionary(crc0_bytes())
        assert ctx.dictionary_id == zlib.crc32(d)
    finally:
        ctx.set_dictionary(None)
        ctx.level = pmc_codec.LEVEL_FAST


def test_size_conditions(ctx, base):
    """On both baseline sets the dictionary members sum to at most zlib level 1's total with the same zdict,
    and to at most 0.75 of zlib level 9's without a dictionary."""
    d, sets, mem = base
    with open(os.path.join(GOLDEN, "dict_baseline.json")) as f:
        doc = json.load(f)
    assert doc["dict_crc32"] == zlib.crc32(d)
    for name, (size, count) in BASELINE_SETS.items():
        b = doc["sets"][name]
        assert (b["size"], b["count"]) == (size, count)
        total = sum(map(len, mem[name]))
        print(f"dict {name}: {total} B, level 1 + zdict {b['level1_dict_total']} "
              f"({total / b['level1_dict_total']:.4f}), level 9 + zdict {b['level9_dict_total']} "
              f"({total / b['level9_dict_total']:.4f}), level 9 {b['level9_total']} ({total / b['level9_total']:.4f})")
        assert total <= b["level1_dict_total"], (name, total, b["level1_dict_total"])
        assert total <= 0.75 * b["level9_total"], (name, total, b["level9_total"])
    assert ctx.guard_counts()["sort"] == 0

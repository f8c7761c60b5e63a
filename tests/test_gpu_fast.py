"""GPU: the fast compression level (PMC_LEVEL_FAST, include/pmc_codec.h "compression level").

The fast front's token sequence must be tests/fast_model.py's for every value of the edge list; a fast
member is one valid single-block gzip member (header byte 8 = 4) whatever entry point, batch size or batch
position produced it; the library's own decompress takes it; level 9 on the same context is untouched; and
on two seeded JSON-slice sets the fast members are no larger in total than zlib level 1's
(tests/golden/fast_baseline.json)."""
import ctypes
import json
import os
import zlib

import numpy as np
import pytest

from deflate_dissect import dissect
from fast_model import fast_tokens
from fast_values import BASELINE_SETS, edge_values, json_slices

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    assert c.level == pmc_codec.LEVEL_EXACT  # the default (PMC_LEVEL unset)
    c.level = pmc_codec.LEVEL_FAST
    assert c.level == pmc_codec.LEVEL_FAST
    yield c
    c.close()


def device_compress(ctx, values):
    import torch
    from pmc_codec import device as D
    out, rc = D.compress(ctx, D.pack(values))
    torch.cuda.synchronize()
    assert int((rc != 0).sum()) == 0, rc
    return out.host_items()


@pytest.fixture(scope="module")
def edge(golden):
    return edge_values(golden.corpus)


@pytest.fixture(scope="module")
def edge_members(ctx, edge):
    """The whole edge list as one ragged device batch at the fast level (computed once)."""
    return device_compress(ctx, [v for _, v in edge])


def test_spec_parity(ctx, edge, edge_members):
    import pmc_codec
    stored = 0
    for (name, v), m in zip(edge, edge_members):
        assert m[:4] == b"\x1f\x8b\x08\x00" and m[8] == 4, name
        assert len(m) <= pmc_codec.gzip_bound(len(v)), name
        assert zlib.decompress(m, 31) == v, name
        blocks = dissect(m)
        assert len(blocks) == 1, name
        if blocks[0]["type"] == 0:
            stored += 1
            continue
        got, want = blocks[0]["tokens"], fast_tokens(v)
        if got != want:
            k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
            raise AssertionError(f"{name}: tokens differ at #{k}: {got[k:k + 3]} vs {want[k:k + 3]}")
    assert stored < len(edge) // 2  # (a stored block has no tokens to compare)
    assert ctx.guard_counts()["sort"] == 0


def test_deterministic_across_batches_and_positions(ctx, edge, edge_members):
    vals = [v for _, v in edge]
    perm = np.random.default_rng(5).permutation(len(vals))[:len(vals) - 7]
    got = device_compress(ctx, [vals[i] for i in perm])
    assert got == [edge_members[i] for i in perm]
    # one value at 70 indices of a batch: several work-counter grabs at 4, 2 and 1 values per grab
    by = dict(zip((n for n, _ in edge), range(len(edge))))
    for name in ("json257", "json1025", "json4095"):
        i = by[name]
        assert set(device_compress(ctx, [vals[i]] * 70)) == {edge_members[i]}, name


def test_every_entry_point_gives_the_same_member(ctx, golden, edge, edge_members):
    import torch
    import pmc_codec
    from pmc_codec import device as D
    L = pmc_codec.lib()
    pick = [i for i, (n, v) in enumerate(edge) if n.startswith("json") or n in ("lazy", "collide", "pos0", "too_far")]
    vals, want = [edge[i][1] for i in pick], [edge_members[i] for i in pick]
    n = len(vals)
    assert 20 <= n <= 40
    # host batch
    assert ctx.compress_many(vals) == [(0, m) for m in want]
    # single value
    for v, m in list(zip(vals, want))[::5]:
        out = ctypes.create_string_buffer(pmc_codec.gzip_bound(len(v)))
        olen = ctypes.c_size_t(0)
        assert L.pmc_gzip_compress(ctx.handle, v, len(v), out, len(out), ctypes.byref(olen)) == 0
        assert out.raw[:olen.value] == m
    # pinned, pipelined in chunks of 7
    lens = np.array([len(v) for v in vals], dtype=np.int64)
    caps = np.array([pmc_codec.gzip_bound(int(x)) for x in lens], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
    doff = np.concatenate([[0], np.cumsum(caps)[:-1]])
    pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
    src = torch.frombuffer(bytearray(b"".join(vals) + bytes(64)), dtype=torch.uint8).pin_memory()
    dst = torch.zeros(int(caps.sum()) + 64, dtype=torch.uint8).pin_memory()
    dlen, rc = torch.zeros(n, dtype=torch.int32).pin_memory(), torch.full((n,), 7, dtype=torch.int32).pin_memory()
    ctx.compress_pinned(src, pin(soff, np.int64), pin(lens, np.int32), dst, pin(doff, np.int64), pin(caps, np.int32),
                        dlen, rc, int(lens.max()), 7)
    assert (rc.numpy() == 0).all()
    raw = dst.numpy().tobytes()
    assert [raw[int(doff[k]):int(doff[k]) + int(dlen[k])] for k in range(n)] == want
    # store
    st = pmc_codec.Store(ctx, 16 << 20)
    ext, src_rc = st.put(vals)
    assert src_rc == [0] * n
    assert st.members(ext, n) == want
    assert st.get(ext, n) == [(0, v) for v in vals]
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
    dst, doff_t, dcap = D.slots_for([len(v) for v in vals])
    dlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    grc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    slab.get(slots, dst, doff_t, dcap, dlen, grc, D.stream_handle())
    torch.cuda.synchronize()
    assert int((grc != 0).sum()) == 0
    assert D.Batch(dst, doff_t, dlen, n, 0).host_items() == vals
    slab.close()
    # a group of two contexts on device 0
    g = ctypes.c_void_p()
    assert L.pmc_group_create((ctypes.c_int * 2)(0, 0), 2, ctypes.byref(g)) == 0
    try:
        assert L.pmc_group_set_level(g, 5) == pmc_codec.E_ARG
        assert L.pmc_group_set_level(g, pmc_codec.LEVEL_FAST) == 0
        kh = np.array([L.pmc_key_hash(b"key%d" % i, len(b"key%d" % i)) for i in range(n)], dtype=np.uint64)
        u_soff, u_len, u_cap, u_doff = (soff.astype(np.uint64), lens.astype(np.uint32), caps.astype(np.uint32),
                                        doff.astype(np.uint64))
        out = ctypes.create_string_buffer(int(caps.sum()) + 64)
        glen, grc2 = np.zeros(n, dtype=np.uint32), np.full(n, 7, dtype=np.int32)
        assert L.pmc_group_compress_batch(g, b"".join(vals), u_soff.ctypes.data, u_len.ctypes.data, kh.ctypes.data, 128,
                                          n, out, u_doff.ctypes.data, u_cap.ctypes.data, glen.ctypes.data,
                                          grc2.ctypes.data, int(lens.max())) == 0
        assert (grc2 == 0).all()
        assert [out.raw[int(doff[k]):int(doff[k]) + int(glen[k])] for k in range(n)] == want
    finally:
        L.pmc_group_destroy(g)


def test_own_decompress_takes_fast_members(ctx, edge, edge_members):
    import torch
    from pmc_codec import device as D
    for lo, hi in ((0, 4096), (4096, 16382)):  # the record kernel's members, the lane kernel's
        idx = [i for i, (_, v) in enumerate(edge) if lo < len(v) <= hi]
        assert len(idx) >= 10
        back, rc = D.decompress(ctx, D.pack([edge_members[i] for i in idx]), [len(edge[i][1]) for i in idx])
        torch.cuda.synchronize()
        assert int((rc != 0).sum()) == 0
        assert back.host_items() == [edge[i][1] for i in idx]


def test_exact_level_is_untouched(ctx, golden, edge_members):
    import pmc_codec
    # values above 16382 B take the exact paths at the fast level too
    big = [json_slices(golden.corpus, 16383, 1, 3)[0], json_slices(golden.corpus, 40000, 1, 4)[0]]
    fast_big = device_compress(ctx, big + [big[0][:1000]])
    assert fast_big[2][8] == 4
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        pairs = [(r, g) for r, g in golden.pairs() if r][:100]
        got = device_compress(ctx, [r for r, _ in pairs])
        assert got == [g for _, g in pairs]
        assert all(m[8] == 2 for m in got)
        exact_big = device_compress(ctx, big)
        assert fast_big[:2] == exact_big and all(m[8] == 2 for m in exact_big)
        assert [zlib.decompress(m, 31) for m in exact_big] == big
        with pytest.raises(ValueError):
            ctx.level = 6
        assert ctx.level == pmc_codec.LEVEL_EXACT
    finally:
        ctx.level = pmc_codec.LEVEL_FAST


def test_total_size_is_at_most_zlib_level_1(ctx, golden):
    """The ratio condition: on both baseline sets the fast members sum to at most zlib level 1's total."""
    with open(os.path.join(GOLDEN, "fast_baseline.json")) as f:
        base = json.load(f)["sets"]
    for name, (size, count) in BASELINE_SETS.items():
        b = base[name]
        assert (b["size"], b["count"]) == (size, count)
        vals = json_slices(golden.corpus, size, count, b["seed"])
        mem = device_compress(ctx, vals)
        total = sum(map(len, mem))
        print(f"fast {name}: {total} B, level 1 {b['level1_total']} ({total / b['level1_total']:.4f}), "
              f"level 9 {b['level9_total']} ({total / b['level9_total']:.4f})")
        assert [zlib.decompress(m, 31) for m in mem[::17]] == vals[::17]
        assert total <= b["level1_total"], (name, total, b["level1_total"])

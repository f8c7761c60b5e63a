"""GPU: the host-memory entries where their bookkeeping meets -- a pinned call whose chunks alternate between the
tiled and the compacted way back (the slot of a busy chunk grows, the bounce buffer grows while it still holds an
earlier chunk's outputs), and pmc_gzip_*_batch_host with slots the caller scattered, on both of its routes.
Every test makes its own context, so the pinned pipe's slots and bounce buffers start empty."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xEE
E_CAPACITY = -101


def corpus_values(golden, lens):
    """values of these lengths cut from the JSON corpus, each from a place of its own"""
    c = golden.corpus
    starts = [(7919 * k) % (len(c) - int(n)) for k, n in enumerate(lens)]
    return [c[s:s + int(n)] for s, n in zip(starts, lens)]


def mixed_slots(caps, chunk, rng, base=7):
    """Slot offsets for chunks of `chunk` values: an even chunk's slots tile one range in index order, an odd
    chunk's lie in permuted order with 0..9 bytes between them; 13 bytes between the chunks' ranges.  Returns the
    offsets, each chunk's (begin, end, tiled) and the buffer size."""
    caps = np.asarray(caps, dtype=np.int64)
    off, ranges, at = np.zeros(len(caps), dtype=np.int64), [], base
    for c, a in enumerate(range(0, len(caps), chunk)):
        idx = np.arange(a, min(a + chunk, len(caps)))
        tiled = c % 2 == 0
        begin = at
        order = idx if tiled else rng.permutation(idx)
        for i in order:
            if not tiled:
                at += int(rng.integers(0, 10))
            off[i] = at
            at += int(caps[i])
        ranges.append((begin, at, tiled))
        at += 13
    return off, ranges, at + 64


def untouched_mask(size, off, written, chunk, ranges):
    """True where a pinned call must leave dst alone: everything but the tiled chunks' ranges (copied back whole)
    and, in the other chunks, [off, off + written) of every value"""
    mask = np.ones(size, dtype=bool)
    for c, (begin, end, tiled) in enumerate(ranges):
        if tiled:
            mask[begin:end] = False
        else:
            for i in range(c * chunk, min((c + 1) * chunk, len(off))):
                mask[off[i]:off[i] + written[i]] = False
    return mask


def test_pinned_mixed_chunks(golden):
    """32 values in chunks of 8, slot mode: chunk 0 tiled (values of 1..200 bytes), chunk 1 permuted slots with
    gaps, chunk 2 tiled (3,000..5,000 bytes: slot 0 grows while chunk 0 may still be using it), chunk 3 permuted
    with gaps (the bounce buffer grows, after chunk 1's outputs have left it).  One value of chunk 1 and one of
    chunk 2 have 8 bytes of capacity.  Then the good members back through decompress_pinned, read where the
    compress call put them, into the same mix of layouts."""
    import torch
    import pmc_codec
    from oracle import pyoracle as O
    n, chunk = 32, 8
    rng = np.random.default_rng(20)
    lens = np.concatenate([rng.integers(1, 201, 16), rng.integers(3000, 5001, 16)])
    lens[[0, 8]], lens[[7, 15]], lens[[16, 24]], lens[[23, 31]] = 1, 200, 3000, 5000
    values = corpus_values(golden, lens)
    members = [O.compress(v) for v in values]
    short = [11, 19]
    caps = pmc_codec.gzip_bounds(lens.astype(np.uint32)).astype(np.int64)
    caps[short] = 8
    good = np.ones(n, dtype=bool)
    good[short] = False
    need = np.array([len(m) for m in members], dtype=np.int64)
    # the bounce buffer (4 KiB at least) holds chunk 1's outputs and must grow for chunk 3's
    assert need[8:16][good[8:16]].sum() + 64 <= 4096 < need[24:32].sum() + 64

    pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
    gaps = rng.integers(0, 5, n)
    soff = np.cumsum(np.concatenate([[3], (lens + gaps)[:-1]]))
    src = torch.zeros(int(soff[-1] + lens[-1] + 64), dtype=torch.uint8).pin_memory()
    for k, v in enumerate(values):
        src[int(soff[k]):int(soff[k]) + len(v)] = torch.frombuffer(bytearray(v), dtype=torch.uint8)
    doff, ranges, size = mixed_slots(caps, chunk, rng)
    assert [t for _, _, t in ranges] == [True, False, True, False]
    dst = torch.full((size,), FILL, dtype=torch.uint8).pin_memory()
    dlen = torch.full((n,), 12345, dtype=torch.int32).pin_memory()
    rc = torch.full((n,), 7, dtype=torch.int32).pin_memory()
    ctx = pmc_codec.Context(0)
    try:
        ctx.compress_pinned(src, pin(soff, np.int64), pin(lens, np.int32), dst, pin(doff, np.int64), pin(caps, np.int32),
                            dlen, rc, int(lens.max()), chunk)
    finally:
        ctx.close()
    rcn, dl, out = rc.numpy(), dlen.numpy().astype(np.int64), dst.numpy()
    assert (rcn[good] == 0).all() and (rcn[~good] == E_CAPACITY).all() and (dl[~good] == 0).all(), (rcn, dl)
    bad = [k for k in np.flatnonzero(good) if dl[k] != need[k] or out[doff[k]:doff[k] + need[k]].tobytes() != members[k]]
    assert not bad, bad
    changed = np.flatnonzero(untouched_mask(size, doff, dl, chunk, ranges) & (out != FILL))
    assert changed.size == 0, changed[:10]

    # the good members, read where they lie in the compress call's dst
    pick = np.flatnonzero(good)
    m = len(pick)
    vcap = lens[pick]
    voff, vranges, vsize = mixed_slots(vcap, chunk, rng)
    assert [t for _, _, t in vranges] == [True, False, True, False]
    back = torch.full((vsize,), FILL, dtype=torch.uint8).pin_memory()
    vlen = torch.full((m,), 12345, dtype=torch.int32).pin_memory()
    vrc = torch.full((m,), 7, dtype=torch.int32).pin_memory()
    ctx = pmc_codec.Context(0)
    try:
        ctx.decompress_pinned(dst, pin(doff[pick], np.int64), pin(need[pick], np.int32), back, pin(voff, np.int64),
                              pin(vcap, np.int32), vlen, vrc, int(vcap.max()), chunk)
    finally:
        ctx.close()
    vr, vl, got = vrc.numpy(), vlen.numpy().astype(np.int64), back.numpy()
    assert (vr == 0).all() and (vl == vcap).all(), (vr, vl)
    bad = [int(i) for k, i in enumerate(pick) if got[voff[k]:voff[k] + vcap[k]].tobytes() != values[i]]
    assert not bad, bad
    changed = np.flatnonzero(untouched_mask(vsize, voff, vl, chunk, vranges) & (got != FILL))
    assert changed.size == 0, changed[:10]


@pytest.mark.parametrize("route", ["latency", "pipeline"])
def test_host_entry_scattered_slots(golden, route):
    """pmc_gzip_compress_batch_host, then pmc_gzip_decompress_batch_host, dst_off given: permuted slots with gaps.
    Eight values of at most 4,096 bytes take the latency route; with one of 50,000 bytes (above the compress
    route's 4,096 and the decompress route's 49,152) both calls take the pipeline."""
    import pmc_codec
    from oracle import pyoracle as O
    L = pmc_codec.lib()
    rng = np.random.default_rng(8)
    lens = np.array([1, 4096, 17, 1500, 4095, 300, 2048, 777], dtype=np.int64)
    if route == "pipeline":
        lens[3] = 50000
    n = len(lens)
    values = corpus_values(golden, lens)
    members = [O.compress(v) for v in values]
    need = np.array([len(m) for m in members], dtype=np.int64)

    def scattered(caps):
        perm = rng.permutation(n)
        g = rng.integers(0, 10, n)
        pos = np.cumsum(np.concatenate([[7], (caps[perm] + g[perm])[:-1]]))
        off = np.empty(n, dtype=np.int64)
        off[perm] = pos
        return off, int(pos[-1] + caps[perm[-1]] + 16)

    def call(ctx, fn, counter, src, soff, slen, caps):
        """the call into slots scattered() lays out; returns offsets, lengths and the buffer, after checking the
        verdicts, the route counter and the bytes outside the outputs"""
        off, size = scattered(caps)
        dst = np.full(size, FILL, dtype=np.uint8)
        dlen = np.full(n, 12345, dtype=np.uint32)
        rc = np.full(n, 7, dtype=np.int32)
        so, sl, do, dc = soff.astype(np.uint64), slen.astype(np.uint32), off.astype(np.uint64), caps.astype(np.uint32)
        before = ctx.path_counts()
        r = fn(ctx.handle, src.ctypes.data, so.ctypes.data, sl.ctypes.data, n, dst.ctypes.data, do.ctypes.data,
               dc.ctypes.data, dlen.ctypes.data, rc.ctypes.data)
        assert r == 0, pmc_codec.last_error()
        after = ctx.path_counts()
        assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {counter: 1}
        assert (rc == 0).all(), rc
        dl = dlen.astype(np.int64)
        mask = np.ones(size, dtype=bool)
        for k in range(n):
            mask[off[k]:off[k] + dl[k]] = False
        changed = np.flatnonzero(mask & (dst != FILL))
        assert changed.size == 0, changed[:10]
        return off, dl, dst

    gaps = rng.integers(0, 5, n)
    soff = np.cumsum(np.concatenate([[3], (lens + gaps)[:-1]]))
    src = np.zeros(int(soff[-1] + lens[-1] + 64), dtype=np.uint8)
    for k, v in enumerate(values):
        src[soff[k]:soff[k] + len(v)] = np.frombuffer(v, dtype=np.uint8)
    ctx = pmc_codec.Context(0)
    try:
        caps = pmc_codec.gzip_bounds(lens.astype(np.uint32)).astype(np.int64)
        moff, mlen, mem = call(ctx, L.pmc_gzip_compress_batch_host, route + "_compress", src, soff, lens, caps)
        assert (mlen == need).all(), (mlen, need)
        assert [mem[moff[k]:moff[k] + need[k]].tobytes() for k in range(n)] == members
        # the members, read where the compress call put them; capacities: the values' lengths
        voff, vlen, back = call(ctx, L.pmc_gzip_decompress_batch_host, route + "_decompress", mem, moff, mlen, lens)
        assert (vlen == lens).all(), (vlen, lens)
        assert [back[voff[k]:voff[k] + lens[k]].tobytes() for k in range(n)] == values
    finally:
        ctx.close()

"""GPU: the edges of a group batch (pmc_group_*, csrc/pmc_group.hip), members 2 and 3 on device 0.

A group gathers each member's share into pinned memory, runs the pinned call (compress: packed mode, where a
failed value takes no bytes) and scatters the successful outputs to the caller's dst_off.  Here values fail in
the middle of a share, a share is empty, a share is large enough for the threaded gather and scatter (more than
16,384 values per host thread), and a batch is empty.  Expected bytes are the goldens, the oracle's members and
the source values; verdicts of damaged members are the oracle's."""
import contextlib
import ctypes
import hashlib

import numpy as np
import pytest

import store_model as M

pytestmark = pytest.mark.gpu

GUARD = 0xA5
E_CAPACITY = -101
SHARDS = 128


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def group_of(members):
    import torch  # noqa: F401
    import pmc_codec
    L = pmc_codec.lib()
    g = ctypes.c_void_p()
    assert L.pmc_group_create((ctypes.c_int * members)(*([0] * members)), members, ctypes.byref(g)) == 0
    try:
        yield g
    finally:
        L.pmc_group_destroy(g)


def packed(items):
    lens = np.array([len(x) for x in items], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return b"".join(items), off, lens


def gapped_slots(caps, seed):
    """Permuted slots with 3 bytes between them -> offsets, total size."""
    caps = np.asarray(caps, dtype=np.uint64)
    perm = np.random.default_rng(seed).permutation(len(caps))
    off = np.zeros(len(caps), dtype=np.uint64)
    off[perm] = 5 + np.concatenate([[0], np.cumsum(caps[perm][:-1] + np.uint64(3))]).astype(np.uint64)
    return off, int(off.max() + caps.max()) + 64


def call(g, compress, items, kh, caps, off, total, max_len):
    """One group call into a 0xA5-filled destination -> rc, dst_len, destination after the call."""
    import pmc_codec
    L = pmc_codec.lib()
    src, soff, slen = packed(items)
    n = len(items)
    dst = np.full(total, GUARD, dtype=np.uint8)
    cap32 = np.asarray(caps, dtype=np.uint32)
    off = np.asarray(off, dtype=np.uint64)
    kh = np.asarray(kh, dtype=np.uint64)
    dlen = np.full(n, 12345, dtype=np.uint32)
    rc = np.full(n, 7, dtype=np.int32)
    fn = L.pmc_group_compress_batch if compress else L.pmc_group_decompress_batch
    r = fn(g, src, soff.ctypes.data, slen.ctypes.data, kh.ctypes.data, SHARDS, n, dst.ctypes.data, off.ctypes.data,
           cap32.ctypes.data, dlen.ctypes.data, rc.ctypes.data, max_len)
    assert r == 0, (r, pmc_codec.last_error())
    return rc, dlen.astype(np.int64), dst


def check(tag, want, caps, off, rc, dlen, out):
    """want[i]: (0, bytes) or (a failure's rc, None).  Verdicts, lengths and bytes, a failed compress value's
    dst_len 0, and no byte outside the successful outputs changed."""
    bad = []
    untouched = np.ones(len(out), dtype=bool)
    for i, (wrc, wbytes) in enumerate(want):
        o = int(off[i])
        if wrc == 0:
            if rc[i] != 0 or dlen[i] != len(wbytes) or out[o:o + len(wbytes)].tobytes() != wbytes:
                bad.append((i, "cap", int(caps[i]), "want", len(wbytes), "rc", int(rc[i]), "dst_len", int(dlen[i])))
            untouched[o:o + len(wbytes)] = False
        elif rc[i] != wrc or (tag[0] == "compress" and dlen[i] != 0):
            bad.append((i, "cap", int(caps[i]), "want rc", wrc, "rc", int(rc[i]), "dst_len", int(dlen[i])))
    assert not bad, (tag, len(bad), bad[:8])
    changed = np.flatnonzero(untouched & (out != GUARD))
    assert len(changed) == 0, (tag, len(changed), "bytes outside the successful outputs changed, first at", int(changed[0]))


@pytest.fixture(scope="module")
def mixed(golden):
    """Golden pairs up to 16,382 bytes and four values of 40,000 to 70,001 bytes with the oracle's members."""
    pairs = [(r, g) for r, g in golden.pairs() if 0 < len(r) <= 16382][:330]
    corpus = golden.corpus
    for n, o in ((40000, 11), (50001, 2000), (65536, 7001), (70001, 12000)):
        v = corpus[o:o + n]
        pairs.insert(37 * (n % 7) + 5, (v, M.member_of(v)))
    return pairs


@pytest.mark.parametrize("members", [2, 3])
def test_group_failed_values_in_the_middle(ctx, mixed, members):
    import pmc_codec
    from oracle import pyoracle as O
    vals, gz = [r for r, _ in mixed], [g for _, g in mixed]
    n = len(vals)
    kh = np.random.default_rng(members).integers(0, 1 << 62, n).astype(np.uint64)
    route = (kh % np.uint64(SHARDS)) % np.uint64(members)
    assert len(set(route.tolist())) == members
    max_len = max(map(len, vals))
    with group_of(members) as g:
        # compress: the capacity cycle of tests/test_gpu_compress_bounds.py
        need = np.array([len(m) for m in gz], dtype=np.int64)
        bound = pmc_codec.gzip_bounds([len(v) for v in vals]).astype(np.int64)
        for turn in (0, 1):
            caps = np.array([(need[i], need[i] - 1, need[i] + 1, 0, min(need[i] - 1, 17), bound[i])[(i + 3 * turn) % 6]
                             for i in range(n)], dtype=np.int64)
            assert 3 * int((caps < need).sum()) >= n and 3 * int((caps >= need).sum()) >= n
            off, total = gapped_slots(caps, 10 + turn)
            rc, dlen, out = call(g, True, vals, kh, caps, off, total, max_len)
            want = [(0, gz[i]) if caps[i] >= need[i] else (E_CAPACITY, None) for i in range(n)]
            check(("compress", members, turn), want, caps, off, rc, dlen, out)
        # decompress: capacities around raw_len, and one damaged member in every share
        raw = np.array([len(v) for v in vals], dtype=np.int64)
        src = list(gz)
        for k in range(members):
            i = [int(j) for j in np.flatnonzero(route == k) if j % 6 in (0, 2)][3 + k]
            d = bytearray(src[i])
            d[len(d) - 7] ^= 0x20  # CRC-32 trailer
            src[i] = bytes(d)
        for turn in (0, 1):
            caps = np.array([(raw[i], raw[i] - 1, raw[i] + 1, 0, min(raw[i] - 1, 17), raw[i] + 64)[(i + 3 * turn) % 6]
                             for i in range(n)], dtype=np.int64)
            off, total = gapped_slots(caps, 20 + turn)
            rc, dlen, out = call(g, False, src, kh, caps, off, total, max_len)
            want = []
            for i in range(n):
                erc, eout = O.decompress(src[i], cap=int(caps[i]), grow=False)
                want.append((0, eout) if erc == 0 else (erc, None))
            verdicts = [w[0] for w in want]
            if turn == 0:  # (the damaged members' capacities suffice in this turn)
                assert verdicts.count(pmc_codec.Z_DATA_ERROR) == members
            assert 3 * verdicts.count(E_CAPACITY) >= n and 3 * verdicts.count(0) >= n
            check(("decompress", members, turn), want, caps, off, rc, dlen, out)


@pytest.mark.parametrize("members", [2, 3])
def test_group_empty_share(ctx, golden, members):
    """Every key routed to member 0: members 1 and up get nothing.  Then a batch that reaches all of them."""
    import pmc_codec
    pairs = [(r, g) for r, g in golden.pairs() if 0 < len(r) <= 16382][40:240]
    vals, gz = [r for r, _ in pairs], [g for _, g in pairs]
    n = len(vals)
    rng = np.random.default_rng(members)
    lone = (rng.integers(0, 1 << 40, n) * SHARDS + members * rng.integers(0, SHARDS // members, n)).astype(np.uint64)
    assert (((lone % np.uint64(SHARDS)) % np.uint64(members)) == 0).all()
    spread = rng.integers(0, 1 << 62, n).astype(np.uint64)
    assert len(set(((spread % np.uint64(SHARDS)) % np.uint64(members)).tolist())) == members
    bound = pmc_codec.gzip_bounds([len(v) for v in vals]).astype(np.int64)
    raw = np.array([len(v) for v in vals], dtype=np.int64)
    with group_of(members) as g:
        for tag, kh in (("lone", lone), ("spread", spread), ("lone again", lone)):
            off, total = gapped_slots(bound, 3)
            rc, dlen, out = call(g, True, vals, kh, bound, off, total, int(raw.max()))
            check(("compress", members, tag), [(0, m) for m in gz], bound, off, rc, dlen, out)
            off, total = gapped_slots(raw, 4)
            rc, dlen, out = call(g, False, gz, kh, raw, off, total, int(raw.max()))
            check(("decompress", members, tag), [(0, v) for v in vals], raw, off, rc, dlen, out)


@pytest.mark.parametrize("members", [2, 3])
def test_group_threaded_gather_scatter(ctx, golden, members):
    """40,000 values of 64 to 200 bytes per member: the gather and the scatter of every share run on several
    host threads (one per 16,384 values).  Members against the oracle's by a seeded sample of 1,000 and the
    SHA-256 over all; decompress returns the source."""
    import pmc_codec
    from oracle import pyoracle as O
    n = 40000 * members
    rows = O.gen_values(golden.corpus, 0x6A7E + members, 0, 0, n, 200)
    lens = 64 + (np.arange(n, dtype=np.int64) * 61) % 137
    assert lens.min() == 64 and lens.max() == 200
    vals = [rows[i, :lens[i]].tobytes() for i in range(n)]
    gz = [O.compress(v) for v in vals]
    kh = np.arange(n, dtype=np.uint64)
    share = np.bincount(((kh % np.uint64(SHARDS)) % np.uint64(members)).astype(np.int64), minlength=members)
    assert share.min() > 2 * 16384, share
    bound = pmc_codec.gzip_bounds(lens).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum(bound)[:-1]])
    roff = np.concatenate([[0], np.cumsum(lens)[:-1]])
    with group_of(members) as g:
        rc, dlen, out = call(g, True, vals, kh, bound, boff, int(bound.sum()) + 64, 200)
        assert (rc == 0).all() and (dlen == np.array([len(m) for m in gz])).all(), np.flatnonzero(rc != 0)[:8]
        got = [out[o:o + m].tobytes() for o, m in zip(boff.tolist(), dlen.tolist())]
        pick = np.random.default_rng(9).choice(n, 1000, replace=False).tolist()
        bad = [i for i in pick if got[i] != gz[i]]
        assert not bad, (len(bad), bad[:8])
        assert hashlib.sha256(b"".join(got)).hexdigest() == hashlib.sha256(b"".join(gz)).hexdigest()
        rc, dlen, out = call(g, False, gz, kh, lens, roff, int(lens.sum()) + 64, 200)
        assert (rc == 0).all() and (dlen == lens).all(), np.flatnonzero(rc != 0)[:8]
        assert out[:int(lens.sum())].tobytes() == b"".join(vals)
        assert (out[int(lens.sum()):] == GUARD).all()


@pytest.mark.parametrize("members", [2, 3])
def test_group_empty_batch(ctx, members):
    """n == 0 returns PMC_OK and touches nothing, whatever the pointers."""
    import pmc_codec
    L = pmc_codec.lib()
    dst = np.full(256, GUARD, dtype=np.uint8)
    arr = np.full(4, 0x7777, dtype=np.uint64)
    dlen = np.full(4, 12345, dtype=np.uint32)
    rc = np.full(4, 7, dtype=np.int32)
    with group_of(members) as g:
        for fn in (L.pmc_group_compress_batch, L.pmc_group_decompress_batch):
            assert fn(g, b"x", arr.ctypes.data, dlen.ctypes.data, arr.ctypes.data, SHARDS, 0, dst.ctypes.data,
                      arr.ctypes.data, dlen.ctypes.data, dlen.ctypes.data, rc.ctypes.data, 64) == 0
            assert fn(g, None, None, None, None, SHARDS, 0, None, None, None, None, None, 0) == 0
        assert (dst == GUARD).all() and (arr == 0x7777).all() and (dlen == 12345).all() and (rc == 7).all()

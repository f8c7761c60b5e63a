"""GPU: same-direction calls of one context on two streams, with no host synchronisation between them.

include/pmc_codec.h: scratch is per context and per direction, and the library orders two compress calls (or two
decompress calls, two slab sets, two slab gets) that are issued on different streams -- the later one waits on
the device for the earlier one (dir_enter / dir_leave in csrc/pmc_capi.hip).  Every other test passes one stream,
so that wait is executed only here.

What a test can and cannot show: a missing wait corrupts results only if the later call's kernels really run
while the earlier call still uses the scratch, which is a matter of timing.  The shapes are chosen to make that
likely -- A (32,768 values) is still running when B's kernels are enqueued, and B, C and D lay the same scratch
out in other ways -- but a pass proves the ordering only with some probability, whatever a test does.  The
context is warmed with every shape first: a call that grew scratch would free the old buffer, which
synchronises the device and would hide a missing wait.

Expected bytes are the oracle's members, computed once for the module."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SEED = 0x5712EA


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


class Shape:
    """One batch: values (host), the oracle's members, and the device tensors of a compress and a decompress
    call on it."""

    def __init__(self, name, rows, lens):
        import torch
        import pmc_codec
        from oracle import pyoracle as O
        self.name, self.n, self.vlen = name, len(rows), rows.shape[1]
        self.lens = np.asarray(lens, dtype=np.int64)
        self.rows = rows
        self.values = [rows[i, :self.lens[i]].tobytes() for i in range(self.n)]
        self.members = [O.compress(v) for v in self.values]
        self.mlens = np.array([len(m) for m in self.members], dtype=np.int64)
        self.max_len = int(self.lens.max())
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
        # compress: values where the generator put them (row i at i * vlen), members into bound-sized slots
        self.src = torch.from_numpy(rows.reshape(-1)).cuda()
        self.soff = dev(np.arange(self.n, dtype=np.int64) * self.vlen, np.int64)
        self.slen = dev(self.lens, np.int32)
        caps = pmc_codec.gzip_bounds(self.lens).astype(np.int64)
        self.coff = np.concatenate([[0], np.cumsum((caps + 3) & ~3)[:-1]])
        self.c_dst = torch.empty(int(self.coff[-1] + caps[-1]) + 64, dtype=torch.uint8, device="cuda")
        self.c_off, self.c_cap = dev(self.coff, np.int64), dev(caps, np.int32)
        self.c_len = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.c_rc = torch.empty(self.n, dtype=torch.int32, device="cuda")
        # decompress: the oracle's members back to back, values into slots of exactly their size
        self.moff = np.concatenate([[0], np.cumsum(self.mlens)[:-1]])
        self.m_src = torch.from_numpy(np.frombuffer(b"".join(self.members) + bytes(16), dtype=np.uint8).copy()).cuda()
        self.m_off, self.m_len = dev(self.moff, np.int64), dev(self.mlens, np.int32)
        self.doff = np.concatenate([[0], np.cumsum((self.lens + 3) & ~3)[:-1]])
        self.d_dst = torch.empty(int(self.doff[-1] + self.lens[-1]) + 64, dtype=torch.uint8, device="cuda")
        self.d_off, self.d_cap = dev(self.doff, np.int64), dev(self.lens, np.int32)
        self.d_len = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.d_rc = torch.empty(self.n, dtype=torch.int32, device="cuda")

    def prefill(self):
        for t, v in ((self.c_dst, GUARD), (self.d_dst, GUARD), (self.c_len, 12345), (self.d_len, 12345), (self.c_rc, 7),
                     (self.d_rc, 7)):
            t.fill_(v)

    def compress(self, ctx, stream):
        ctx.compress_device(self.src, self.soff, self.slen, self.c_dst, self.c_off, self.c_cap, self.c_len, self.c_rc,
                            self.max_len, stream)

    def decompress(self, ctx, stream):
        ctx.decompress_device(self.m_src, self.m_off, self.m_len, self.d_dst, self.d_off, self.d_cap, self.d_len,
                              self.d_rc, self.max_len, stream)

    def check_members(self, sample=None):
        """The compress call's outputs against the oracle's: verdicts and lengths of all; bytes of all, or of a
        seeded sample with the SHA-256 of the rest."""
        rc, dlen, out = self.c_rc.cpu().numpy(), self.c_len.cpu().numpy().astype(np.int64), self.c_dst.cpu().numpy()
        assert (rc == 0).all(), (self.name, np.flatnonzero(rc != 0)[:8], rc[rc != 0][:8])
        assert (dlen == self.mlens).all(), (self.name, np.flatnonzero(dlen != self.mlens)[:8])
        got = [out[o:o + n].tobytes() for o, n in zip(self.coff.tolist(), dlen.tolist())]
        pick = range(self.n) if sample is None else sorted(np.random.default_rng(SEED).choice(self.n, sample, replace=False).tolist())
        bad = [i for i in pick if got[i] != self.members[i]]
        assert not bad, (self.name, len(bad), bad[:8])
        if sample is not None:
            rest = sorted(set(range(self.n)) - set(pick))
            sha = lambda ms: hashlib.sha256(b"".join(ms[i] for i in rest)).hexdigest()  # noqa: E731
            assert sha(got) == sha(self.members), (self.name, "the members outside the sample differ")

    def check_values(self):
        rc, dlen, out = self.d_rc.cpu().numpy(), self.d_len.cpu().numpy().astype(np.int64), self.d_dst.cpu().numpy()
        assert (rc == 0).all(), (self.name, np.flatnonzero(rc != 0)[:8], rc[rc != 0][:8])
        assert (dlen == self.lens).all(), (self.name, np.flatnonzero(dlen != self.lens)[:8])
        bad = [i for i, (o, n) in enumerate(zip(self.doff.tolist(), dlen.tolist())) if out[o:o + n].tobytes() != self.values[i]]
        assert not bad, (self.name, len(bad), bad[:8])


@pytest.fixture(scope="module")
def shapes(golden):
    from oracle import pyoracle as O
    corpus = golden.corpus
    a = O.gen_values(corpus, SEED, 0, 0, 32768, 1024)
    b = O.gen_values(corpus, SEED, 0, 100000, 300, 256)
    c = O.gen_values(corpus, SEED, 0, 200000, 2000, 4096)
    d = O.gen_values(corpus, SEED, 0, 300000, 40, 40000)
    return {"A": Shape("A", a, [1024] * 32768), "B": Shape("B", b, [256] * 300),
            "C": Shape("C", c, [3073 + (37 * i) % 1024 for i in range(2000)]), "D": Shape("D", d, [40000] * 40)}


def test_compress_calls_on_two_streams(ctx, shapes):
    """A on s1, B on s2, C on s1, D on s2, one synchronisation after D: every member is the oracle's."""
    import torch
    A, B, C, D = (shapes[k] for k in "ABCD")
    for s in (A, B, C, D):  # warm: the scratch of every shape exists before the sequence
        s.compress(ctx, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s in (A, B, C, D):
        s.prefill()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    A.compress(ctx, s1.cuda_stream)
    B.compress(ctx, s2.cuda_stream)
    C.compress(ctx, s1.cuda_stream)
    D.compress(ctx, s2.cuda_stream)
    torch.cuda.synchronize()
    B.check_members()
    C.check_members()
    D.check_members()
    A.check_members(sample=2000)


def test_decompress_calls_on_two_streams(ctx, shapes):
    """The same four batches back in the order B, A, D, C on alternating streams."""
    import torch
    A, B, C, D = (shapes[k] for k in "ABCD")
    for s in (A, B, C, D):
        s.decompress(ctx, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s in (A, B, C, D):
        s.prefill()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    B.decompress(ctx, s1.cuda_stream)
    A.decompress(ctx, s2.cuda_stream)
    D.decompress(ctx, s1.cuda_stream)
    C.decompress(ctx, s2.cuda_stream)
    torch.cuda.synchronize()
    for s in (B, A, D, C):
        s.check_values()


def _d2h(ptr, nbytes):
    """Copy nbytes of device memory at ptr into host bytes (HIP runtime through ctypes)."""
    hip = ctypes.CDLL("libamdhip64.so")
    buf = ctypes.create_string_buffer(nbytes)
    assert hip.hipMemcpy(buf, ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return buf.raw


def test_slab_sets_and_gets_on_two_streams(ctx, shapes):
    """Two sets with disjoint slots on s1 and s2 back to back, then two gets on s2 and s1; each get is ordered
    after its set by an event of the caller's, as the header asks.  All values come back and the slab holds
    the oracle's members."""
    import torch
    import pmc_codec
    A = shapes["A"]
    K, h = 4096, 2000
    slab = pmc_codec.Slab(ctx, K, 1024)
    perm = np.random.default_rng(SEED).permutation(K).astype(np.int32)
    slots = [torch.from_numpy(perm[:h].copy()).cuda(), torch.from_numpy(perm[h:2 * h].copy()).cuda()]
    src = lambda first: (A.src[first * 1024:(first + h) * 1024 + 16], A.soff[:h], A.slen[:h])  # noqa: E731
    new = lambda fill, dt: torch.full((h,), fill, dtype=dt, device="cuda")  # noqa: E731
    doff = torch.arange(h, dtype=torch.int64, device="cuda") * 1028 + 1
    dcap = new(1024, torch.int32)
    # warm with other values of the same shape, so the slots hold other members before the sequence
    null = torch.cuda.current_stream().cuda_stream
    for k in (0, 1):
        slab.set(*src(4 * h), slots[k], new(7, torch.int32), null)
        slab.get(slots[k], torch.empty(h * 1028 + 64, dtype=torch.uint8, device="cuda"), doff, dcap, new(0, torch.int32),
                 new(7, torch.int32), null)
    torch.cuda.synchronize()
    src_rc = [new(7, torch.int32), new(7, torch.int32)]
    dst = [torch.full((h * 1028 + 64,), GUARD, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
    dlen, rc = [new(12345, torch.int32) for _ in (0, 1)], [new(7, torch.int32) for _ in (0, 1)]
    ins = [src(0), src(h)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    e1, e2 = torch.cuda.Event(), torch.cuda.Event()
    slab.set(*ins[0], slots[0], src_rc[0], s1.cuda_stream)
    slab.set(*ins[1], slots[1], src_rc[1], s2.cuda_stream)
    e1.record(s1)
    e2.record(s2)
    s2.wait_event(e1)
    slab.get(slots[0], dst[0], doff, dcap, dlen[0], rc[0], s2.cuda_stream)
    s1.wait_event(e2)
    slab.get(slots[1], dst[1], doff, dcap, dlen[1], rc[1], s1.cuda_stream)
    torch.cuda.synchronize()
    lens = np.frombuffer(_d2h(slab.lengths_ptr(), 4 * K), dtype=np.uint32)
    data = np.frombuffer(_d2h(slab.data_ptr(), slab.stride * K), dtype=np.uint8).reshape(K, slab.stride)
    for k in (0, 1):
        assert int((src_rc[k] != 0).sum()) == 0 and int((rc[k] != 0).sum()) == 0 and int((dlen[k] != 1024).sum()) == 0, k
        out = dst[k].cpu().numpy()
        assert (out[0] == GUARD) and (out[1:1 + h * 1028].reshape(h, 1028)[:, 1024:] == GUARD).all()
        assert (out[1:1 + h * 1028].reshape(h, 1028)[:, :1024] == A.rows[k * h:(k + 1) * h]).all(), k
        bad = [i for i in range(h) if lens[perm[k * h + i]] != A.mlens[k * h + i]
               or data[perm[k * h + i], :A.mlens[k * h + i]].tobytes() != A.members[k * h + i]]
        assert not bad, (k, len(bad), bad[:8])
    assert (lens[perm[2 * h:]] == 0).all()
    slab.close()

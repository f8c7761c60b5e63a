"""GPU: every inflate route against the oracle on members this project did not write.

The corpus is tests/foreign_members.py's (zlib's members at every level, strategy, memLevel and flush,
hand-assembled valid and invalid streams, mutations of both); tests/test_foreign_members.py holds the oracle
itself to zlib on the same corpus.  Each test below sends it down one route, chosen by batch size and max_len
alone (no environment switch), into slots at unaligned offsets with 1-7 guard bytes between them, and asserts
for every member the oracle's verdict and bytes at that capacity, and that no byte outside any member's
[dst_off, dst_off + dst_cap) changed, whatever its verdict.  A PMC_E_CAPACITY answer is followed by a second
call with the reported size, which must give the oracle's verdict.

Capacities: the exact output size for a member the oracle decodes, 0 and 1 for the empty value, the size its
author meant + 8 for the rest."""
import ctypes
import zlib

import numpy as np
import pytest

import foreign_members as F

pytestmark = pytest.mark.gpu

PIPELINE_N = 4200  # more members than the wave-kernel-only route of a device batch takes (4,096)
PAD_VALUE = b"padding " * 8
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


def oracle(member, cap):
    """(rc, bytes, decoded size) of the oracle at this capacity (no growing)."""
    from oracle import pyoracle as O
    out = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_size_t(0)
    rc = O.lib().oracle_gzip_decompress(member, len(member), out, cap, ctypes.byref(n))
    return rc, (out.raw[:n.value] if rc == 0 else b""), n.value


class Case:
    """One member at one capacity, and what the oracle says about it."""

    def __init__(self, name, member, cap):
        self.name, self.member, self.cap = name, member, cap
        self.rc, self.out, self.need = oracle(member, cap)

    def must_decline(self):
        """The record and lane kernels' own rules hand this member on: a verdict other than 0, header
        flags (lane_prepare), a stored first block (lane_block)."""
        m = self.member
        return self.rc != 0 or m[3] != 0 or (m[10] >> 1) & 3 == 0


def cases_of(entries, tail=b""):
    out = []
    for e in entries:
        m = e.member + tail
        rc, val, _ = oracle(m, 1 << 20)
        if rc == 0 and len(val) == 0:
            out += [Case(e.name + "@0", m, 0), Case(e.name + "@1", m, 1)]
        else:
            out.append(Case(e.name, m, len(val) if rc == 0 else e.size + 8))
    return out


@pytest.fixture(scope="module")
def cases(golden):
    """The whole corpus as cases, computed once and not changed by any test."""
    return cases_of(F.entries(golden.corpus))


def device_call(ctx, cases, max_len, pad_to=0, seed=1):
    """One device-resident call over `cases` (+ copies of one plain member up to pad_to): asserts the guard
    bytes and the padding, returns (rc, dst_len, [slot bytes])."""
    import torch
    from pmc_codec import device as D
    rng = np.random.default_rng(seed)
    n0 = len(cases)
    members = [c.member for c in cases]
    caps = [c.cap for c in cases]
    if pad_to > n0:
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        pad = c.compress(PAD_VALUE) + c.flush()
        members += [pad] * (pad_to - n0)
        caps += [len(PAD_VALUE)] * (pad_to - n0)
    n = len(members)
    caps = np.asarray(caps, dtype=np.int64)
    gaps = rng.integers(1, 8, n)
    off = np.zeros(n, dtype=np.int64)
    pos = 3
    for i in range(n):
        off[i] = pos
        pos += int(caps[i]) + int(gaps[i])
    host0 = np.full(pos + 16, GUARD, dtype=np.uint8)
    dst = torch.from_numpy(host0.copy()).cuda()
    doff = torch.from_numpy(off).cuda()
    dcap = torch.from_numpy(caps.astype(np.int32)).cuda()
    dlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    b = D.pack(members)
    ctx.decompress_device(b.data, b.off, b.len, dst, doff, dcap, dlen, rc, int(max_len), D.stream_handle())
    torch.cuda.synchronize()
    rc, dlen, out = rc.cpu().numpy(), dlen.cpu().numpy(), dst.cpu().numpy()
    outside = np.ones(len(out), dtype=bool)
    for i in range(n):
        outside[off[i]:off[i] + caps[i]] = False
    changed = np.flatnonzero(outside & (out != host0))
    if len(changed):
        k = int(np.searchsorted(off, changed[0], side="right")) - 1
        raise AssertionError(f"{len(changed)} bytes outside the slots changed, first at {int(changed[0])}: slot {k} "
                             f"({cases[k].name if k < n0 else 'padding'}) is [{int(off[k])}, {int(off[k] + caps[k])})")
    for i in range(n0, n):
        assert rc[i] == 0 and out[off[i]:off[i] + dlen[i]].tobytes() == PAD_VALUE, ("padding", i, int(rc[i]))
    return rc[:n0], dlen[:n0], [out[off[i]:off[i] + caps[i]] for i in range(n0)]


def check_route(ctx, cases, max_len, pad_to=0):
    """The call, the comparison with the oracle, and the second call for PMC_E_CAPACITY answers.  Returns the
    growth of the context's inflate_retry counter over the first call."""
    import pmc_codec
    before = ctx.guard_counts()["inflate_retry"]
    rc, dlen, slots = device_call(ctx, cases, max_len, pad_to)
    grew = ctx.guard_counts()["inflate_retry"] - before
    bad, again = [], []
    for k, c in enumerate(cases):
        if rc[k] != c.rc or (c.rc == 0 and (dlen[k] != len(c.out) or slots[k][:dlen[k]].tobytes() != c.out)):
            bad.append((c.name, c.cap, int(rc[k]), c.rc, int(dlen[k]), len(c.out)))
        elif c.rc == pmc_codec.E_CAPACITY:
            assert dlen[k] > c.cap, (c.name, int(dlen[k]), c.cap)
            again.append(Case(c.name + "@reported", c.member, int(dlen[k])))
    assert not bad, (len(bad), bad[:8])
    if again:
        assert all(c.rc != pmc_codec.E_CAPACITY for c in again), [c.name for c in again if c.rc == pmc_codec.E_CAPACITY]
        rc, dlen, slots = device_call(ctx, again, max(max_len, max(c.cap for c in again)), pad_to, seed=2)
        bad = [(c.name, c.cap, int(rc[k]), c.rc) for k, c in enumerate(again)
               if rc[k] != c.rc or (c.rc == 0 and slots[k][:dlen[k]].tobytes() != c.out)]
        assert not bad, (len(bad), bad[:8])
    return grew


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def pipeline_route(ctx, cases, max_len):
    """A batch of more than 4,096 members (padded): the record / lane kernels with the wave kernels behind.
    Returns the growth of the context's inflate_retry counter over the first call; asserts that it covers
    every member the fast paths must decline."""
    assert max_len == max(c.cap for c in cases)
    grew = check_route(ctx, cases, max_len, max(PIPELINE_N, len(cases) + 1))
    declined = sum(1 for c in cases if c.must_decline())
    print(f"max_len {max_len}: {len(cases)} members, {declined} the fast paths must decline, inflate_retry +{grew}")
    assert grew >= declined, (grew, declined)
    return grew


def test_wave_kernel_alone(ctx, cases):
    """A device call of at most 4 members per CU takes the wave kernels whatever its sizes
    (pmc_capi.hip:1305-1306, pmc_gzip_decompress_batch's `small`): the LDS decoder, and the general decoder
    for members past its image (48 KiB of output, or more input than gzip_bound of the image)."""
    step = 4 * cus()
    for a in range(0, len(cases), step):
        part = cases[a:a + step]
        check_route(ctx, part, max(c.cap for c in part))


def test_general_decoder_on_small_members(ctx, golden):
    """Members of <= 256 output bytes, each followed by 1 KiB of arbitrary bytes, in calls of at most 4
    members per CU with max_len their largest capacity: the LDS decoder's input limit is gzip_bound(image) + 64
    (pmc_capi.hip:1196-1199), every member is longer, so the general (HBM) decoder takes it
    (pmc_capi.hip:1245-1249)."""
    tail = bytes(np.random.default_rng(77).integers(0, 256, 1024, dtype=np.uint8))
    small = [c for c in cases_of([e for e in F.entries(golden.corpus) if e.size <= 256], tail) if c.cap <= 264]
    max_len = max(c.cap for c in small)
    image = (max_len + 63) & ~63
    assert image + (image >> 3) + 6 + 32 + 64 < 1024  # (gzip_bound(image) + 64: below every member's length)
    step = 4 * cus()
    for a in range(0, len(small), step):
        check_route(ctx, small[a:a + step], max_len)


def test_record_kernel_1k_image(ctx, cases):
    """More than 4,096 members with max_len <= 1024: inflate_rec_kernel<1024> (pmc_plan.hpp
    InflatePlan::out1k), the lane passes for what it marks too large for its rows, the wave kernels for what both
    decline."""
    part = [c for c in cases if c.cap <= 1024]
    assert max(c.cap for c in part) == 1024
    pipeline_route(ctx, part, 1024)


def test_record_kernel_4k_image(ctx, cases):
    """More than 4,096 members with max_len = 4096: inflate_rec_kernel<4096> (pmc_plan.hpp InflatePlan::out1k is off)."""
    part = [c for c in cases if c.cap <= 4096]
    assert max(c.cap for c in part) == 4096
    pipeline_route(ctx, part, 4096)


def test_lane_passes_without_the_multiblock_pass(ctx, cases):
    """max_len in 4097..16383 leaves multi_pass off (pmc_capi.hip:1170): members above the record kernel's
    4 KiB go to inflate_lane_kernel<96,false> and <128,false>, and every member of several blocks, the small
    memLevel-1 and flush members among them, must come back through the wave kernels' retry."""
    part = [c for c in cases if c.cap <= 16383]
    assert max(c.cap for c in part) == 16383
    pipeline_route(ctx, part, 16383)


def test_lane_passes_with_the_multiblock_pass(ctx, cases):
    """max_len > 16383 turns multi_pass on (pmc_capi.hip:1170, 1176-1178): members above the record kernel's
    4 KiB whose first block is not their last go to inflate_lane_kernel<128,true>, which meets stored blocks and
    defects in later blocks (pmc_inflate_lane.hip:661-671) after it has written earlier blocks to dst; the wave
    kernels redo those.  (Smaller members of several blocks never reach that pass: the record kernel calls
    lane_prepare without `multi` and declines them straight to the wave kernels, pmc_inflate_rec.hip:280.)
    The fast passes must decode the plain single-block zlib members themselves: the retry counter may not
    grow by the whole corpus."""
    max_len = max(c.cap for c in cases)
    assert max_len > 16383
    grew = pipeline_route(ctx, cases, max_len)
    assert grew < len(cases), (grew, len(cases))


def test_host_calls(ctx, cases):
    """ctx.decompress_many: calls within the latency limits (<= 4,096 members of <= 48 KiB capacity and
    <= 16 MiB of output, pmc_plan.hpp inflate_latency) take the wave kernel over host memory, one call of
    more members takes the throughput pipeline -- both confirmed by the context's path counters."""
    import pmc_codec

    def call(part, pad_to=0):
        members = [c.member for c in part]
        caps = [c.cap for c in part]
        if pad_to > len(part):
            z = zlib.compressobj(6, zlib.DEFLATED, 31)
            pad = z.compress(PAD_VALUE) + z.flush()
            members += [pad] * (pad_to - len(part))
            caps += [len(PAD_VALUE)] * (pad_to - len(part))
        res = ctx.decompress_many(members, caps)
        assert res[len(part):] == [(0, PAD_VALUE)] * (len(res) - len(part))
        bad = [(c.name, c.cap, r[0], c.rc) for c, r in zip(part, res) if r[0] != c.rc or (c.rc == 0 and r[1] != c.out)]
        assert not bad, (len(bad), bad[:8])
        return [Case(c.name + "@needed", c.member, c.need) for c in part if c.rc == pmc_codec.E_CAPACITY]

    within = [c for c in cases if c.cap <= 48 * 1024]
    chunks, cur, total = [], [], 0
    for c in within:
        if len(cur) == 4096 or total + c.cap > (16 << 20):
            chunks.append(cur)
            cur, total = [], 0
        cur.append(c)
        total += c.cap
    chunks.append(cur)
    before = ctx.path_counts()
    again = []
    for part in chunks:
        again += call(part)
    mid = ctx.path_counts()
    assert mid["latency_decompress"] - before["latency_decompress"] == len(chunks)
    assert mid["pipeline_decompress"] == before["pipeline_decompress"]
    again += call(cases, max(PIPELINE_N, len(cases) + 1))
    after = ctx.path_counts()
    assert after["pipeline_decompress"] - mid["pipeline_decompress"] == 1
    assert after["latency_decompress"] == mid["latency_decompress"]
    if again:  # PMC_E_CAPACITY answers: the size the oracle reports suffices for a verdict
        assert all(c.rc != pmc_codec.E_CAPACITY for c in again)
        assert call(again) == []

"""GPU: the boundaries of a compress call -- what it reads around a value and what it writes around a slot.

Inputs are tests/boundary_values.py's: every value is a window of a 1 MiB stream (periods 1, 2, 259 and 4099, tiled
JSON) and is compressed where it lies, so the bytes on both sides continue it; tests/test_boundary_model.py (CPU)
holds every batch shape to the route it is meant for and to a share of windows whose member would change if a
matcher read a byte outside the value.  One test per route row; the rows behind an environment switch
(PMC_DEFLATE_V1, PMC_DEFLATE_MONO: read once per process) run in a child process each.

Reads (roomy call, capacities pmc_gzip_bound(len)): level 9 must give the reference's member of every value
(tests/golden/boundary_golden.json) and the oracle's; a fast level must give, byte for byte, the member a control
call gives for the same values packed by pmc_codec.device.pack (apart, zero bytes between them), which must inflate
to the value.

Writes (tight calls): the same sources, capacities cycling over need, need - 1, need + 1, 0, 17 and
pmc_gzip_bound(len) (need: the member's size), slots at unaligned offsets with 1-7 guard bytes between them and 64
behind the last, everything prefilled 0xA5, dst_len prefilled 12345 and rc 7.  A value whose capacity suffices
must give rc 0, dst_len = need and the roomy call's bytes; every other one PMC_E_CAPACITY and dst_len 0; and no
byte outside [dst_off, dst_off + need) of the successful values may change -- guard bytes, failed slots and the
unused tail of roomy slots alike.  The cycle runs twice, the second time with neighbours swapped, so every value
meets a sufficient and a short capacity.

The host-memory entries (pmc_gzip_compress_batch_host with packed slots on both of its routes,
pmc_gzip_compress_batch_pinned scattered, packed and tiled) get the same capacity cycle."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import boundary_values as BV

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 0xA5
E_CAPACITY = -101
NO_RETRY_ROWS = ("mono", "split-s12", "split", "fast")  # the retry counter must not grow on these


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


def bounds(lens):
    import pmc_codec
    return pmc_codec.gzip_bounds(lens).astype(np.int64)


# The capacity cycle over need, need - 1, need + 1, 0, min(need - 1, 17), pmc_gzip_bound(len), and the same with
# neighbours swapped: a value that meets a sufficient capacity in the one meets a short one in the other
CYCLES = ((0, 1, 2, 3, 4, 5), (1, 0, 3, 2, 5, 4))


def capacities(need, lens, cycle=0):
    """The capacity cycle, and the condition it is chosen for: at least a third of the values short, at least a
    third exact or one over."""
    bound = bounds(lens)
    kinds = [lambda k: need[k], lambda k: need[k] - 1, lambda k: need[k] + 1, lambda k: 0,
             lambda k: min(need[k] - 1, 17), lambda k: bound[k]]
    caps = np.array([kinds[CYCLES[cycle][k % 6]](k) for k in range(len(need))], dtype=np.int64)
    need = np.asarray(need, dtype=np.int64)
    assert (caps >= 0).all() and (need <= bound).all()
    assert 3 * int((caps < need).sum()) >= len(need), "capacity cycle: too few short slots"
    assert 3 * int(((caps == need) | (caps == need + 1)).sum()) >= len(need), "capacity cycle: too few exact slots"
    return caps


def check_slots(tag, ws, members, caps, off, rc, dlen, out, filled):
    """The verdicts, lengths and bytes of a tight call, and that nothing outside the successful members changed.
    out: the destination after the call, filled: before it."""
    bad = []
    untouched = np.ones(len(out), dtype=bool)
    for k, m in enumerate(members):
        need, o = len(m), int(off[k])
        if caps[k] >= need:
            if rc[k] != 0 or dlen[k] != need or out[o:o + need].tobytes() != m:
                bad.append((k, ws[k], "cap", int(caps[k]), "need", need, "rc", int(rc[k]), "dst_len", int(dlen[k])))
            untouched[o:o + need] = False
        elif rc[k] != E_CAPACITY or dlen[k] != 0:
            bad.append((k, ws[k], "cap", int(caps[k]), "need", need, "rc", int(rc[k]), "dst_len", int(dlen[k])))
    assert not bad, (tag, len(bad), bad[:6])
    changed = np.flatnonzero(untouched & (out != filled))
    if len(changed):
        at = int(changed[0])
        k = int(np.searchsorted(np.asarray(off), at, side="right")) - 1
        raise AssertionError(f"{tag}: {len(changed)} bytes outside the members changed, first at {at}: slot {k} ({ws[k]}) is "
                             f"[{int(off[k])}, {int(off[k]) + int(caps[k])}), its member {len(members[k])} bytes, "
                             f"rc {int(rc[k])}")


class Call:
    """The device tensors of one batch shape: the streams (with a random window's bytes written in), offsets and
    lengths."""

    def __init__(self, ws):
        import torch
        self.ws = ws
        self.lens = np.array([w.n for w in ws], dtype=np.int64)
        self.src = torch.from_numpy(BV.source_for(ws)).cuda()
        self.soff = torch.from_numpy(np.array([w.off for w in ws], dtype=np.int64)).cuda()
        self.slen = torch.from_numpy(self.lens.astype(np.int32)).cuda()
        self.max_len = int(self.lens.max())
        self.values = [BV.value(w) for w in ws]

    def compress(self, ctx, caps, off, total):
        """One pmc_gzip_compress_batch into a 0xA5-filled buffer of `total` bytes -> (rc, dst_len, bytes after,
        bytes before)."""
        import torch
        from pmc_codec import device as D
        n = len(self.ws)
        filled = np.full(total, GUARD, dtype=np.uint8)
        dst = torch.from_numpy(filled.copy()).cuda()
        doff = torch.from_numpy(np.asarray(off, dtype=np.int64)).cuda()
        dcap = torch.from_numpy(np.asarray(caps, dtype=np.int64).astype(np.int32)).cuda()
        dlen = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
        rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.compress_device(self.src, self.soff, self.slen, dst, doff, dcap, dlen, rc, self.max_len, D.stream_handle())
        torch.cuda.synchronize()
        return rc.cpu().numpy(), dlen.cpu().numpy(), dst.cpu().numpy(), filled


def unaligned_slots(caps, seed):
    """Slots at unaligned offsets, 1-7 guard bytes between them, 64 behind the last (the layout of
    test_gpu_foreign.device_call)."""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(caps), dtype=np.int64)
    pos = 3
    for i in range(len(caps)):
        off[i] = pos
        # the next slot's offset modulo 4 steps on by one, and once more after every capacity cycle, so every
        # kind of capacity meets every alignment; of the two gaps that give it, one at random
        want = (3 + (i + 1) + (i + 1) // 6) % 4
        gap = (want - (pos + int(caps[i]))) % 4 or 4
        pos += int(caps[i]) + (gap + 4 if gap <= 3 and rng.integers(0, 2) else gap)
    return off, pos + 64


def roomy(ctx, call):
    """The roomy call: rc 0 for every value -> the members."""
    caps = bounds(call.lens)
    off = np.concatenate([[0], np.cumsum((caps + 3) & ~3)[:-1]])
    rc, dlen, out, _ = call.compress(ctx, caps, off, int(off[-1] + caps[-1] + 64))
    bad = [(k, call.ws[k], int(rc[k])) for k in range(len(rc)) if rc[k] != 0]
    assert not bad, bad[:8]
    return [out[int(off[k]):int(off[k]) + int(dlen[k])].tobytes() for k in range(len(rc))]


def tight(ctx, call, members, tag):
    need = np.array([len(m) for m in members], dtype=np.int64)
    for cycle in (0, 1):
        caps = capacities(need, call.lens, cycle)
        off, total = unaligned_slots(caps, 11 + cycle)
        assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
        rc, dlen, out, filled = call.compress(ctx, caps, off, total)
        check_slots(f"{tag} cycle {cycle}", call.ws, members, caps, off, rc, dlen, out, filled)


def explain_first(got, want):
    import deflate_dissect
    k = next(k for k in range(len(want)) if got[k] != want[k])
    return k, deflate_dissect.explain(got[k], want[k])


def level9_shape(ctx, row, shape, golden):
    """One level-9 batch: reads against the reference and the oracle, then the tight calls.  Returns the growth
    of the retry counter over the roomy call."""
    from oracle import pyoracle as O
    call = Call(BV.shape(shape))
    before = ctx.guard_counts()["retry"]
    members = roomy(ctx, call)
    grew = ctx.guard_counts()["retry"] - before
    want = [O.compress(v) for v in call.values]
    if members != want:
        k, why = explain_first(members, want)
        raise AssertionError(f"{row}/{shape}: {sum(a != b for a, b in zip(members, want))} members differ from the "
                             f"oracle's, first {call.ws[k]}: {why}")
    bad = golden.mismatches(call.values, members)
    assert not bad, (row, shape, "reference", [call.ws[k] for k in bad[:8]])
    tight(ctx, call, members, f"{row}/{shape}")
    return grew, call, members


def inflate(member, dictionary):
    """The value of a member by a decoder that is not this library's: the oracle, or for a dictionary member
    (header bytes 4..7 hold the dictionary's id) zlib's raw inflate behind the dictionary."""
    from oracle import pyoracle as O
    if dictionary and member[3] == 0 and member[4:8] == struct.pack("<I", zlib.crc32(dictionary)) and member[8] == 4:
        v = zlib.decompressobj(-15, zdict=dictionary).decompress(member[10:-8])
        assert member[-8:] == struct.pack("<II", zlib.crc32(v), len(v))
        return v
    rc, v = O.decompress(member)
    assert rc == 0, rc
    return v


def fast_row(ctx, row):
    """A fast-level row: the windows' members equal the control call's (the same values packed apart, zero
    bytes between them, on the same context), which inflate to the values; then the tight calls."""
    import torch
    from pmc_codec import device as D
    r = BV.ROWS[row]
    d = BV.dictionary() if r.get("dict") else None
    ctx.level = r["level"]
    try:
        if d:
            ctx.set_dictionary(d)
        ctx.index = bool(r.get("index"))
        ctx.index_crc = bool(r.get("index_crc"))
        (shape,) = r["shapes"]
        call = Call(BV.shape(shape))
        before = ctx.guard_counts()["retry"]
        members = roomy(ctx, call)
        grew = ctx.guard_counts()["retry"] - before
        out, rc = D.compress(ctx, D.pack(call.values))
        torch.cuda.synchronize()
        assert int((rc != 0).sum()) == 0
        control = out.host_items()
        bad = [(k, call.ws[k]) for k in range(len(members)) if members[k] != control[k]]
        if bad:
            k, why = explain_first(members, control)
            raise AssertionError(f"{row}: {len(bad)} members differ from the control call's, first {call.ws[k]}: {why}")
        bad = [(k, call.ws[k]) for k, (m, v) in enumerate(zip(members, call.values)) if inflate(m, d) != v]
        assert not bad, (row, "inflate", bad[:8])
        # the members are the level's own: fast members (header byte 8 = 4), dictionary marks and indexes where meant
        import pmc_codec
        assert all(m[8] == 4 for m in members), row
        if d:
            marked = [m[4:8] != bytes(4) for m in members]
            assert marked == [w.n <= BV.DICT_EDGE for w in call.ws], row
        if r.get("index"):
            assert all(pmc_codec.index_info(m) == (32768, -(-w.n // 32768)) for m, w in zip(members, call.ws)), row
            assert all((pmc_codec.index_crc_info(m) is not None) == bool(r.get("index_crc")) for m in members), row
        if row in NO_RETRY_ROWS:
            assert grew == 0, (row, grew)
        tight(ctx, call, members, row)
    finally:
        ctx.index_crc = False
        ctx.index = False
        if d:
            ctx.set_dictionary(None)
        ctx.level = BV.EXACT


def level9_row(ctx, row):
    import torch
    from pmc_codec import device as D
    golden = BV.BoundaryGolden()
    for shape in BV.ROWS[row]["shapes"]:
        grew, call, members = level9_shape(ctx, row, shape, golden)
        print(f"{row}/{shape}: {len(members)} values, retry +{grew}")
        if row == "big":  # the gated HBM kernel really ran: it redid the value of several blocks
            assert grew >= 1, (row, grew)
        if row in NO_RETRY_ROWS:
            assert grew == 0, (row, grew)
        if row == "lv" and shape == "lv-json":
            # Tiled JSON stitches (tests/test_gpu_large.py holds it to that), so a retry here is a parse that did
            # not end on its value's last byte: every one of these windows ends in a match that the byte behind
            # the value would lengthen, and the emit kernel declines a token stream of another length than the
            # value's -- the HBM kernel would then redo it to the right bytes, and only this counter would tell
            # (a lane-order guard would count here too: none has fired on gfx950, and tests/test_gpu_large.py
            # holds its JSON values to the same counter)
            assert grew == 0, (row, shape, grew)
        if row == "lv" and shape == "lv":
            # the same reading on more windows: only the large period-1 and period-2 windows may take the
            # stitch's fallback, so the counter may grow by at most their number; one retry of a large p259,
            # p4099 or JSON window beside theirs exceeds it
            may = sum(1 for w in call.ws if w.n > 16382 and w.name in ("p1", "p2"))
            assert may == 6 and grew <= may, (row, shape, grew, may)
        if shape in ("lv", "lv-json"):  # (lv: periodic windows may take the stitch's fallback, no counter check)
            back, brc = D.decompress(ctx, D.pack(members), [len(v) for v in call.values])
            torch.cuda.synchronize()
            assert int((brc != 0).sum()) == 0
            assert back.host_items() == call.values


def child(row):
    """A row behind an environment switch, in a process of its own (the switches are read once per process)."""
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    try:
        level9_row(c, row)
    finally:
        c.close()


CHILD = "import sys; sys.path[:0] = [sys.argv[1]]; import conftest; import test_gpu_compress_bounds as T; T.child(sys.argv[2])"


@pytest.mark.parametrize("row", list(BV.ROWS))
def test_route_row(ctx, row):
    r = BV.ROWS[row]
    if r.get("env"):
        import torch
        torch.cuda.synchronize()  # (raises if an earlier test left the device in error: then no child is started)
        env = dict(os.environ, **{r["env"]: "1"})
        out = subprocess.run([sys.executable, "-c", CHILD, HERE, row], env=env, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    elif r["level"] == BV.EXACT:
        level9_row(ctx, row)
    else:
        fast_row(ctx, row)


# ---- host-memory entries ------------------------------------------------------------------------------------
def small_windows(n):
    """n windows of the split-s12 shape, every edge length up to 4096 among them: its first 75 windows are the
    edge lengths on every stream (a batch of under 75 drops one stream of each, by turns)."""
    ws = BV.shape("split-s12")
    if n < 75:
        ws = [w for k, w in enumerate(ws[:75]) if k % 5 != (k // 5) % 5] + ws[75:]
    ws = ws[:n]
    assert {w.n for w in ws} >= set(BV.EDGE_4K) and max(w.n for w in ws) == 4096
    return ws


@pytest.mark.parametrize("n,route", [(64, "latency_compress"), (1100, "pipeline_compress")])
def test_host_entry_packed_slots(ctx, n, route):
    """pmc_gzip_compress_batch_host with dst_off == NULL: slot i starts where slot i - 1's capacity ends, so every
    slot's neighbours are its canaries; failed slots and the bytes behind dst_len stay as they were."""
    import pmc_codec
    from oracle import pyoracle as O
    ws = small_windows(n)
    members = [O.compress(BV.value(w)) for w in ws]
    need = np.array([len(m) for m in members], dtype=np.int64)
    lens = np.array([w.n for w in ws], dtype=np.int64)
    src = BV.source_for(ws)
    soff = np.array([w.off for w in ws], dtype=np.uint64)
    slen = lens.astype(np.uint32)
    for cycle in (0, 1):
        caps = capacities(need, lens, cycle)
        off = np.concatenate([[0], np.cumsum(caps)[:-1]])
        filled = np.full(int(caps.sum()) + 64, GUARD, dtype=np.uint8)
        dst = filled.copy()
        cap32 = caps.astype(np.uint32)
        dlen = np.full(n, 12345, dtype=np.uint32)
        rc = np.full(n, 7, dtype=np.int32)
        before = ctx.path_counts()
        r = pmc_codec.lib().pmc_gzip_compress_batch_host(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, n,
                                                         dst.ctypes.data, None, cap32.ctypes.data, dlen.ctypes.data,
                                                         rc.ctypes.data)
        assert r == 0, pmc_codec.last_error()
        after = ctx.path_counts()
        assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {route: 1}
        check_slots(f"host n={n} cycle {cycle}", ws, members, caps, off, rc, dlen.astype(np.int64), dst, filled)


@pytest.mark.parametrize("mode", ["scattered", "packed", "tiled"])
def test_pinned_entry(ctx, mode):
    """pmc_gzip_compress_batch_pinned, 200 values in chunks of 64.  Scattered slots (gaps between them): only
    [dst_off, dst_off + dst_len) of the successful values is written.  Packed (dst_off NULL): the successful
    members back to back, nothing behind them.  Tiled slots: the range is written back whole and slot bytes past
    dst_len and failed slots are unspecified (include/pmc_codec.h), so only the members and the bytes outside the
    tiled range are checked."""
    import torch
    from oracle import pyoracle as O
    n = 200
    ws = small_windows(n)
    members = [O.compress(BV.value(w)) for w in ws]
    need = np.array([len(m) for m in members], dtype=np.int64)
    lens = np.array([w.n for w in ws], dtype=np.int64)
    pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
    src = torch.from_numpy(BV.source_for(ws)).pin_memory()
    for cycle in (0, 1):
        caps = capacities(need, lens, cycle)
        if mode == "scattered":
            off, total = unaligned_slots(caps, 5 + cycle)
        else:
            off = 5 + np.concatenate([[0], np.cumsum(caps)[:-1]])
            total = int(5 + caps.sum() + 64)
        filled = np.full(total, GUARD, dtype=np.uint8)
        dst = torch.from_numpy(filled.copy()).pin_memory()
        dlen = torch.full((n,), 12345, dtype=torch.int32).pin_memory()
        rc = torch.full((n,), 7, dtype=torch.int32).pin_memory()
        base = dst[5:] if mode == "packed" else dst
        ctx.compress_pinned(src, pin([w.off for w in ws], np.int64), pin(lens, np.int32), base,
                            None if mode == "packed" else pin(off, np.int64), pin(caps, np.int32), dlen, rc, 4096, 64)
        rc, dlen, out = rc.numpy(), dlen.numpy().astype(np.int64), dst.numpy()
        ok = caps >= need
        if mode == "packed":  # output i at the sum of the successful lengths before it
            off = 5 + np.concatenate([[0], np.cumsum(np.where(ok, need, 0))[:-1]])
        if mode == "tiled":
            bad = [(k, ws[k], int(rc[k]), int(dlen[k])) for k in range(n)
                   if (rc[k] != 0 or dlen[k] != need[k] or out[off[k]:off[k] + need[k]].tobytes() != members[k]) if ok[k]]
            bad += [(k, ws[k], int(rc[k]), int(dlen[k])) for k in range(n) if not ok[k] and (rc[k] != E_CAPACITY or dlen[k] != 0)]
            assert not bad, (cycle, len(bad), bad[:6])
            assert (out[:5] == GUARD).all() and (out[5 + int(caps.sum()):] == GUARD).all()
        else:
            check_slots(f"pinned {mode} cycle {cycle}", ws, members, caps, off, rc, dlen, out, filled)

"""GPU: ranged reads of indexed members (include/pmc_codec.h "ranged reads").

pmc_gzip_decompress_range_batch returns bytes [off, off + len) of a value, clamped as Redis GETRANGE clamps,
and decodes only the chunks that hold them (pmc_ctx_range_counts proves it); it writes nothing outside a
request's slot, declines (PMC_E_NO_INDEX) every member it cannot serve by its chunks, and judges damaged
members as tests/range_model.py does.  pmc_store_get_range_batch always returns the range, falling back to a
whole read where the ranged call declines.  Slots lie at unaligned offsets with 16 canary bytes on both sides."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from fast_large_values import BIG_NAME
from indexed_model import C, assemble, parse_index
from indexed_values import RANDOM_NAME, indexed_values
from range_model import chunk_bytes, chunk_span, covered, range_of, ranges_for, read_range
from test_gpu_indexed import corruptions

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 0xA5
CANARY = 16


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    c.level = pmc_codec.LEVEL_FAST_ALL
    c.index = True
    yield c
    c.close()


def device_compress(ctx, values):
    import torch
    from pmc_codec import device as D
    out, rc = D.compress(ctx, D.pack(values, align=1))
    torch.cuda.synchronize()
    assert int((rc != 0).sum()) == 0, rc
    return out.host_items()


@pytest.fixture(scope="module")
def vals(golden):
    return indexed_values(golden.corpus)


@pytest.fixture(scope="module")
def members(ctx, vals):
    """The whole value list as one device batch, level fast-all, index on (computed once, never changed)."""
    return device_compress(ctx, [v for _, v in vals])


def clamp(n, off, ln):
    o = min(off, n)
    return o, min(ln, n - o)


def ranged_call(ctx, reqs, caps=None, seed=1):
    """One device call over reqs = [(member, off, len)]; requests of the same member object alias its bytes.
    Slot i has caps[i] bytes (default: the clamped length), an unaligned offset and CANARY guard bytes on both
    sides.  Asserts that no byte outside the slots changed; returns (rc, dst_len, [slot bytes])."""
    import torch
    from pmc_codec import device as D
    rng = np.random.default_rng(seed)
    n = len(reqs)
    uniq, where = [], {}
    for m, _, _ in reqs:
        if id(m) not in where:
            where[id(m)] = len(uniq)
            uniq.append(m)
    b = D.pack(uniq, align=1)
    ix = torch.from_numpy(np.array([where[id(m)] for m, _, _ in reqs], dtype=np.int64)).cuda()
    soff, slen = b.off[ix].contiguous(), b.len[ix].contiguous()
    if caps is None:
        caps = [clamp(int.from_bytes(m[-4:], "little"), off, ln)[1] for m, off, ln in reqs]
    caps = np.asarray(caps, dtype=np.int64)
    gaps = rng.integers(0, 4, n)
    off = np.zeros(n, dtype=np.int64)
    pos = CANARY + 3
    for i in range(n):
        off[i] = pos
        pos += int(caps[i]) + CANARY + int(gaps[i])
    host0 = np.full(pos + CANARY, GUARD, dtype=np.uint8)
    dst = torch.from_numpy(host0.copy()).cuda()
    doff = torch.from_numpy(off).cuda()
    dcap = torch.from_numpy(caps.astype(np.uint32).view(np.int32).copy()).cuda()
    roff = torch.from_numpy(np.array([r[1] for r in reqs], dtype=np.uint32).view(np.int32).copy()).cuda()
    rlen = torch.from_numpy(np.array([r[2] for r in reqs], dtype=np.uint32).view(np.int32).copy()).cuda()
    dlen = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.decompress_range_device(b.data, soff, slen, roff, rlen, dst, doff, dcap, dlen, rc, D.stream_handle())
    torch.cuda.synchronize()
    rc, dlen, out = rc.cpu().numpy(), dlen.cpu().numpy().view(np.uint32), dst.cpu().numpy()
    outside = np.ones(len(out), dtype=bool)
    for i in range(n):
        outside[off[i]:off[i] + caps[i]] = False
    changed = np.flatnonzero(outside & (out != host0))
    assert len(changed) == 0, f"{len(changed)} bytes outside the slots changed, first at {int(changed[0])}"
    return rc, dlen, [out[off[i]:off[i] + caps[i]].tobytes() for i in range(n)]


def counted(ctx, fn):
    a = ctx.range_counts()
    res = fn()
    b = ctx.range_counts()
    return res, tuple(int(b[k] - a[k]) for k in ("served", "declined", "chunks"))


def untouched(slot):
    return slot == bytes([GUARD]) * len(slot)


def test_bytes_and_bounds(ctx, vals, members):
    import pmc_codec
    reqs, want, chunks = [], [], 0
    for (name, v), m in zip(vals, members):
        if name == RANDOM_NAME or len(v) <= C:
            continue
        assert pmc_codec.index_info(m) == (C, -(-len(v) // C)), name
        for off, ln in ranges_for(len(v), C):
            reqs.append((m, off, ln))
            want.append(v[off:off + ln])
            chunks += range_of(len(v), 15, off, ln)[3]
    assert len(reqs) > 150
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
    bad = [(k, int(rc[k]), int(dlen[k]), len(want[k])) for k in range(len(reqs))
           if rc[k] != 0 or dlen[k] != len(want[k]) or slots[k] != want[k]]
    assert not bad, (len(bad), bad[:8])
    assert got == (len(reqs), 0, chunks), (got, len(reqs), chunks)
    # one byte of a 33-chunk member costs one chunk
    v, m = next((v, m) for (name, v), m in zip(vals, members) if name == BIG_NAME)
    assert -(-len(v) // C) >= 32
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, [(m, C, 1)]))
    assert (int(rc[0]), int(dlen[0]), slots[0]) == (0, 1, v[C:C + 1]) and got == (1, 0, 1), got


def test_capacity(ctx, vals, members):
    import pmc_codec
    by = {n: (v, m) for (n, v), m in zip(vals, members)}
    v, m = by["json100000"]
    reqs = [(m, 0, 1), (m, C - 1, 2), (m, C, C), (m, 0, len(v)), (m, len(v) - 3, 10), (m, 0, 0xFFFFFFFF)]
    need = [clamp(len(v), off, ln)[1] for _, off, ln in reqs]
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs, caps=[x - 1 for x in need]))
    assert list(rc) == [pmc_codec.E_CAPACITY] * len(reqs) and [int(x) for x in dlen] == need
    assert all(untouched(s) for s in slots) and got == (0, 0, 0), got
    # a capacity above the need is fine, and only the need is written
    rc, dlen, slots = ranged_call(ctx, reqs[:3], caps=[x + 5 for x in need[:3]])
    for k, (_, off, ln) in enumerate(reqs[:3]):
        assert rc[k] == 0 and dlen[k] == need[k] and slots[k] == v[off:off + ln] + bytes([GUARD]) * 5


def test_declined_members(ctx, vals, members):
    import pmc_codec
    from fast_large_model import fast_large_tokens
    by = {n: (v, m) for (n, v), m in zip(vals, members)}
    v, m = by["json100000"]
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        exact = device_compress(ctx, [v])[0]
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index = False
        plain = device_compress(ctx, [v])[0]
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index = True
    assert exact[3] == 0 and plain[3] == 0 and pmc_codec.index_info(m) is not None
    z = zlib.compressobj(6, zlib.DEFLATED, 31)
    foreign = z.compress(v) + z.flush()
    small_v, small_m = by[f"json{C}"]
    rand_v, rand_m = by[RANDOM_NAME]
    assert pmc_codec.index_info(rand_m) is not None and pmc_codec.index_info(small_m) is None
    wide_v = v * 3
    wide = assemble(wide_v, chunk=1 << 17)
    assert pmc_codec.index_info(wide) == (1 << 17, 3) and zlib.decompress(wide, 31) == wide_v
    reqs = []
    for mm in (exact, plain, foreign, small_m, rand_m, wide):
        reqs += [(mm, 0, 100), (mm, C - 1, 2), (mm, C, C)]
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
    assert list(rc) == [pmc_codec.E_NO_INDEX] * len(reqs), list(rc)
    # (only the member with stored blocks reaches the decoder: 1 + 2 + 1 chunks are given to it)
    assert not dlen.any() and all(untouched(s) for s in slots) and got == (0, len(reqs), 4), got
    # a foreign index: chunks of 4 KiB in fixed blocks, put together on the CPU, is served ...
    fv = by[f"json{C + 1}"][0]
    good = assemble(fv, chunk=4096)
    reqs = [(good, off, ln) for off, ln in ranges_for(len(fv), 4096)]
    rc, dlen, slots = ranged_call(ctx, reqs)
    assert not rc.any() and [s for s in slots] == [fv[off:off + ln] for _, off, ln in reqs]
    # ... and its variant whose matches reach before their chunks (the unchunked parse, cut at multiples of
    # 4 KiB): served in chunk 0, declined in a chunk that reaches back
    cut, p = [[]], 0
    for t in fast_large_tokens(fv):
        cut[-1].append(t)
        p += t[0] if isinstance(t, tuple) else 1
        if p % 4096 == 0 and p < len(fv):
            cut.append([])
    it = iter(cut)
    reaching = assemble(fv, chunk=4096, tokens_of=lambda part: next(it))
    assert zlib.decompress(reaching, 31) == fv and pmc_codec.index_info(reaching) == (4096, 9)
    back = [k for k in range(9) if chunk_bytes(reaching, k) is None]
    assert back and 0 not in back
    k = back[0]
    reqs = [(reaching, 7, 50), (reaching, 4096 * k + 7, 50), (reaching, 4096 * k, 4096), (reaching, 0, 4096)]
    rc, dlen, slots = ranged_call(ctx, reqs)
    assert list(rc) == [0, pmc_codec.E_NO_INDEX, pmc_codec.E_NO_INDEX, 0], list(rc)
    assert slots[0] == fv[7:57] and slots[3] == fv[:4096] and list(dlen) == [50, 0, 0, 4096]
    assert untouched(slots[1])  # (an edge chunk: decoded into scratch)


def test_damaged_members(ctx, vals, members):
    import pmc_codec
    by = {n: (v, m) for (n, v), m in zip(vals, members)}
    reqs, info = [], []
    for name in (f"json{2 * C + 3}", "json100000"):
        v, m = by[name]
        for cname, b in corruptions(m):
            if len(b) < 18:
                b = b + bytes(18 - len(b))  # (the packing reads ISIZE for the default capacity)
            for off, ln in ((5, 100), (C - 3, 9), (len(v) - 50, 50)):
                model = read_range(b, off, ln)
                ks = covered(b, off, ln)
                same = False
                if ks is not None and ks == covered(m, off, ln) and len(b) == len(m):
                    spans = [chunk_span(m, k)[:2] for k in ks]
                    same = (parse_index(b)[:2] == parse_index(m)[:2] and b[-4:] == m[-4:]
                            and [chunk_span(b, k)[:2] for k in ks] == spans and all(b[s:e] == m[s:e] for s, e in spans))
                    assert not same or model == v[off:off + ln]
                reqs.append((b, off, ln))
                info.append((f"{name}:{cname}@{off}", model, same))
    assert len(reqs) > 1200 and sum(1 for i in info if i[2]) >= 100 and sum(1 for i in info if i[1] is None) >= 100
    rc, dlen, slots = ranged_call(ctx, reqs, caps=[ln for _, _, ln in reqs])
    bad = []
    for k, (name, model, same) in enumerate(info):
        if rc[k] not in (0, pmc_codec.E_NO_INDEX):
            bad.append((name, "rc", int(rc[k])))
        elif model is None and rc[k] != pmc_codec.E_NO_INDEX:
            bad.append((name, "served what the model declines", int(rc[k])))
        elif rc[k] == 0 and (not isinstance(model, bytes) or dlen[k] != len(model) or slots[k][:dlen[k]] != model):
            bad.append((name, "bytes", int(dlen[k])))
        elif same and rc[k] != 0:
            bad.append((name, "declined untouched chunks", int(rc[k])))
        elif rc[k] != 0 and dlen[k] != 0:
            bad.append((name, "dst_len", int(dlen[k])))
    assert not bad, (len(bad), bad[:8])


def test_more_items_than_one_grid_pass(ctx, vals, members):
    """100,000 requests of 16 bytes: every item is an edge chunk, and the rows are reused across the grid-stride
    loop (csrc/pmc_plan.hpp plan_range: more requests than rows)."""
    pick = [(v, m) for (name, v), m in zip(vals, members) if name != RANDOM_NAME and len(v) > C]
    rng = np.random.default_rng(20264)
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
    chunks = int((((offs + 15) >> 15) - (offs >> 15) + 1).sum())
    assert chunks > n
    (rc, dlen, slots), got = counted(ctx, lambda: ranged_call(ctx, reqs))
    odd = np.flatnonzero((rc != 0) | (dlen != 16))
    print("requests not served in full:", len(odd), [(int(k), int(rc[k]), int(dlen[k]), int(offs[k])) for k in odd[:8]])
    assert not rc.any() and (dlen == 16).all()
    assert (np.frombuffer(b"".join(slots), dtype=np.uint8).reshape(n, 16) == want).all()
    assert got == (n, 0, chunks), (got, chunks)


def expect_frame(frame, b):
    import pmc_codec
    if frame == pmc_codec.FRAME_RESP:
        return b"$%d\r\n" % len(b) + b + b"\r\n"
    return b


def store_pairs(values):
    return [(i, max(off, 0), max(ln, 0)) for i, v in enumerate(values) for off, ln in ranges_for(len(v), C)]


def repeat_extents(ext, idx):
    import pmc_codec
    out = (pmc_codec.Extent * len(idx))()
    for k, i in enumerate(idx):
        out[k] = ext[i]
    return out


def store_check(ctx, st, values, ext, frames):
    pairs = store_pairs(values)
    e = repeat_extents(ext, [i for i, _, _ in pairs])
    for frame in frames:
        res = st.get_range(e, [(off, ln) for _, off, ln in pairs], frame=frame)
        bad = [(i, off, ln, r[0]) for (i, off, ln), r in zip(pairs, res)
               if r != (0, expect_frame(frame, values[i][off:off + ln]))]
        assert not bad, (frame, len(bad), bad[:8])
    return pairs


STORE_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1]]
from conftest import Golden
from indexed_values import indexed_values
from fast_large_values import BIG_NAME
from test_gpu_range import store_check
import pmc_codec
vals = [v for n, v in indexed_values(Golden().corpus) if n != BIG_NAME] + [b"x", b"y" * 1024]
ctx = pmc_codec.Context(0)
ctx.level = pmc_codec.LEVEL_FAST_ALL
ctx.index = True
st = pmc_codec.Store(ctx, 16 << 20)
ext, rc = st.put(vals)
assert rc == [0] * len(vals)
assert any(pmc_codec.index_info(m) for m in st.members(ext, len(vals)))
pairs = store_check(ctx, st, vals, ext, [pmc_codec.FRAME_RAW])
res = {"pairs": len(pairs), "counts": ctx.range_counts(), "index": ctx.index_counts()}
st.close()
ctx.close()
print(json.dumps(res))
"""


def test_store(ctx, vals, members):
    import pmc_codec
    values = [v for _, v in vals] + [b"x", b"y" * 1024]
    names = [n for n, _ in vals] + ["one", "kib"]
    st = pmc_codec.Store(ctx, 32 << 20)
    try:
        ext, rc = st.put(values)
        assert rc == [0] * len(values)
        a = ctx.range_counts()
        pairs = store_check(ctx, st, values, ext, [pmc_codec.FRAME_RAW])
        b = ctx.range_counts()
        # the ranged call sees the non-empty ranges of values above 4 KiB: it serves the indexed ones and
        # declines (the store falls back) the value of C bytes and the one whose chunks hold stored blocks
        live = [(i, off, ln) for i, off, ln in pairs if clamp(len(values[i]), off, ln)[1] and len(values[i]) > 4096]
        served = [p for p in live if len(values[p[0]]) > C and names[p[0]] != RANDOM_NAME]
        assert (b["served"] - a["served"], b["declined"] - a["declined"]) == (len(served), len(live) - len(served))
        assert len(served) > 100 and len(live) - len(served) >= 10
        store_check(ctx, st, values, ext, [pmc_codec.FRAME_RESP])
        res = st.get_range(repeat_extents(ext, [0, 1]), [(0, 4), (C, 4)], frame=pmc_codec.FRAME_CUSTOM)
        assert res == [(0, values[0][:4] + b"\x1f"), (0, values[1][C:C + 4] + b"\x1f")]
        # a freed extent
        one = repeat_extents(ext, [2, 3])
        st.free(one, 1)
        res = st.get_range(one, [(0, 5), (0, 5)])
        assert res == [(pmc_codec.E_ARG, b""), (0, values[3][:5])]
    finally:
        st.close()
    # a level-9 store: everything through the whole reads, in more than one round (80 x 1 MiB of scratch)
    c9 = pmc_codec.Context(0)
    try:
        st9 = pmc_codec.Store(c9, 32 << 20)
        ext, rc = st9.put(values)
        assert rc == [0] * len(values) and all(m[3] == 0 for m in st9.members(ext, len(values)))
        pairs = store_check(c9, st9, values, ext, [pmc_codec.FRAME_RAW])
        live = [p for p in pairs if clamp(len(values[p[0]]), p[1], p[2])[1] and len(values[p[0]]) > 4096]
        assert c9.range_counts() == {"served": 0, "declined": len(live), "chunks": 0}
        big = names.index(BIG_NAME)
        rng = np.random.default_rng(7)
        rs = [(int(o), 33) for o in rng.integers(0, len(values[big]) - 33, 80)]
        res = st9.get_range(repeat_extents(ext, [big] * 80), rs, frame=pmc_codec.FRAME_RESP)
        assert res == [(0, expect_frame(pmc_codec.FRAME_RESP, values[big][o:o + 33])) for o, _ in rs]
        st9.close()
    finally:
        c9.close()
    # the fast paths off (a fresh process): every request is declined, and every result still right
    env = dict(os.environ, PMC_INFLATE_WAVE="1")
    out = subprocess.run([sys.executable, "-c", STORE_CHILD, HERE], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["counts"]["served"] == 0 and r["counts"]["chunks"] == 0 and r["counts"]["declined"] > 100, r
    assert r["index"] == {"completed": 0, "handed_over": 0}, r


def test_unchanged_ground(ctx, vals, members):
    """After the ranged calls, a full read of the same members gives the values through the chunk pass."""
    import torch
    from pmc_codec import device as D
    big = [(n, v, m) for (n, v), m in zip(vals, members) if len(v) > C]
    a = ctx.index_counts()
    ranged_call(ctx, [(m, C - 1, C + 2) for _, _, m in big])
    # (the packing helper beside device.decompress: slots of the clamped lengths)
    part, rc = D.decompress_range(ctx, D.pack([m for _, _, m in big], align=1), [C - 1] * len(big), [C + 2] * len(big))
    torch.cuda.synchronize()
    got = list(zip(rc.cpu().numpy().tolist(), part.host_items()))
    assert got == [(-103, b"") if n == RANDOM_NAME else (0, v[C - 1:2 * C + 1]) for n, v, _ in big]
    back, rc = D.decompress(ctx, D.pack([m for _, _, m in big], align=1), [len(v) for _, v, _ in big])
    torch.cuda.synchronize()
    assert not rc.cpu().numpy().any() and back.host_items() == [v for _, v, _ in big]
    b = ctx.index_counts()
    # every JSON / periodic member by the chunk pass; the random one handed over
    assert (b["completed"] - a["completed"], b["handed_over"] - a["handed_over"]) == (len(big) - 1, 1)

"""GPU: indexed members (include/pmc_codec.h "member index").

With the level at PMC_LEVEL_FAST_ALL and the index switch on, a value above C bytes becomes one valid gzip
member whose FEXTRA field names the byte where each chunk of C value bytes begins, whose chunks hold
tests/indexed_model.py's tokens and are separated by empty stored blocks; every other value gives the bytes
it gives with the switch off.  The member is the same whatever entry point, batch or position produced it.
The library's own decompress, on every route, gives each chunk to one lane (pmc_ctx_index_counts tells that
path from the fallback); a member whose index or stream is damaged gets the oracle's verdict and bytes, as
if FLG.FEXTRA were skipped; and under the lane-order fault build guarded values come out as level-9 bytes."""
import base64
import ctypes
import json
import os
import pickle
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

from deflate_dissect import dissect
from fast_large_values import BIG_NAME
from indexed_model import C, LOG2C, header, header_len, indexed_chunks, parse_index
from indexed_values import LAST_MATCH_NAME, RANDOM_NAME, indexed_values
from test_gpu_foreign import PAD_VALUE, PIPELINE_N, Case, check_route, device_call

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "poor-man-s-cache_amd", "pmc_codec")


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    c.level = pmc_codec.LEVEL_FAST_ALL
    assert c.index is False
    c.index = True
    assert c.index is True
    with pytest.raises(ValueError):
        c.index = 2
    assert c.index is True
    yield c
    c.close()


def device_compress(ctx, values):
    """One ragged device batch, the values packed back to back (unaligned offsets)."""
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
    """The whole value list as one device batch, level fast-all, index on (computed once)."""
    return device_compress(ctx, [v for _, v in vals])


def oracle_value(m):
    from oracle import pyoracle as O
    cap = int.from_bytes(m[-4:], "little")
    out = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_size_t(0)
    rc = O.lib().oracle_gzip_decompress(m, len(m), out, cap, ctypes.byref(n))
    return rc, out.raw[:n.value]


def split_blocks(m, hdr):
    """The member's blocks (tests/deflate_dissect.py, fed from ten bytes before the header's end) as chunks:
    [[block, ...], ...] cut at the empty stored blocks, and the byte offset in m that follows each of those."""
    blocks = dissect(m[hdr - 10:])
    chunks, after, cur = [], [], []
    for b in blocks:
        if b["type"] == 0 and b["stored_len"] == 0 and not b["last"]:
            chunks.append(cur)
            cur = []
            after.append(hdr - 10 + ((b["start_bit"] + 3 + 7) // 8) + 4)
        else:
            cur.append(b)
    chunks.append(cur)
    return chunks, after


def test_format_and_parity(ctx, vals, members):
    import pmc_codec
    for (name, v), m in zip(vals, members):
        assert len(m) <= pmc_codec.gzip_bound(len(v)), name
        assert zlib.decompress(m, 31) == v, name
        assert oracle_value(m) == (0, v), name
        if len(v) <= C:
            assert m[:4] == b"\x1f\x8b\x08\x00" and pmc_codec.index_info(m) is None, name
            continue
        k = -(-len(v) // C)
        hdr = header_len(len(v))
        cb, kk, offs, hend = parse_index(m)
        assert (cb, kk, hend) == (C, k, hdr) == pmc_codec.index_info(m) + (hdr,), name
        assert m[:hdr] == header(len(v), offs), name  # FLG = FEXTRA only, MTIME 0, XFL 4, OS 3, one subfield
        assert m[17] == LOG2C
        if name == BIG_NAME:
            continue
        chunks, after = split_blocks(m, hdr)
        # the index entries are the bytes that follow the empty stored blocks
        assert after == offs, name
        for o in offs:
            assert m[o - 4:o] == b"\x00\x00\xff\xff", name
        assert len(chunks) == k and all(len(c) >= 1 for c in chunks), name
        assert chunks[-1][-1]["last"] == 1 and sum(b["last"] for c in chunks for b in c) == 1, name
        if name == RANDOM_NAME:
            assert any(b["type"] == 0 for c in chunks for b in c)  # (round trip, bound and index only)
            continue
        assert all(b["type"] != 0 for c in chunks for b in c), name
        want = indexed_chunks(v)
        for j, (c, w) in enumerate(zip(chunks, want)):
            got = [t for b in c for t in b["tokens"]]
            if got != w:
                q = next((i for i in range(min(len(got), len(w))) if got[i] != w[i]), min(len(got), len(w)))
                raise AssertionError(f"{name} chunk {j}: tokens differ at #{q}: {got[q:q + 3]} vs {w[q:q + 3]}")
            assert all(len(b["tokens"]) == 16383 for b in c[:-1]) and 1 <= len(c[-1]["tokens"]) <= 16383, (name, j)
        if name == LAST_MATCH_NAME:  # the 16383rd symbol is the value's last token: it ends the final block
            assert [len(b["tokens"]) for b in chunks[-1]] == [16383] and chunks[-1][0]["last"] == 1
    assert ctx.guard_counts()["sort"] == 0


def test_unchanged_bytes(ctx, golden, vals, members):
    """Values of at most C bytes, and every value at level 9 and at `fast`, do not depend on the switch."""
    import pmc_codec
    from fast_values import edge_values
    small = [v for _, v in edge_values(golden.corpus)][::7] + [v for n, v in vals if len(v) <= C]
    small += [(golden.corpus * 2)[300:300 + n] for n in (16383, 20000, C - 1)]
    large = [v for n, v in vals if len(v) > C and n != BIG_NAME]
    try:
        on_small = device_compress(ctx, small)
        on = {}
        for lvl in (pmc_codec.LEVEL_EXACT, pmc_codec.LEVEL_FAST):
            ctx.level = lvl
            on[lvl] = device_compress(ctx, large + small[-4:])
        ctx.index = False
        for lvl in (pmc_codec.LEVEL_EXACT, pmc_codec.LEVEL_FAST):
            ctx.level = lvl
            assert device_compress(ctx, large + small[-4:]) == on[lvl], lvl
        assert all(m[3] == 0 and m[8] == 2 for m in on[pmc_codec.LEVEL_EXACT][:len(large)])
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        assert device_compress(ctx, small) == on_small
        off_large = device_compress(ctx, large)
        assert all(m[3] == 0 and pmc_codec.index_info(m) is None for m in off_large)
        by = dict(zip([n for n, v in vals if len(v) > C and n != BIG_NAME], off_large))
        ratio = {n: len(m) / len(by[n]) for (n, v), m in zip(vals, members) if n in by}
        print("indexed / plain member bytes:", {n: round(r, 4) for n, r in ratio.items()})
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index = True


def test_deterministic_across_batches_positions_and_entry_points(ctx, vals, members):
    import torch
    import pmc_codec
    from pmc_codec import device as D
    L = pmc_codec.lib()
    values = [v for _, v in vals]
    perm = np.random.default_rng(5).permutation(len(values))[:len(values) - 3]
    assert device_compress(ctx, [values[i] for i in perm]) == [members[i] for i in perm]
    i100 = [n for n, _ in vals].index("json100000")
    assert set(device_compress(ctx, [values[i100]] * 40)) == {members[i100]}
    pick = [i for i, (n, _) in enumerate(vals) if n != BIG_NAME]
    values, want = [values[i] for i in pick], [members[i] for i in pick]
    n = len(values)
    assert ctx.compress_many(values) == [(0, m) for m in want]  # host batch
    for v, m in list(zip(values, want))[1::5]:  # single value
        out = ctypes.create_string_buffer(pmc_codec.gzip_bound(len(v)))
        olen = ctypes.c_size_t(0)
        assert L.pmc_gzip_compress(ctx.handle, v, len(v), out, len(out), ctypes.byref(olen)) == 0
        assert out.raw[:olen.value] == m
    # pinned, pipelined in chunks of 3
    lens = np.array([len(v) for v in values], dtype=np.int64)
    caps = np.array([pmc_codec.gzip_bound(int(x)) for x in lens], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
    doff = np.concatenate([[0], np.cumsum(caps)[:-1]])
    pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
    src = torch.frombuffer(bytearray(b"".join(values) + bytes(64)), dtype=torch.uint8).pin_memory()
    dst = torch.zeros(int(caps.sum()) + 64, dtype=torch.uint8).pin_memory()
    dlen, rc = torch.zeros(n, dtype=torch.int32).pin_memory(), torch.full((n,), 7, dtype=torch.int32).pin_memory()
    ctx.compress_pinned(src, pin(soff, np.int64), pin(lens, np.int32), dst, pin(doff, np.int64), pin(caps, np.int32),
                        dlen, rc, int(lens.max()), 3)
    assert (rc.numpy() == 0).all()
    raw = dst.numpy().tobytes()
    assert [raw[int(doff[k]):int(doff[k]) + int(dlen[k])] for k in range(n)] == want
    # store: put, read_members, and get through the chunk pass
    before = ctx.index_counts()
    st = pmc_codec.Store(ctx, 16 << 20)
    ext, src_rc = st.put(values)
    assert src_rc == [0] * n
    assert st.members(ext, n) == want
    assert st.get(ext, n) == [(0, v) for v in values]
    st.close()
    after = ctx.index_counts()
    indexed = sum(1 for m in want if pmc_codec.index_info(m))
    assert after["completed"] - before["completed"] == indexed - 1 and after["handed_over"] - before["handed_over"] == 1
    # slab: set, then get through the chunk pass
    slab = pmc_codec.Slab(ctx, 32, int(lens.max()))
    b = D.pack(values)
    slots = torch.from_numpy(np.random.default_rng(9).permutation(32)[:n].astype(np.int32)).cuda()
    src_rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    slab.set(b.data, b.off, b.len, slots, src_rc, D.stream_handle())
    torch.cuda.synchronize()
    assert int((src_rc != 0).sum()) == 0
    lens_t = torch.zeros(32, dtype=torch.int32, device="cuda")
    data_t = torch.zeros(slab.stride * 32, dtype=torch.uint8, device="cuda")
    hip = ctypes.CDLL("libamdhip64.so")
    for t, p, nb in ((lens_t, slab.lengths_ptr(), 4 * 32), (data_t, slab.data_ptr(), slab.stride * 32)):
        assert hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(nb), 3) == 0
    sl, ln, data = slots.cpu().numpy(), lens_t.cpu().numpy(), data_t.cpu().numpy().tobytes()
    assert [data[int(s) * slab.stride:int(s) * slab.stride + int(ln[s])] for s in sl] == want
    sdst, sdoff, sdcap = D.slots_for([len(v) for v in values], align=1)
    sdlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    grc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    slab.get(slots, sdst, sdoff, sdcap, sdlen, grc, D.stream_handle())
    torch.cuda.synchronize()
    assert int((grc != 0).sum()) == 0
    assert D.Batch(sdst, sdoff, sdlen, n, 0).host_items() == values
    slab.close()
    end = ctx.index_counts()
    assert end["completed"] - after["completed"] == indexed - 1 and end["handed_over"] - after["handed_over"] == 1
    # a group of two contexts on device 0
    g = ctypes.c_void_p()
    assert L.pmc_group_create((ctypes.c_int * 2)(0, 0), 2, ctypes.byref(g)) == 0
    try:
        assert L.pmc_group_set_index(g, 2) == pmc_codec.E_ARG
        assert L.pmc_group_set_level(g, pmc_codec.LEVEL_FAST_ALL) == 0 and L.pmc_group_set_index(g, 1) == 0
        kh = np.array([L.pmc_key_hash(b"key%d" % i, len(b"key%d" % i)) for i in range(n)], dtype=np.uint64)
        u_soff, u_len, u_cap, u_doff = (soff.astype(np.uint64), lens.astype(np.uint32), caps.astype(np.uint32),
                                        doff.astype(np.uint64))
        out = ctypes.create_string_buffer(int(caps.sum()) + 64)
        glen, grc2 = np.zeros(n, dtype=np.uint32), np.full(n, 7, dtype=np.int32)
        assert L.pmc_group_compress_batch(g, b"".join(values), u_soff.ctypes.data, u_len.ctypes.data, kh.ctypes.data, 128,
                                          n, out, u_doff.ctypes.data, u_cap.ctypes.data, glen.ctypes.data,
                                          grc2.ctypes.data, int(lens.max())) == 0
        assert (grc2 == 0).all()
        assert [out.raw[int(doff[k]):int(doff[k]) + int(glen[k])] for k in range(n)] == want
    finally:
        L.pmc_group_destroy(g)


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def counted(ctx, fn):
    """fn(), and the growth of the context's two index counters over it."""
    a = ctx.index_counts()
    res = fn()
    b = ctx.index_counts()
    return res, (b["completed"] - a["completed"], b["handed_over"] - a["handed_over"])


# A device call in a fresh process with PMC_LATENCY_BATCH=0 (so that a small batch takes the record / lane
# pipeline): members, capacities and max_len come from a pickle, verdicts, lengths, slot bytes and the index
# counters go back in one.  Slots are unaligned, as tests/test_gpu_foreign.py's.
CHILD = r"""
import pickle, sys
sys.path[:0] = [sys.argv[1]]
import conftest  # noqa: F401  (puts the package on sys.path)
import pmc_codec
import torch
from test_gpu_foreign import device_call
job = pickle.load(open(sys.argv[2], "rb"))
ctx = pmc_codec.Context(0)
class C:
    pass
cases = []
for m, cap in zip(job["members"], job["caps"]):
    c = C()
    c.name, c.member, c.cap = "", m, cap
    cases.append(c)
rc, dlen, slots = device_call(ctx, cases, job["max_len"])
res = {"rc": [int(x) for x in rc], "dlen": [int(x) for x in dlen], "slots": [s.tobytes() for s in slots],
       "counts": ctx.index_counts(), "retry": ctx.guard_counts()["inflate_retry"]}
ctx.close()
pickle.dump(res, open(sys.argv[3], "wb"))
"""


def child_call(members, caps, max_len):
    d = tempfile.mkdtemp(prefix="pmc_indexed_")
    job, res = os.path.join(d, "job.pkl"), os.path.join(d, "res.pkl")
    with open(job, "wb") as f:
        pickle.dump({"members": members, "caps": caps, "max_len": max_len}, f)
    env = dict(os.environ, PMC_LATENCY_BATCH="0")
    out = subprocess.run([sys.executable, "-c", CHILD, HERE, job, res], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with open(res, "rb") as f:
        return pickle.load(f)


def test_own_decompress_on_every_route(ctx, vals, members):
    import torch
    import pmc_codec
    from pmc_codec import device as D
    L = pmc_codec.lib()
    big = [(n, v, m) for (n, v), m in zip(vals, members) if len(v) > C]
    cases = [Case(n, m, len(v)) for n, v, m in big]
    assert all(c.rc == 0 and c.out == v for c, (_, v, _) in zip(cases, big))
    want = (len(big) - 1, 1)  # every JSON / periodic member by the chunk pass; the random one handed over
    # at most 4 members per CU: the wave-only route
    assert len(cases) <= 4 * cus()
    _, got = counted(ctx, lambda: check_route(ctx, cases, max(c.cap for c in cases)))
    assert got == want, got
    # more than 4 members per CU, padded with small members: the record / lane pipeline
    pad_to = max(PIPELINE_N, 4 * cus() + 8)
    grew, got = counted(ctx, lambda: check_route(ctx, cases, max(c.cap for c in cases), pad_to))
    assert got == want and grew == 1, (got, grew)  # (only the random member reached the wave kernels)
    # the pipeline again, for the small batch: a fresh process with PMC_LATENCY_BATCH=0
    small = [c for c in cases if c.name != BIG_NAME]
    r = child_call([c.member for c in small], [c.cap for c in small], max(c.cap for c in small))
    assert r["rc"] == [0] * len(small) and [s[:n] for s, n in zip(r["slots"], r["dlen"])] == [c.out for c in small]
    assert r["counts"] == {"completed": len(small) - 1, "handed_over": 1} and r["retry"] == 1, r["counts"]
    # host batch: the throughput pipeline (capacities above the latency path's 48 KiB) ...
    res, got = counted(ctx, lambda: ctx.decompress_many([c.member for c in small]))
    assert res == [(0, c.out) for c in small] and got == (len(small) - 1, 1), got
    # ... and the latency path, the wave kernel over host memory (<= 48 KiB each)
    low = [c for c in small if c.cap <= 48 * 1024]
    assert len(low) >= 2
    before = ctx.path_counts()["latency_decompress"]
    res, got = counted(ctx, lambda: ctx.decompress_many([c.member for c in low]))
    assert ctx.path_counts()["latency_decompress"] == before + 1
    assert res == [(0, c.out) for c in low] and got == (len(low), 0), got
    # single value
    def single():
        for c in small[::4]:
            out = ctypes.create_string_buffer(c.cap)
            olen = ctypes.c_size_t(0)
            assert L.pmc_gzip_decompress(ctx.handle, c.member, len(c.member), out, c.cap, ctypes.byref(olen)) == 0
            assert out.raw[:olen.value] == c.out
    _, got = counted(ctx, single)
    assert got == (sum(1 for c in small[::4] if c.name != RANDOM_NAME), sum(1 for c in small[::4] if c.name == RANDOM_NAME))
    # pinned, pipelined in chunks of 4
    n = len(small)
    lens = np.array([len(c.member) for c in small], dtype=np.int64)
    caps = np.array([c.cap for c in small], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
    doff = np.concatenate([[0], np.cumsum(caps + 3)[:-1]]) + 1
    pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
    src = torch.frombuffer(bytearray(b"".join(c.member for c in small) + bytes(64)), dtype=torch.uint8).pin_memory()
    dst = torch.zeros(int((caps + 3).sum()) + 64, dtype=torch.uint8).pin_memory()
    dlen, rc = torch.zeros(n, dtype=torch.int32).pin_memory(), torch.full((n,), 7, dtype=torch.int32).pin_memory()
    _, got = counted(ctx, lambda: ctx.decompress_pinned(src, pin(soff, np.int64), pin(lens, np.int32), dst,
                                                        pin(doff, np.int64), pin(caps, np.int32), dlen, rc,
                                                        int(caps.max()), 4))
    assert (rc.numpy() == 0).all() and got == (n - 1, 1), got
    raw = dst.numpy().tobytes()
    assert [raw[int(doff[k]):int(doff[k]) + int(dlen[k])] for k in range(n)] == [c.out for c in small]
    # a call with max_len <= C moves neither counter, whatever its members
    tiny = [Case(n, m, len(v)) for (n, v), m in zip(vals, members) if len(v) <= C]
    z = zlib.compressobj(6, zlib.DEFLATED, 31)
    tiny.append(Case("zlib", z.compress(PAD_VALUE) + z.flush(), len(PAD_VALUE)))
    for pad in (0, pad_to):
        _, got = counted(ctx, lambda: check_route(ctx, tiny, C, pad))
        assert got == (0, 0), got
    # (store get and slab get: test_deterministic_across_batches_positions_and_entry_points)


def corruptions(m):
    """[(name, bytes)]: every single-entry corruption of m's index, then seeded byte mutations."""
    cb, k, offs, hdr = parse_index(m)
    assert k >= 3

    def put(at, b):
        return m[:at] + bytes(b) + m[at + len(b):]

    def u32(x):
        return int(x).to_bytes(4, "little")

    out = [("off+1", put(20, u32(offs[0] + 1))), ("off-1", put(20, u32(offs[0] - 1))),
           ("last_off+1", put(20 + 4 * (k - 2), u32(offs[-1] + 1))), ("last_off-1", put(20 + 4 * (k - 2), u32(offs[-1] - 1))),
           ("swapped", put(20, u32(offs[1]) + u32(offs[0]))), ("off0", put(24, u32(0))),
           ("off_beyond", put(24, u32(len(m) + 5))), ("off_in_trailer", put(20 + 4 * (k - 2), u32(len(m) - 8))),
           ("off_other_block", put(24, u32(offs[1] + 4000))),
           # K off by one through a changed LEN (XLEN kept, and XLEN moved with it: the header's end moves)
           ("len-4", put(14, (4 + 4 * (k - 2)).to_bytes(2, "little"))), ("len+4", put(14, (4 + 4 * k).to_bytes(2, "little"))),
           ("xlen-4", put(10, (8 + 4 * (k - 2)).to_bytes(2, "little") + m[12:14] + (4 + 4 * (k - 2)).to_bytes(2, "little"))),
           ("log2c-1", put(17, [LOG2C - 1])), ("log2c+1", put(17, [LOG2C + 1])), ("log2c_11", put(17, [11])),
           ("version2", put(16, [2])), ("id", put(12, b"XI")), ("reserved", put(18, [7])),
           ("flg_name", put(3, [12])), ("flg_0", put(3, [0]))]
    rng = np.random.default_rng(len(m))
    for j in range(200):
        at = int(rng.integers(0, hdr + 64)) if j % 2 else int(rng.integers(0, len(m)))
        out.append((f"mut{j}@{at}", put(at, [m[at] ^ int(rng.integers(1, 256))])))
    out += [("truncated", m[:len(m) - 9]), ("truncated_in_index", m[:22]), ("trailing", m + b"trailing bytes"),
            ("crc", put(len(m) - 8, [m[-8] ^ 1]))]
    return out


@pytest.fixture(scope="module")
def damaged(vals, members):
    """Cases of two indexed members: each corruption at the value's size, and each member once at a capacity
    one below ISIZE.  Checked here on the CPU: the oracle and zlib agree on every string."""
    by = {n: (v, m) for (n, v), m in zip(vals, members)}
    cases, index_only = [], []
    for name in (f"json{2 * C + 3}", "json100000"):
        v, m = by[name]
        for cname, b in corruptions(m):
            c = Case(f"{name}:{cname}", b, len(v))
            d = zlib.decompressobj(31)
            try:
                z = d.decompress(b)
                z_ok = d.eof
            except zlib.error:
                z, z_ok = b"", False
            assert (c.rc == 0) == z_ok and (not z_ok or c.out == z), (c.name, c.rc, z_ok)
            cases.append(c)
            if (b[12 + int.from_bytes(b[10:12], "little"):] == m[header_len(len(v)):] and b[:4] == m[:4]
                    and len(b) == len(m)):
                index_only.append(c)  # only header bytes differ, and the header keeps its length
        cases.append(Case(f"{name}:cap-1", m, len(v) - 1))
    # the index is advisory: a member with only its index damaged still decodes to the value
    assert len(index_only) >= 30 and all(c.rc == 0 and c.out == by[c.name.split(":")[0]][0] for c in index_only)
    return cases


def test_corrupt_and_foreign_indexes(ctx, damaged, vals, members):
    """rc and output equal the oracle's for every damaged string on the wave-only route, the pipeline, the
    pipeline of a small batch (fresh process) and the host calls."""
    import pmc_codec
    assert len(damaged) > 400
    max_len = max(c.cap for c in damaged)
    step = 4 * cus()
    for a in range(0, len(damaged), step):
        check_route(ctx, damaged[a:a + step], max_len)
    check_route(ctx, damaged, max_len, max(PIPELINE_N, 4 * cus() + 8))
    part = damaged
    r = child_call([c.member for c in part], [c.cap for c in part], max_len)
    bad = [(c.name, r["rc"][k], c.rc) for k, c in enumerate(part)
           if r["rc"][k] != c.rc or (c.rc == 0 and r["slots"][k][:r["dlen"][k]] != c.out)]
    assert not bad, (len(bad), bad[:8])
    res = ctx.decompress_many([c.member for c in damaged], [c.cap for c in damaged])
    bad = [(c.name, g[0], c.rc) for c, g in zip(damaged, res) if g[0] != c.rc or (c.rc == 0 and g[1] != c.out)]
    assert not bad, (len(bad), bad[:8])
    # pinned, pipelined in chunks of 64, slots unaligned and apart
    import torch
    n = len(damaged)
    lens = np.array([len(c.member) for c in damaged], dtype=np.int64)
    caps = np.array([c.cap for c in damaged], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
    doff = np.concatenate([[0], np.cumsum(caps + 3)[:-1]]) + 1
    pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
    src = torch.frombuffer(bytearray(b"".join(c.member for c in damaged) + bytes(64)), dtype=torch.uint8).pin_memory()
    dst = torch.zeros(int((caps + 3).sum()) + 64, dtype=torch.uint8).pin_memory()
    dlen, rc = torch.zeros(n, dtype=torch.int32).pin_memory(), torch.full((n,), 7, dtype=torch.int32).pin_memory()
    ctx.decompress_pinned(src, pin(soff, np.int64), pin(lens, np.int32), dst, pin(doff, np.int64), pin(caps, np.int32),
                          dlen, rc, int(caps.max()), 64)
    raw, prc, plen = dst.numpy().tobytes(), rc.numpy(), dlen.numpy()
    bad = [(c.name, int(prc[k]), c.rc) for k, c in enumerate(damaged)
           if prc[k] != c.rc or (c.rc == 0 and raw[int(doff[k]):int(doff[k]) + int(plen[k])] != c.out)]
    assert not bad, (len(bad), bad[:8])
    # single values
    L = pmc_codec.lib()
    for c in damaged:
        out = ctypes.create_string_buffer(max(c.cap, 1))
        olen = ctypes.c_size_t(0)
        got = L.pmc_gzip_decompress(ctx.handle, c.member, len(c.member), out, c.cap, ctypes.byref(olen))
        assert got == c.rc and (c.rc != 0 or out.raw[:olen.value] == c.out), (c.name, got, c.rc)
    # a foreign index: the same layout with chunks of 4 KiB in fixed blocks, put together on the CPU -- the chunk
    # pass takes it; with a match that reaches before its chunk (the unchunked parse) it hands the member over
    from fast_large_model import fast_large_tokens
    from indexed_model import assemble
    v = dict(vals)[f"json{C + 1}"]
    good = assemble(v, chunk=4096)
    whole = fast_large_tokens(v)
    cut, p = [[]], 0
    for t in whole:  # the unchunked tokens, cut where they happen to end on a multiple of 4 KiB (else later)
        cut[-1].append(t)
        p += t[0] if isinstance(t, tuple) else 1
        if p % 4096 == 0 and p < len(v):
            cut.append([])
    assert len(cut) == -(-len(v) // 4096)  # (matches end at the 2 KiB segment ends)
    it = iter(cut)
    reaching = assemble(v, chunk=4096, tokens_of=lambda part: next(it))
    assert zlib.decompress(good, 31) == v and zlib.decompress(reaching, 31) == v
    assert pmc_codec.index_info(good) == pmc_codec.index_info(reaching) == (4096, 9)
    for m, want in ((good, (1, 0)), (reaching, (0, 1))):
        _, got = counted(ctx, lambda: check_route(ctx, [Case("foreign", m, len(v))], C + 1))
        assert got == want, got


GUARD_CHILD = r"""
import base64, json, sys
sys.path[:0] = [sys.argv[1]]
from conftest import Golden
from indexed_values import indexed_values
import pmc_codec
from pmc_codec import device as D
import torch
names = sys.argv[2].split(",")
by = dict(indexed_values(Golden().corpus))
vals = [by[n] for n in names]
ctx = pmc_codec.Context(0)
ctx.level = pmc_codec.LEVEL_FAST_ALL
ctx.index = True
out, rc = D.compress(ctx, D.pack(vals, align=1))
torch.cuda.synchronize()
res = {"rc": [int(x) for x in rc.cpu().numpy()], "members": [base64.b64encode(m).decode() for m in out.host_items()],
       "guards": ctx.guard_counts()}
ctx.close()
print(json.dumps(res))
"""


def test_guard_fallback_gives_level_9_bytes_without_an_index(ctx, vals, members):
    """libpmc_codec_fault.so reverses the sort's lanes for the odd batch indices: such a value fails the
    guard and the retry kernel redoes it at level 9 -- FLG 0, no index."""
    import pmc_codec
    if not os.path.exists(os.path.join(PKG, "libpmc_codec_fault.so")):
        pytest.fail("libpmc_codec_fault.so missing: run make -C poor-man-s-cache_amd")
    names = [f"json{C + 1}", f"json{2 * C + 3}", "json100000", f"json{4 * C}", "across", f"json{3 * C - 1}"]
    by = {n: (v, m) for (n, v), m in zip(vals, members)}
    values = [by[n][0] for n in names]
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        exact = device_compress(ctx, values)
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
    env = dict(os.environ, PMC_LIB="libpmc_codec_fault.so")
    out = subprocess.run([sys.executable, "-c", GUARD_CHILD, HERE, ",".join(names)], env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    got = [base64.b64decode(m) for m in r["members"]]
    assert r["rc"] == [0] * len(names), r["rc"]
    assert [zlib.decompress(m, 31) for m in got] == values
    assert got[1::2] == exact[1::2] and all(m[3] == 0 and m[8] == 2 for m in got[1::2])
    assert got[0::2] == [by[n][1] for n in names[0::2]]  # (the even ones: the same indexed members)
    assert r["guards"]["sort"] > 0, r["guards"]

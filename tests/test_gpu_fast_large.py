"""GPU: the fast level for values of every size (PMC_LEVEL_FAST_ALL, include/pmc_codec.h "compression
level").

A value above 16382 bytes becomes a segmented fast member: one valid gzip member of 16383-symbol blocks (header bytes
4..7 = 0, byte 8 = 4, within pmc_gzip_bound) whose tokens are tests/fast_large_model.py's; it is the same
member whatever entry point, batch or batch position produced it; the library's own decompress takes it;
values of up to 16382 bytes are PMC_LEVEL_FAST's members byte for byte; the other two levels are untouched;
on 24 seeded 64 KiB JSON slices the members are no larger in total than zlib level 1's
(tests/golden/fast_large_baseline.json); and under the lane-order fault build the values whose sort the guard
refuses come out as level-9 bytes.

(The listed lengths of at most 16382 bytes -- G + H always -- are plain single-block fast members at this
level, so their tokens are compared with tests/fast_model.py's.)"""
import base64
import ctypes
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from deflate_dissect import dissect
from fast_large_model import G, H, fast_large_tokens
from fast_large_values import BASELINE_COUNT, BASELINE_SIZE, BIG_NAME, M, large_values
from fast_model import FAST_MAX, fast_tokens
from fast_values import edge_values, json_slices

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PKG = os.path.join(os.path.dirname(HERE), "poor-man-s-cache_amd", "pmc_codec")
HDR = b"\x1f\x8b\x08\x00"


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    c.level = pmc_codec.LEVEL_FAST_ALL
    assert c.level == pmc_codec.LEVEL_FAST_ALL == 2
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
def large(golden):
    return large_values(golden.corpus)


@pytest.fixture(scope="module")
def members(ctx, large):
    """The whole value list as one device batch at PMC_LEVEL_FAST_ALL (computed once)."""
    return device_compress(ctx, [v for _, v in large])


def test_spec_parity(ctx, large, members):
    import pmc_codec
    stored_in, nblocks = [], {}
    for (name, v), m in zip(large, members):
        assert m[:4] == HDR and m[4:8] == bytes(4) and m[8] == 4, name
        assert len(m) <= pmc_codec.gzip_bound(len(v)), name
        assert zlib.decompress(m, 31) == v, name
        if name == BIG_NAME:
            continue
        blocks = dissect(m)
        nblocks[name] = len(blocks)
        if any(b["type"] == 0 for b in blocks):
            stored_in.append(name)
            continue
        got = [t for b in blocks for t in b["tokens"]]
        want = fast_large_tokens(v) if len(v) > FAST_MAX else fast_tokens(v)
        if got != want:
            k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
            raise AssertionError(f"{name}: tokens differ at #{k}: {got[k:k + 3]} vs {want[k:k + 3]}")
    assert set(stored_in) <= {"random40000"}, stored_in  # (every JSON and periodic value was compared)
    # a block holds 16383 symbols: 40000 random bytes need three, a value on the small path has one
    assert nblocks["random40000"] == 3 and nblocks[f"json{G + H}"] == 1, nblocks
    assert ctx.guard_counts()["sort"] == 0


def test_own_decompress_takes_segmented_members(ctx, large, members):
    import torch
    from pmc_codec import device as D
    back, rc = D.decompress(ctx, D.pack(members, align=1), [len(v) for _, v in large])
    torch.cuda.synchronize()
    assert int((rc != 0).sum()) == 0, rc
    assert back.host_items() == [v for _, v in large]


def test_deterministic_across_batches_positions_and_entry_points(ctx, large, members):
    import torch
    import pmc_codec
    L = pmc_codec.lib()
    vals = [v for _, v in large]
    perm = np.random.default_rng(5).permutation(len(vals))[:len(vals) - 4]
    assert device_compress(ctx, [vals[i] for i in perm]) == [members[i] for i in perm]
    i40 = [n for n, _ in large].index("json40000")
    assert set(device_compress(ctx, [vals[i40]] * 70)) == {members[i40]}
    # the entry points, on everything but the 1 MiB value
    pick = [i for i, (n, _) in enumerate(large) if n != BIG_NAME]
    vals, want = [vals[i] for i in pick], [members[i] for i in pick]
    n = len(vals)
    # host batch
    assert ctx.compress_many(vals) == [(0, m) for m in want]
    # single value
    for v, m in list(zip(vals, want))[::4]:
        out = ctypes.create_string_buffer(pmc_codec.gzip_bound(len(v)))
        olen = ctypes.c_size_t(0)
        assert L.pmc_gzip_compress(ctx.handle, v, len(v), out, len(out), ctypes.byref(olen)) == 0
        assert out.raw[:olen.value] == m
    # pinned, pipelined in chunks of 3
    lens = np.array([len(v) for v in vals], dtype=np.int64)
    caps = np.array([pmc_codec.gzip_bound(int(x)) for x in lens], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
    doff = np.concatenate([[0], np.cumsum(caps)[:-1]])
    pin = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).pin_memory()  # noqa: E731
    src = torch.frombuffer(bytearray(b"".join(vals) + bytes(64)), dtype=torch.uint8).pin_memory()
    dst = torch.zeros(int(caps.sum()) + 64, dtype=torch.uint8).pin_memory()
    dlen, rc = torch.zeros(n, dtype=torch.int32).pin_memory(), torch.full((n,), 7, dtype=torch.int32).pin_memory()
    ctx.compress_pinned(src, pin(soff, np.int64), pin(lens, np.int32), dst, pin(doff, np.int64), pin(caps, np.int32),
                        dlen, rc, int(lens.max()), 3)
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
    # a group of two contexts on device 0
    g = ctypes.c_void_p()
    assert L.pmc_group_create((ctypes.c_int * 2)(0, 0), 2, ctypes.byref(g)) == 0
    try:
        assert L.pmc_group_set_level(g, 3) == pmc_codec.E_ARG
        assert L.pmc_group_set_level(g, pmc_codec.LEVEL_FAST_ALL) == 0
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


def test_mixed_batch_small_values_are_the_fast_level_s(ctx, golden, large, members):
    import pmc_codec
    small = [v for _, v in edge_values(golden.corpus)]
    big = [(v, m) for (n, v), m in zip(large, members) if n != BIG_NAME]
    mixed, where = [], []
    step = len(small) // len(big)
    for k, v in enumerate(small):  # the large values spread among the small ones
        mixed.append(v)
        if k % step == step - 1 and len(where) < len(big):
            where.append(len(mixed))
            mixed.append(big[len(where) - 1][0])
    assert len(where) == len(big)
    got = device_compress(ctx, mixed)
    assert [got[i] for i in where] == [m for _, m in big]
    at = set(where)
    got_small = [m for i, m in enumerate(got) if i not in at]
    try:
        ctx.level = pmc_codec.LEVEL_FAST
        assert got_small == device_compress(ctx, small)
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL


def test_other_levels_are_untouched(ctx, large, members):
    import pmc_codec
    pick = [i for i, (n, v) in enumerate(large) if n != BIG_NAME and len(v) > FAST_MAX]
    vals = [large[i][1] for i in pick]
    try:
        ctx.level = pmc_codec.LEVEL_FAST
        at_fast = device_compress(ctx, vals)
        ctx.level = pmc_codec.LEVEL_EXACT
        at_exact = device_compress(ctx, vals)
        assert at_fast == at_exact and all(m[8] == 2 for m in at_exact)
        assert [zlib.decompress(m, 31) for m in at_exact] == vals
        assert all(a != members[i] for a, i in zip(at_exact, pick))
        with pytest.raises(ValueError):
            ctx.level = 3
        assert ctx.level == pmc_codec.LEVEL_EXACT
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL


def test_total_size_is_at_most_zlib_level_1(ctx, golden):
    """The ratio condition: on the baseline set the segmented fast members sum to at most zlib level 1's total."""
    with open(os.path.join(GOLDEN, "fast_large_baseline.json")) as f:
        b = json.load(f)["set"]
    assert (b["size"], b["count"]) == (BASELINE_SIZE, BASELINE_COUNT) == (65536, 24)
    vals = json_slices(golden.corpus, b["size"], b["count"], b["seed"])
    mem = device_compress(ctx, vals)
    total = sum(map(len, mem))
    print(f"fast-all 64 KiB: {total} B, level 1 {b['level1_total']} ({total / b['level1_total']:.4f}), "
          f"level 9 {b['level9_total']} ({total / b['level9_total']:.4f})")
    assert [zlib.decompress(m, 31) for m in mem[::5]] == vals[::5]
    assert total <= b["level1_total"], (total, b["level1_total"])


CHILD = r"""
import base64, json, sys
sys.path[:0] = [sys.argv[1]]
from conftest import Golden
from fast_large_values import large_values
import pmc_codec
from pmc_codec import device as D
import torch
names = sys.argv[2].split(",")
by = dict(large_values(Golden().corpus))
vals = [by[n] for n in names]
ctx = pmc_codec.Context(0)
ctx.level = pmc_codec.LEVEL_FAST_ALL
out, rc = D.compress(ctx, D.pack(vals, align=1))
torch.cuda.synchronize()
res = {"rc": [int(x) for x in rc.cpu().numpy()], "members": [base64.b64encode(m).decode() for m in out.host_items()],
       "guards": ctx.guard_counts()}
ctx.close()
print(json.dumps(res))
"""


def test_guard_fallback_gives_level_9_bytes(ctx, large, members):
    """libpmc_codec_fault.so reverses the sort's lanes for the odd batch indices: every segment of such a
    value fails the guard, and the retry kernel redoes the value at level 9."""
    import pmc_codec
    if not os.path.exists(os.path.join(PKG, "libpmc_codec_fault.so")):
        pytest.skip("libpmc_codec_fault.so is not built (make -C poor-man-s-cache_amd)")
    # (a50000 sits at an even index: all its positions share one hash, so the fault build's two reversed
    # scatter passes cancel and its sort comes out in order)
    names = ["json16383", f"json{M * G + 1}", "a50000", "json65536", "period", "json40000"]
    by = {n: (v, m) for (n, v), m in zip(large, members)}
    vals = [by[n][0] for n in names]
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        exact = device_compress(ctx, vals)
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
    env = dict(os.environ, PMC_LIB="libpmc_codec_fault.so")
    out = subprocess.run([sys.executable, "-c", CHILD, HERE, ",".join(names)], env=env, capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    got = [base64.b64decode(m) for m in r["members"]]
    assert r["rc"] == [0] * len(names), r["rc"]
    assert [zlib.decompress(m, 31) for m in got] == vals
    assert got[1::2] == exact[1::2] and all(m[8] == 2 for m in got[1::2])
    assert got[0::2] == [by[n][1] for n in names[0::2]]  # (the even ones: the same segmented fast members)
    assert r["guards"]["sort"] > 0, r["guards"]

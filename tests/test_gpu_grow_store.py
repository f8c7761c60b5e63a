"""GPU: pmc_store_append_batch and pmc_store_grow_range_batch (include/pmc_codec.h), the growing writes that always
perform the write.

Extents of indexed members with chunk CRCs go through pmc_gzip_grow_range_batch over the heap (the chunk path: their
new members equal a fresh put's); small values and level-9 members are read whole into a zeroed value of the new
length, patched and compressed again at the context's switches (the full path) -- so a value that grows past one
chunk becomes indexed.  New extents are allocated before the old ones are released."""
import numpy as np
import pytest

from fast_large_values import BIG_NAME
from grow_model import grown
from indexed_model import C
from indexed_values import indexed_values
from test_gpu_patch_store import extents, fields

pytestmark = pytest.mark.gpu

MAX_VALUE = 536870912  # the server's MAX_REQUEST_SIZE


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    c.level = pmc_codec.LEVEL_FAST_ALL
    c.index = True
    c.index_crc = True
    yield c
    c.close()


@pytest.fixture(scope="module")
def by(golden):
    return dict(indexed_values(golden.corpus))


def txt(seed, n):
    return np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8).tobytes()


def mixed_store(ctx, golden, by):
    """(store, extents, values): an indexed 100000-byte value, the 1 MiB value, a 1000-byte value, a value of C - 10
    bytes, and a value put at level 9."""
    import pmc_codec
    tiled = golden.corpus * 2
    values = [by["json100000"], by[BIG_NAME], tiled[500:1500], tiled[900:900 + C - 10], by[f"json{3 * C - 1}"]]
    st = pmc_codec.Store(ctx, 64 << 20)
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        e9, rc9 = st.put(values[4:])
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        e, rc = st.put(values[:4])
        assert rc + rc9 == [0] * 5
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
    ext = extents(*e, e9[0])
    assert pmc_codec.index_info(st.members(ext, 5)[4]) is None  # the level-9 member
    return st, ext, values


def check_mixed(ctx, st, ext, values, patches, write):
    """write(ext) performs the patches = [(off, bytes)]: get returns the grown values, the members are a fresh
    put's, raw_len is the new length, and the chunk path served exactly the two indexed extents."""
    import pmc_codec
    n = len(values)
    old = [fields(ext[i]) for i in range(n)]
    want = [grown(v, off, p) for v, (off, p) in zip(values, patches)]
    a = ctx.rewrite_counts()
    rcs = write(ext)
    b = ctx.rewrite_counts()
    assert rcs == [0] * n, rcs
    # the device call saw the extents of more than one chunk: two served, the level-9 member declined at the scan
    assert (b["served"] - a["served"], b["declined"] - a["declined"]) == (2, 1), (a, b)
    assert st.get(ext, n) == [(0, w) for w in want]
    assert all(ext[i].flags == 1 and ext[i].raw_len == len(want[i]) for i in range(n))
    assert all(fields(ext[i])[0] != old[i][0] for i in range(n))
    st2 = pmc_codec.Store(ctx, 64 << 20)
    try:
        fresh, rc = st2.put(want)
        assert rc == [0] * n and st.members(ext, n) == st2.members(fresh, n)
    finally:
        st2.close()
    assert st.stats()["used"] == sum(ext[i].cap for i in range(n))
    return b["decoded"] - a["decoded"], b["compressed"] - a["compressed"], b["copied"] - a["copied"]


def test_append_takes_both_paths(ctx, golden, by):
    import pmc_codec
    st, ext, values = mixed_store(ctx, golden, by)
    try:
        tails = [txt(1, 64), txt(2, 64), txt(3, 10), txt(4, 100), txt(5, 7)]
        patches = [(len(v), t) for v, t in zip(values, tails)]
        figures = check_mixed(ctx, st, ext, values, patches, lambda e: st.append(e, tails))
        # 100000 bytes: the old last chunk again, 3 copied; 1 MiB: the old last chunk and a new one, 31 copied
        assert figures == (2, 1 + 2, 3 + 31), figures
        # the value of C - 10 bytes grew past one chunk: it is indexed now
        assert pmc_codec.index_info(st.members(ext, 5)[3]) is not None
        # an empty patch is served and changes nothing
        before = [fields(ext[i]) for i in range(5)]
        assert st.append(ext, [b""] * 5) == [0] * 5 and [fields(ext[i]) for i in range(5)] == before
        assert st.grow_range(ext, [(0xFFFFFFFF, b"")] * 5) == [0] * 5 and [fields(ext[i]) for i in range(5)] == before
    finally:
        st.close()


def test_grow_range_takes_both_paths(ctx, golden, by):
    st, ext, values = mixed_store(ctx, golden, by)
    try:
        # behind the end with a gap; across the end; a small value with a gap; past one chunk; inside a level-9 value
        patches = [(len(values[0]) + C + 7, txt(6, 5)), (len(values[1]) - 5, txt(7, 10)), (1200, txt(8, 10)),
                   (C - 50, txt(9, 100)), (len(values[4]) + 1, txt(10, 3))]
        figures = check_mixed(ctx, st, ext, values, patches, lambda e: st.grow_range(e, patches))
        assert figures == (2, 2 + 2, 3 + 31), figures
        # within the value it is set_range
        inside = [(5, b"in"), (C - 1, b"side"), (0, b"x"), (C + 1, b"yz"), (2 * C, b"!")]
        now = [r[1] for r in st.get(ext, 5)]
        assert st.grow_range(ext, inside) == [0] * 5
        assert st.get(ext, 5) == [(0, grown(v, off, p)) for v, (off, p) in zip(now, inside)]
    finally:
        st.close()


def test_heap_too_small_for_old_and_new(ctx, by):
    import pmc_codec
    v = by["json100000"]
    big = pmc_codec.Store(ctx, 8 << 20)
    try:
        e, rc = big.put([v])
        cap = e[0].cap
    finally:
        big.close()
    st = pmc_codec.Store(ctx, cap + 1024)
    try:
        ext, rc = st.put([v])
        assert rc == [0]
        old = fields(ext[0])
        assert st.append(ext, [b"no room for two"], 1) == [pmc_codec.Z_MEM_ERROR]
        assert fields(ext[0]) == old and st.get(ext, 1) == [(0, v)]
        assert st.grow_range(ext, [(len(v) + 100, b"nor here")], 1) == [pmc_codec.Z_MEM_ERROR]
        assert fields(ext[0]) == old and st.get(ext, 1) == [(0, v)]
        assert st.stats()["used"] == cap
    finally:
        st.close()


def test_bad_requests_leave_the_extents_alone(ctx, by):
    import pmc_codec
    v, w = by["json100000"], by[f"json{2 * C + 3}"]
    st = pmc_codec.Store(ctx, 8 << 20)
    try:
        ext, rc = st.put([v, w, v[:500]])
        assert rc == [0] * 3
        gone = extents(ext[2])
        st.free(gone, 1)
        empty = pmc_codec.Extent()
        arr = extents(ext[0], ext[1], ext[0], gone[0], empty, ext[1])
        old = [fields(arr[i]) for i in range(6)]
        assert st.append(arr, [b"dup"] * 6) == [pmc_codec.E_ARG] * 6 and [fields(arr[i]) for i in range(6)] == old
        rcs = st.grow_range(arr, [(len(v), b"dup"), (5, b"dup"), (C, b"dup"), (0, b"x"), (0, b"x"),
                                  (len(w) + 9, b"dup")])
        assert rcs == [pmc_codec.E_ARG] * 6 and [fields(arr[i]) for i in range(6)] == old
        # longer than the server takes: refused, and one byte less is not the test's to allocate; a write that ends
        # on the limit's far side by one byte, a 32-bit wrap, and beside them a served append
        arr = extents(ext[0], ext[1])
        rcs = st.grow_range(arr, [(MAX_VALUE, b"x"), (0xFFFFFFFF, b"ab")])
        assert rcs == [pmc_codec.E_ARG] * 2 and st.get(arr, 2) == [(0, v), (0, w)]
        rcs = st.grow_range(arr, [(len(v), b"abc"), (MAX_VALUE - 1, b"ab")])
        assert rcs == [0, pmc_codec.E_ARG]
        assert st.get(arr, 2) == [(0, v + b"abc"), (0, w)]
        # pmc_store_set_range_batch keeps refusing growth
        assert st.set_range(arr, [(len(v) + 3, b"x"), (len(w) - 1, b"ab")]) == [pmc_codec.E_ARG] * 2
        assert st.get(arr, 2) == [(0, v + b"abc"), (0, w)]
    finally:
        st.close()

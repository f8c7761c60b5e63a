"""GPU: pmc_store_set_range_batch (include/pmc_codec.h), the ranged write that always performs the write.

Extents of indexed members with chunk CRCs go through pmc_gzip_rewrite_range_batch over the heap (the chunk path:
their new members equal a fresh put's); small values, level-9 members and chunks of stored blocks are read whole,
patched and compressed again (the full path).  New extents are allocated before the old ones are released: a heap
with no room for both fails the request with PMC_Z_MEM_ERROR and leaves the old extent readable."""
import numpy as np
import pytest

from indexed_model import C
from indexed_values import RANDOM_NAME, indexed_values

pytestmark = pytest.mark.gpu


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


def extents(*es):
    import pmc_codec
    arr = (pmc_codec.Extent * len(es))()
    for i, e in enumerate(es):
        arr[i] = e
    return arr


def fields(e):
    return (e.off, e.cap, e.len, e.raw_len, e.flags)


def patched(v, off, p):
    return v[:off] + p + v[off + len(p):]


def test_mixed_batch_takes_both_paths(ctx, golden, by):
    import pmc_codec
    names = ["json100000", f"json{2 * C + 3}", "a_run", f"json{4 * C}"]
    indexed = [by[n] for n in names]
    small = [(golden.corpus * 2)[500:500 + 1024], (golden.corpus * 2)[900:900 + 20000]]
    nine = by[f"json{3 * C - 1}"]
    rnd = by[RANDOM_NAME]
    values = indexed + small + [nine, rnd]
    st = pmc_codec.Store(ctx, 64 << 20)
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        e9, rc = st.put([nine])  # a level-9 member, put before the level was raised
        assert rc == [0]
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ei, rc = st.put(indexed)
        es, rc2 = st.put(small)
        er, rc3 = st.put([rnd])
        assert rc + rc2 + rc3 == [0] * 7
        ext = extents(*ei, *es, e9[0], er[0])
        n = len(values)
        old = [fields(ext[i]) for i in range(n)]
        old_members = st.members(ext, n)
        assert old_members[6][8] == 2 and pmc_codec.index_info(old_members[6]) is None  # the level-9 member
        rng = np.random.default_rng(41)
        txt = lambda k: rng.integers(97, 123, k, dtype=np.uint8).tobytes()
        patches = [(C + 9000, txt(64)), (2 * C - 3, txt(6)), (C - 10, txt(40)), (C, txt(C)),  # the chunk path
                   (100, txt(50)), (19990, txt(10)), (3 * C - 41, txt(40)),                  # small values, level 9
                   (10, b"edge of stored blocks")]                                           # declined: the full path
        want = [patched(v, off, p) for v, (off, p) in zip(values, patches)]
        a = ctx.rewrite_counts()
        rcs = st.set_range(ext, patches)
        b = ctx.rewrite_counts()
        assert rcs == [0] * n, rcs
        # the device call saw the four indexed extents, the level-9 member and the incompressible one
        assert (b["served"] - a["served"], b["declined"] - a["declined"]) == (4, 2)
        assert b["decoded"] - a["decoded"] == 1 + 1 + 2 + 0 + 1
        assert st.get(ext, n) == [(0, w) for w in want]
        assert all(ext[i].flags == 1 and ext[i].raw_len == len(values[i]) for i in range(n))
        assert all(fields(ext[i])[0] != old[i][0] for i in range(n))
        st2 = pmc_codec.Store(ctx, 64 << 20)
        try:
            fresh, rc = st2.put(want[:4])
            assert rc == [0] * 4 and st.members(ext, n)[:4] == st2.members(fresh, 4)
        finally:
            st2.close()
        assert st.stats()["used"] == sum(ext[i].cap for i in range(n))
        # the old extents are on the free lists: a put of the same values takes them, and no new heap
        reserved = st.stats()["reserved"]
        again, rc = st.put(indexed)
        assert rc == [0] * 4 and st.stats()["reserved"] == reserved
        assert sorted(e.off for e in again) == sorted(o[0] for o in old[:4])
        # an empty patch is served and changes nothing
        before = [fields(ext[i]) for i in range(n)]
        assert st.set_range(ext, [(5, b"")] * n) == [0] * n and [fields(ext[i]) for i in range(n)] == before
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
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
        assert st.set_range(ext, [(C + 5, b"no room for two")], 1) == [pmc_codec.Z_MEM_ERROR]
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
        rcs = st.set_range(arr, [(5, b"dup"), (5, b"dup"), (C, b"dup"), (0, b"x"), (0, b"x"), (9, b"dup")])
        assert rcs == [pmc_codec.E_ARG] * 6 and [fields(arr[i]) for i in range(6)] == old
        # out of bounds: no growth, no wrap; a patch that ends at the value's end is served beside them
        arr = extents(ext[0], ext[1])
        rcs = st.set_range(arr, [(len(v) - 2, b"abc"), (0xFFFFFFFF, b"ab")])
        assert rcs == [pmc_codec.E_ARG] * 2 and st.get(arr, 2) == [(0, v), (0, w)]
        rcs = st.set_range(arr, [(len(v) - 3, b"abc"), (len(w), b"a")])
        assert rcs == [0, pmc_codec.E_ARG]
        assert st.get(arr, 2) == [(0, v[:-3] + b"abc"), (0, w)]
    finally:
        st.close()

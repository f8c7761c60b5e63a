"""GPU: the two-round fallback of the store's ranged calls (pmc_store_get_range_batch, pmc_store_set_range_batch).

Both calls read the members the chunk path declines whole, in rounds of at most kRangeFallbackBudget = 64 MiB of
16-byte-rounded raw values.  At the fast-all level with the index switched off no member carries an index, so the
ranged calls decline every one of them: 64 values of exactly 1 MiB fill the budget and the 65th opens a second
round.  Expected bytes are Python slices of the values with Python framing; the store is never asked for its own
expectation."""
import pytest

import store_model as M

pytestmark = pytest.mark.gpu

N = 65
VLEN = 1 << 20
BUDGET = 64 << 20


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    c.level = pmc_codec.LEVEL_FAST_ALL
    c.index = False
    yield c
    c.close()


def values(corpus):
    tiled = corpus * (VLEN // len(corpus) + 2)
    vals = [tiled[1009 * i:1009 * i + VLEN] for i in range(N)]
    assert all(len(v) == VLEN for v in vals) and len(set(vals)) == N
    return vals


def test_two_fallback_rounds(ctx, golden):
    import pmc_codec
    vals = values(golden.corpus)
    # 64 values fill the budget exactly, the 65th does not fit
    assert 64 * M.round16(VLEN) == BUDGET and N == 65
    st = pmc_codec.Store(ctx, 256 << 20)
    try:
        ext, rc = st.put(vals)
        assert rc == [0] * N
        assert all(pmc_codec.index_info(m) is None for m in st.members(ext, N))
        # one ranged get: a range inside the value, one that reaches past its end, the whole value
        ranges = [(1000 + 4099 * i, 5000 + i) if i % 3 == 0 else (VLEN - 100 - i, 4096) if i % 3 == 1 else (0, VLEN)
                  for i in range(N)]
        a = ctx.range_counts()
        got = st.get_range(ext, ranges, N, pmc_codec.FRAME_RESP)
        b = ctx.range_counts()
        print("range counts", {k: b[k] - a[k] for k in b})
        want = [(0, M.wrap(2, v[o:o + n])) for v, (o, n) in zip(vals, ranges)]
        assert [w[1][:w[1].index(b"\n") + 1] for w in want[:3]] == [b"$5000\r\n", b"$101\r\n", b"$1048576\r\n"]
        assert (b["served"] - a["served"], b["declined"] - a["declined"]) == (0, N)  # every member read whole
        bad = [(i, got[i][0], len(got[i][1]), len(want[i][1])) for i in range(N) if got[i] != want[i]]
        assert not bad, bad[:8]
        # one ranged set: 64-byte patches at distinct offsets
        patches = [(7 + 16001 * i, bytes([65 + (i + j) % 26 for j in range(64)])) for i in range(N)]
        assert len({o for o, _ in patches}) == N and all(o + 64 <= VLEN for o, _ in patches)
        old = [(ext[i].off, ext[i].cap) for i in range(N)]
        ra = ctx.rewrite_counts()
        rcs = st.set_range(ext, patches)
        rb = ctx.rewrite_counts()
        print("rewrite counts", {k: rb[k] - ra[k] for k in rb})
        assert rcs == [0] * N, rcs
        # the chunk path declined every member: all took the full path
        assert (rb["served"] - ra["served"], rb["declined"] - ra["declined"]) == (0, N)
        patched = [v[:o] + p + v[o + 64:] for v, (o, p) in zip(vals, patches)]
        got = st.get(ext, N)
        bad = [(i, got[i][0], len(got[i][1])) for i in range(N) if got[i] != (0, patched[i])]
        assert not bad, bad[:8]
        # the old extents were released: `used` is the new extents' caps, and no new extent is an old one
        assert all(ext[i].flags == 1 and ext[i].raw_len == VLEN for i in range(N))
        assert not {(ext[i].off, ext[i].cap) for i in range(N)} & set(old)
        assert M.disjoint_inside([(ext[i].off, ext[i].cap) for i in range(N)], 256 << 20)
        assert st.stats()["used"] == sum(ext[i].cap for i in range(N))
    finally:
        st.close()

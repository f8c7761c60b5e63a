"""GPU: growing writes of indexed members (include/pmc_codec.h "growing writes").

pmc_gzip_grow_range_batch turns the member of a value V into the member of V' = V with a patch laid at range_off,
which may lie behind V's end (zeros between) or reach past it: the chunks before the first touched one are copied,
the old last chunk is made again as a non-last chunk, the chunks behind it are new.  The oracle is the existing
compress call on V' -- never the code under test: every served member equals it byte for byte, zlib reads it as V',
its entries are V's chunk CRCs, the canaries around its slot stay, and pmc_ctx_rewrite_counts moves by the figures
of tests/grow_model.py."""
import zlib

import numpy as np
import pytest

from fast_large_values import BIG_NAME
from grow_model import MAX_CHUNKS, SAME, SERVE, grow, grow_of, grown
from indexed_crc_model import assemble_crc, chunk_crcs, parse_chunk_crcs
from indexed_model import C, parse_index
from indexed_values import LAST_MATCH_NAME, LAST_MATCH_TEXT, RANDOM_NAME, indexed_values
from range_model import chunk_span
from test_gpu_patch import KEYS, check_served, counted, lib_span_of, rewrite_call
from test_gpu_range import GUARD, device_compress

pytestmark = pytest.mark.gpu


class Grow:
    """The context as test_gpu_patch.rewrite_call sees it, with the growing call in the rewrite call's place."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.rewrite_range_device = ctx.grow_range_device

    def __getattr__(self, name):
        return getattr(self._ctx, name)


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
def vals(golden):
    return indexed_values(golden.corpus)


@pytest.fixture(scope="module")
def members(ctx, vals):
    """The whole value list as one device batch (computed once, never changed)."""
    return device_compress(ctx, [v for _, v in vals])


@pytest.fixture(scope="module")
def by(vals, members):
    return {n: (v, m) for (n, v), m in zip(vals, members)}


def txt(seed, n):
    return np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8).tobytes()


def model_counts(v, off, p):
    """(served, declined, decoded, compressed, copied) of a served request."""
    verdict, _, _, k2, _, _, items, ea, eb = grow_of(len(v), 15, off, len(p))
    assert verdict in (SERVE, SAME)
    return np.array([1, 0, int(ea) + int(eb), items, k2 - items], dtype=np.int64)


def grow_call(ctx, reqs, news, caps=None, seed=1):
    import pmc_codec
    if caps is None:
        caps = [pmc_codec.gzip_bound(len(nv)) for nv in news]
    return rewrite_call(Grow(ctx), reqs, caps=caps, seed=seed)


def check_grown(ctx, cases, seed=1):
    """cases = [(value, member, off, patch)]: every request is served, the new member is the fresh compress of the
    grown value byte for byte, zlib reads it, its entries are the grown value's chunk CRCs, nothing behind it in its
    slot changed, and the counters grew by the model's figures.  Returns the members and the counters' growth."""
    import pmc_codec
    news = [grown(v, off, p) for v, _, off, p in cases]
    fresh = device_compress(ctx, news)
    reqs = [(m, off, p) for _, m, off, p in cases]
    (rc, dlen, slots), got = counted(ctx, lambda: grow_call(ctx, reqs, news, seed=seed))
    want = sum((model_counts(v, off, p) for v, _, off, p in cases), np.zeros(5, dtype=np.int64))
    for i, ((v, m, off, p), nv, f) in enumerate(zip(cases, news, fresh)):
        tag = (i, len(v), off, len(p))
        assert rc[i] == 0 and dlen[i] == len(f), (tag, int(rc[i]), int(dlen[i]), len(f))
        new = slots[i][:len(f)]
        if new != f:
            d = next(j for j in range(len(f)) if new[j] != f[j])
            raise AssertionError((tag, "first difference at byte", d, "of", len(f)))
        assert slots[i][len(f):] == bytes([GUARD]) * (len(slots[i]) - len(f)), tag
        assert zlib.decompress(new, 31) == nv, tag
        assert pmc_codec.index_crc_info(new) == chunk_crcs(nv), tag
    print("cases:", len(cases), "counters", dict(zip(KEYS, got)), "model", want.tolist())
    assert got == tuple(int(x) for x in want), (got, want.tolist())
    return [s[:len(f)] for s, f in zip(slots, fresh)], got


def test_append_behind_a_full_last_chunk(ctx, by):
    """The old last chunk is full: it is decoded, and comes back as a non-last chunk."""
    cases = []
    for name in (f"json{2 * C}", f"json{4 * C}"):
        v, m = by[name]
        cases += [(v, m, len(v), txt(50 + n, n)) for n in (1, 2, 3, C, C + 1)]
    _, got = check_grown(ctx, cases)
    # per request one decode; one new chunk (two for C + 1 bytes) beside the old last one
    assert got == (10, 0, 10, 2 * (2 + 2 + 2 + 2 + 3), 5 * 1 + 5 * 3), got


def test_append_behind_short_last_chunks(ctx, by):
    v, m = by[f"json{3 * C - 1}"]
    cases = [(v, m, len(v), txt(60 + n, n)) for n in (1, 2, C + 1)]  # S' = 3 C; a new 1-byte chunk; S' = 4 C
    v, m = by[f"json{C + 1}"]
    # a 1-byte old last chunk: the parse's 1- and 2-byte tail path before and after
    cases += [(v, m, len(v), txt(70 + n, n)) for n in (1, 2, C - 1, C)]
    _, got = check_grown(ctx, cases)
    assert got == (7, 0, 7, 1 + 2 + 2 + 1 + 1 + 1 + 2, 3 * 2 + 4 * 1), got


def test_json100000(ctx, by):
    v, m = by["json100000"]
    S = len(v)
    assert -(-S // C) == 4
    _, got = check_grown(ctx, [(v, m, S, txt(80, 64))])
    assert got == (1, 0, 1, 1, 3), got
    check_grown(ctx, [(v, m, S - 5, txt(81, 10))])
    # from the last chunk's first byte on: no decode
    _, got = check_grown(ctx, [(v, m, 3 * C, txt(82, S - 3 * C + 9))])
    assert got == (1, 0, 0, 1, 3), got
    _, got = check_grown(ctx, [(v, m, C, txt(83, 3 * C + 100))])
    assert got == (1, 0, 0, 4, 1), got
    # the whole value and more: nothing is copied or decoded
    _, got = check_grown(ctx, [(v, m, 0, txt(84, S + 10))])
    assert got == (1, 0, 0, 4, 0), got
    # zero gaps: one byte, and a whole zero chunk
    _, got = check_grown(ctx, [(v, m, S + 1, b"!"), (v, m, S + 2 * C + 7, b"12345")])
    assert got == (2, 0, 2, 1 + 3, 3 + 3), got
    # all of them in one call, in another order
    check_grown(ctx, [(v, m, S + 2 * C + 7, b"12345"), (v, m, 0, txt(84, S + 10)), (v, m, S, txt(80, 64)),
                      (v, m, C, txt(83, 3 * C + 100)), (v, m, S - 5, txt(81, 10)), (v, m, S + 1, b"!"),
                      (v, m, 3 * C, txt(82, S - 3 * C + 9))], seed=5)


def test_last_match_cut_match_and_runs(ctx, by):
    v, m = by[LAST_MATCH_NAME]
    assert len(v) == C + LAST_MATCH_TEXT + 40
    # the old final block of 16383 symbols is no longer the value's end
    cases = [(v, m, len(v), b"!"), (v, m, C, v[C:] + txt(90, 40))]
    for name in ("across", "a_run"):
        w, mw = by[name]
        cases.append((w, mw, len(w), txt(91, 300)))
    check_grown(ctx, cases)


def declined(ctx, reqs, decoded=0):
    import pmc_codec
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(Grow(ctx), reqs, caps=[4096] * len(reqs)))
    assert list(rc) == [pmc_codec.E_NO_INDEX] * len(reqs) and not dlen.any(), (rc, dlen)
    assert all(s == bytes([GUARD]) * len(s) for s in slots)
    assert got == (0, len(reqs), decoded, 0, 0), got


def test_stored_blocks(ctx, by):
    r, mr = by[RANDOM_NAME]
    assert len(r) == 70000
    # the edge chunk is stored blocks: the chunk decoder declines it
    declined(ctx, [(mr, len(r), b"abc")], decoded=1)
    _, got = check_grown(ctx, [(r, mr, 2 * C, txt(92, len(r) - 2 * C + 100))])
    assert got == (1, 0, 0, 1, 2), got


def test_superset_of_the_rewrite(ctx, by):
    """In-bounds requests of tests/test_gpu_patch.py: the rewrite call's verdicts, bytes and counters."""
    v, m = by["json100000"]
    w, mw = by[f"json{2 * C + 3}"]
    cases = [(v, m, C + 9000, txt(93, 64)), (w, mw, 2 * C - 3, txt(94, 6)), (v, m, C - 5, txt(95, C + 10))]
    check_served(Grow(ctx), cases)
    reqs = [(m, off, p) for _, m, off, p in cases] + [(m, 77, b"")]
    a, ca = counted(ctx, lambda: rewrite_call(ctx, reqs))
    b, cb = counted(ctx, lambda: rewrite_call(Grow(ctx), reqs))
    assert list(a[0]) == list(b[0]) == [0] * 4 and list(a[1]) == list(b[1]) and a[2] == b[2] and ca == cb, (ca, cb)


def test_verdicts_and_capacity(ctx, by):
    import pmc_codec
    v, m = by["json100000"]
    S = len(v)
    # an empty patch copies the member, wherever it points
    reqs = [(m, S + 9, b""), (m, 0xFFFFFFFF, b""), (m, 5, b"")]
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(Grow(ctx), reqs))
    assert list(rc) == [0] * 3 and all(s[:len(m)] == m and int(n) == len(m) for s, n in zip(slots, dlen)), (rc, dlen)
    assert got == (3, 0, 0, 0, 3 * 4), got
    # ... while the rewrite call keeps refusing it behind the end, and growth
    rc, dlen, _ = rewrite_call(ctx, [(m, S + 9, b""), (m, S, b"x"), (m, S - 1, b"xy")])
    assert list(rc) == [pmc_codec.E_ARG] * 3 and not dlen.any()
    # ISIZE would wrap: an argument error, nothing written, nothing counted
    reqs = [(m, 0xFFFFFFFF, b"xy"), (m, 0xFFFFFFFE, b"xyz"), (m, 0xFFFFFFF0, bytes(17))]
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(Grow(ctx), reqs, caps=[4096] * 3))
    assert list(rc) == [pmc_codec.E_ARG] * 3 and not dlen.any() and got == (0, 0, 0, 0, 0), (rc, dlen, got)
    assert all(s == bytes([GUARD]) * len(s) for s in slots)
    # more chunks than a member with chunk CRCs may have: declined, nothing decoded
    assert grow_of(S, 15, MAX_CHUNKS * C - 1, 1)[:4] == (SERVE, True, MAX_CHUNKS * C, MAX_CHUNKS)
    declined(ctx, [(m, MAX_CHUNKS * C, b"x"), (m, MAX_CHUNKS * C - 1, b"xy"), (m, 0xFFFFFFFE, b"x")])
    # capacity: need is served, need - 1 is not, and says how much it needs
    cases = [(v, m, S, b"capacity"), (v, m, S + C, b"?"), (v, m, S + 9, b"")]
    news = [grown(v, off, p) for v, _, off, p in cases]
    fresh = device_compress(ctx, news)
    need = [len(f) for f in fresh]
    assert need[2] == len(m)
    reqs = [(m, off, p) for _, m, off, p in cases]
    rc, dlen, slots = grow_call(ctx, reqs, news, caps=need)
    assert list(rc) == [0] * 3 and [int(x) for x in dlen] == need and slots == fresh
    (rc, dlen, slots), got = counted(ctx, lambda: grow_call(ctx, reqs, news, caps=[x - 1 for x in need]))
    assert list(rc) == [pmc_codec.E_CAPACITY] * 3 and [int(x) for x in dlen] == need, (rc, dlen)
    assert all(s == bytes([GUARD]) * len(s) for s in slots)
    assert got[:2] == (0, 0) and got[3:] == (0, 0), got
    # pmc_gzip_bound(S') always suffices (the default slots of every served case above), and the old value's bound
    # is not asked for: a slot of the old member's length is too small for any append here
    rc, dlen, _ = grow_call(ctx, reqs[:2], news[:2], caps=[0, 19])
    assert list(rc) == [pmc_codec.E_CAPACITY] * 2 and [int(x) for x in dlen] == need[:2]


def test_declined_members(ctx, by):
    import pmc_codec
    v, m = by["json100000"]
    values = [v, by[f"json{2 * C + 3}"][0]]
    try:
        ctx.level = pmc_codec.LEVEL_EXACT
        exact = device_compress(ctx, values)
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index = False
        plain = device_compress(ctx, values)
        ctx.index = True
        ctx.index_crc = False
        nocrc = device_compress(ctx, values)
    finally:
        ctx.level = pmc_codec.LEVEL_FAST_ALL
        ctx.index = True
        ctx.index_crc = True
    assert all(parse_index(x) is not None and parse_chunk_crcs(x) is None for x in nocrc)
    small = device_compress(ctx, [v[:1000], v[:C]])
    lens = [len(values[0]), len(values[1])] * 3 + [1000, C]
    reqs = [(x, n, b"abc") for x, n in zip(exact + plain + nocrc + small, lens)]
    reqs += [(x, n + 9, b"") for x, n in zip(exact + nocrc, lens)]
    reqs += [(b"", 0, b"x"), (m[:40], 0, b"x"), (m[:-1], len(v), b"abc")]
    declined(ctx, reqs)


def test_damage_is_not_laundered(ctx, golden):
    import pmc_codec
    from test_gpu_range_crc import FLIP_SEED, flips_of
    v = (golden.corpus * 4)[100:100 + 2 * C + 3]
    m = assemble_crc(v)
    S = len(v)
    flips, per = flips_of(m, np.random.default_rng(FLIP_SEED))
    assert all(x >= 50 for x in per), per
    p = b"[growing write]"
    nv = grown(v, S, p)
    # the foreign member itself: chunks 0 and 1 verbatim, the old last chunk and header and trailer the library's
    want, figures = grow(m, S, p, lib_span_of(ctx, nv))
    (rc, dlen, slots), got = counted(ctx, lambda: grow_call(ctx, [(m, S, p)], [nv]))
    assert rc[0] == 0 and slots[0][:dlen[0]] == want and got == (1, 0) + figures == (1, 0, 1, 1, 2), (got, figures)
    assert zlib.decompress(want, 31) == nv
    # a flip in chunk 0 with an append: served, the damaged span in the output verbatim, and the full read of the
    # result fails; the same kind of flip in the old last chunk: declined
    first = [b for j, b in flips if j == 0][::25]
    last = [b for j, b in flips if j == 2][::25]
    assert first and last
    reqs = [(b, S, p) for b in first + last]
    (rc, dlen, slots), got = counted(ctx, lambda: grow_call(ctx, reqs, [nv] * len(reqs)))
    assert got == (len(first), len(last), len(reqs), len(first), 2 * len(first)), got
    carried = []
    for i, b in enumerate(first):
        w = grow(b, S, p, lib_span_of(ctx, nv))[0]
        assert isinstance(w, bytes) and rc[i] == 0 and slots[i][:dlen[i]] == w, i
        s0, e0, _, _ = chunk_span(b, 0)
        s1, e1, _, _ = chunk_span(w, 0)
        assert w[s1:e1] == b[s0:e0]
        with pytest.raises(zlib.error):
            zlib.decompress(w, 31)
        carried.append(w)
    for i in range(len(first), len(reqs)):
        assert (rc[i], dlen[i]) == (pmc_codec.E_NO_INDEX, 0), i
    res = ctx.decompress_many(carried, caps=[len(nv)] * len(carried))
    assert [r[0] for r in res] == [pmc_codec.Z_DATA_ERROR] * len(res)
    # a flipped CRC entry is declined at the scan, whichever chunk it belongs to; so is a flipped trailer CRC
    at = 16 + 4 * 3 + 8
    reqs = []
    for j in range(3):
        b = m[:at + 4 * j + 2] + bytes([m[at + 4 * j + 2] ^ 4]) + m[at + 4 * j + 3:]
        reqs += [(b, S, b"ab"), (b, S + C, b"ab"), (b, S + 9, b"")]
    b = m[:-7] + bytes([m[-7] ^ 0x80]) + m[-6:]
    reqs += [(b, S, b"ab"), (b, S + 9, b"")]
    declined(ctx, reqs)


def test_one_mebibyte_value(ctx, by):
    """64 bytes behind the 1 MiB value: one decode, the old last chunk and one new chunk compressed, 31 copied."""
    v, m = by[BIG_NAME]
    assert len(v) == 1 << 20
    _, got = check_grown(ctx, [(v, m, len(v), txt(96, 64))])
    assert got == (1, 0, 1, 2, 31), got


def test_rounds_of_touched_chunks(ctx, by):
    """More touched chunks than one round holds (csrc/pmc_plan.hpp kPatchRoundChunks = 8192): 2100 requests that
    write all five chunks of the grown value, 10,500 touched chunks in two rounds, into slots of the fresh member's
    size."""
    v, m = by["json100000"]
    new = bytes(reversed(v)) + txt(97, C)
    fresh = device_compress(ctx, [new])[0]
    n = 2100
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(Grow(ctx), [(m, 0, new)] * n, caps=[len(fresh)] * n))
    assert not rc.any() and (dlen == len(fresh)).all() and got == (n, 0, 0, 5 * n, 0), got
    assert all(s == fresh for s in slots)


def test_unchanged_ground(ctx, vals, members):
    """After the growing calls above, compress and decompress of the module's values give the bytes from before."""
    assert device_compress(ctx, [v for _, v in vals]) == members
    assert ctx.decompress_many(members) == [(0, v) for _, v in vals]

"""GPU: ranged writes of indexed members (include/pmc_codec.h "ranged writes").

pmc_gzip_rewrite_range_batch turns the member of a value V into the member of V' = V with a byte range replaced,
compressing again only the chunks the patch touches.  For members this library wrote (level fast-all, index and
index_crc on) the new member is byte for byte what a fresh compress of V' gives -- the oracle here is that existing
compress call, not the code under test -- and zlib reads it as V'.  pmc_ctx_rewrite_counts proves which chunks were
decoded, compressed and copied (tests/patch_model.py states the figures).  Every member the contract declines is
declined; damage in an untouched chunk is carried along, never laundered.  Slots lie at unaligned offsets with 16
canary bytes on both sides, and no byte outside a served request's member changes."""
import zlib

import numpy as np
import pytest

from fast_large_values import BIG_NAME
from indexed_crc_model import assemble_crc, chunk_crcs, crc_defects, parse_chunk_crcs
from indexed_model import C, parse_index
from indexed_values import LAST_MATCH_NAME, LAST_MATCH_TEXT, RANDOM_NAME, indexed_values
from patch_model import NO_INDEX, patch_of, rewrite
from range_model import chunk_bytes, chunk_span
from test_gpu_range import CANARY, GUARD, device_compress

pytestmark = pytest.mark.gpu

KEYS = ("served", "declined", "decoded", "compressed", "copied")


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


def isize(m):
    return int.from_bytes(m[-4:], "little") if len(m) >= 4 else 0


def rewrite_call(ctx, reqs, caps=None, seed=1):
    """One device call over reqs = [(member, off, patch)]; requests of the same member (or patch) object alias its
    bytes.  Slot i has caps[i] bytes (default: pmc_gzip_bound of the member's ISIZE), an unaligned offset and
    CANARY guard bytes on both sides.  Asserts that no byte outside the members of the served requests changed;
    returns (rc, dst_len, [slot bytes])."""
    import torch
    import pmc_codec
    from pmc_codec import device as D
    rng = np.random.default_rng(seed)
    n = len(reqs)

    def dedupe(items):
        uniq, where = [], {}
        for x in items:
            if id(x) not in where:
                where[id(x)] = len(uniq)
                uniq.append(x)
        return uniq, np.array([where[id(x)] for x in items], dtype=np.int64)

    um, im = dedupe([r[0] for r in reqs])
    up, ip = dedupe([r[2] for r in reqs])
    bm, bp = D.pack(um, align=1), D.pack(up, align=1)
    im, ip = torch.from_numpy(im).cuda(), torch.from_numpy(ip).cuda()
    soff, slen = bm.off[im].contiguous(), bm.len[im].contiguous()
    poff, plen = bp.off[ip].contiguous(), bp.len[ip].contiguous()
    if caps is None:
        caps = [pmc_codec.gzip_bound(isize(m)) for m, _, _ in reqs]
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
    dlen = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    rc = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.rewrite_range_device(bm.data, soff, slen, bp.data, poff, plen, roff, dst, doff, dcap, dlen, rc, D.stream_handle())
    torch.cuda.synchronize()
    rc, dlen, out = rc.cpu().numpy(), dlen.cpu().numpy().view(np.uint32), dst.cpu().numpy()
    # WRITES: only [dst_off, dst_off + need) of the requests answered PMC_OK
    may = np.zeros(len(out), dtype=bool)
    for i in range(n):
        if rc[i] == 0:
            may[off[i]:off[i] + min(int(dlen[i]), int(caps[i]))] = True
    changed = np.flatnonzero(~may & (out != host0))
    assert len(changed) == 0, f"{len(changed)} bytes outside the served members changed, first at {int(changed[0])}"
    return rc, dlen, [out[off[i]:off[i] + caps[i]].tobytes() for i in range(n)]


def counts(ctx):
    c = ctx.rewrite_counts()
    return np.array([c[k] for k in KEYS], dtype=np.int64)


def counted(ctx, fn):
    a = counts(ctx)
    res = fn()
    return res, tuple(int(x) for x in counts(ctx) - a)


def patched(v, off, p):
    return v[:off] + p + v[off + len(p):]


def model_counts(v, off, p):
    """(served, declined, decoded, compressed, copied) of a served request."""
    k = -(-len(v) // C)
    ok, a, b, items, ea, eb = patch_of(len(v), 15, off, len(p))
    assert ok
    return np.array([1, 0, int(ea) + int(eb), items, k - items], dtype=np.int64)


def check_served(ctx, cases, seed=1):
    """cases = [(value, member, off, patch)]: every request is served, the new member is the fresh compress of the
    patched value byte for byte, zlib reads it, its entries are the patched value's chunk CRCs, nothing behind it
    in its slot changed, and the counters grew by the model's figures."""
    import pmc_codec
    news = [patched(v, off, p) for v, _, off, p in cases]
    fresh = device_compress(ctx, news)
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(ctx, [(m, off, p) for _, m, off, p in cases], seed=seed))
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
    return [s[:len(f)] for s, f in zip(slots, fresh)]


def test_tail_chunks_and_chunk_edges(ctx, by):
    rng = np.random.default_rng(31)
    txt = lambda n: rng.integers(97, 123, n, dtype=np.uint8).tobytes()
    cases = []
    v, m = by[f"json{C + 1}"]
    cases += [(v, m, 100, txt(64)), (v, m, C, b"#"), (v, m, C - 1, b"<>"), (v, m, 0, txt(C))]
    v, m = by[f"json{2 * C}"]
    cases += [(v, m, 2 * C - 70, txt(70)), (v, m, C - 2, txt(4)), (v, m, C, txt(C))]
    v, m = by[f"json{2 * C + 2}"]
    cases += [(v, m, 2 * C, b"xy"), (v, m, 2 * C + 1, b"z"), (v, m, 2 * C - 3, txt(5)), (v, m, 50, txt(7))]
    v, m = by[f"json{2 * C + 3}"]
    cases += [(v, m, 2 * C, b"xyz"), (v, m, 2 * C + 1, b"qq"), (v, m, 2 * C - 3, txt(6)), (v, m, C + 50, txt(7))]
    check_served(ctx, cases)


def test_json100000(ctx, by):
    rng = np.random.default_rng(32)
    v, m = by["json100000"]
    txt = lambda n: rng.integers(97, 123, n, dtype=np.uint8).tobytes()
    check_served(ctx, [(v, m, C + 9000, txt(64))])
    # exactly chunk 1: nothing is decoded
    _, got = counted(ctx, lambda: check_served(ctx, [(v, m, C, txt(C))]))
    assert got == (1, 0, 0, 1, 3), got
    check_served(ctx, [(v, m, C - 5, txt(C + 10))])
    _, got = counted(ctx, lambda: check_served(ctx, [(v, m, 0, txt(len(v)))]))
    assert got == (1, 0, 0, 4, 0), got
    # all of them in one call, in another order
    check_served(ctx, [(v, m, 0, txt(len(v))), (v, m, C - 5, txt(C + 10)), (v, m, C + 9000, txt(64)), (v, m, C, txt(C)),
                       (v, m, 3 * C + 1, txt(len(v) - 3 * C - 1)), (v, m, len(v) - 1, b"}")], seed=5)


def test_cut_match_last_match_and_stored_blocks(ctx, by):
    rng = np.random.default_rng(33)
    cases = []
    v, m = by["across"]
    # the bytes the match that is cut at C was copied from, and the copy itself
    cases += [(v, m, C - 1174, b"?" * 300), (v, m, C - 150, bytes(reversed(v[C - 150:C + 150])))]
    v, m = by[LAST_MATCH_NAME]
    assert len(v) == C + LAST_MATCH_TEXT + 40
    # chunk 0 only: the last chunk's 16383-symbol final block is copied; the last chunk with the same text: the
    # emit reproduces "no empty block after the 16383rd symbol"
    cases += [(v, m, 20, b"[patched]"), (v, m, C, v[C:]), (v, m, C + 1, v[C + 1:len(v) - 1])]
    v, m = by["a_run"]
    noise = rng.integers(0, 256, C, dtype=np.uint8).tobytes()
    cases += [(v, m, C, noise), (v, m, 100, noise[:20000]), (v, m, C - 10, noise[:20])]
    v, m = by[f"json{4 * C}"]
    cases += [(v, m, C, bytes(C)), (v, m, 2 * C + 77, bytes(9000))]
    outs = check_served(ctx, cases)
    assert outs[3] == by[LAST_MATCH_NAME][1] and outs[4] == by[LAST_MATCH_NAME][1]
    # the incompressible chunk came out as stored blocks
    start, nxt, _, _ = chunk_span(outs[5], 1)
    assert nxt - start > C


def test_same_bytes_same_member_any_position(ctx, by):
    v, m = by["json100000"]
    w, mw = by[f"json{2 * C + 3}"]
    same = [(v, m, C - 40, v[C - 40:C + 40]), (v, m, 5, v[5:6]), (w, mw, 2 * C, w[2 * C:]), (w, mw, 0, w)]
    outs = check_served(ctx, same)
    assert outs == [m, m, mw, mw]
    # the same request at several batch positions, and twice in one call
    p = b"0123456789" * 7
    one = check_served(ctx, [(v, m, C + 11, p)])[0]
    q = b"-" * 33
    outs = check_served(ctx, [(v, m, C + 11, p), (w, mw, 9, q), (v, m, C + 11, p), (w, mw, C - 9, q), (v, m, C + 11, p)], seed=9)
    assert outs[0] == outs[2] == outs[4] == one


def test_verdicts_bounds_and_capacity(ctx, by):
    import pmc_codec
    v, m = by["json100000"]
    S, K = len(v), 4
    # an empty patch copies the member; a patch that ends at S is served
    outs = check_served(ctx, [(v, m, 77, b""), (v, m, S, b""), (v, m, S - 3, b"end"), (v, m, 0, b"")])
    assert outs[0] == outs[1] == outs[3] == m
    # one byte more, and a 32-bit wrap, are argument errors: nothing written, nothing counted
    reqs = [(m, S - 3, b"end!"), (m, S, b"x"), (m, 0xFFFFFFFF, b"xy"), (m, 0xFFFFFFFE, b"xyz"), (m, S + 1, b"")]
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(ctx, reqs))
    assert list(rc) == [pmc_codec.E_ARG] * len(reqs) and not dlen.any() and got == (0, 0, 0, 0, 0), (rc, dlen, got)
    assert all(s == bytes([GUARD]) * len(s) for s in slots)
    # capacity: need is served, need - 1 is not, and says how much it needs
    cases = [(v, m, C + 5, b"capacity"), (v, m, 0, b""), (v, m, C, bytes(C))]
    fresh = device_compress(ctx, [patched(v, off, p) for v, _, off, p in cases])
    need = [len(f) for f in fresh]
    reqs = [(m, off, p) for _, m, off, p in cases]
    rc, dlen, slots = rewrite_call(ctx, reqs, caps=need)
    assert list(rc) == [0] * 3 and [int(x) for x in dlen] == need and slots == fresh
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(ctx, reqs, caps=[x - 1 for x in need]))
    assert list(rc) == [pmc_codec.E_CAPACITY] * 3 and [int(x) for x in dlen] == need, (rc, dlen)
    assert all(s == bytes([GUARD]) * len(s) for s in slots)
    assert got[:2] == (0, 0) and got[3:] == (0, 0), got
    rc, dlen, slots = rewrite_call(ctx, reqs, caps=[0, 5, 19])
    assert list(rc) == [pmc_codec.E_CAPACITY] * 3 and [int(x) for x in dlen] == need


def declined(ctx, reqs, decoded=0):
    import pmc_codec
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(ctx, reqs))
    assert list(rc) == [pmc_codec.E_NO_INDEX] * len(reqs) and not dlen.any(), (rc, dlen)
    assert all(s == bytes([GUARD]) * len(s) for s in slots)
    assert got == (0, len(reqs), decoded, 0, 0), got


def test_declined_members(ctx, golden, by, vals):
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
    reqs = [(x, 5, b"abc") for x in exact + plain + nocrc + small] + [(x, 0, b"") for x in exact + nocrc]
    reqs += [(b"", 0, b""), (m[:40], 0, b"x"), (m[:-1], 5, b"abc")]
    declined(ctx, reqs)
    w = (golden.corpus * 4)[100:100 + 2 * C + 3]
    reqs = [(assemble_crc(w, sub=sub), 5, b"abc") for sub in crc_defects(w).values()]
    reqs.append((assemble_crc(w, chunk=1 << 14), 5, b"abc"))
    for x, _, _ in reqs:
        assert zlib.decompress(x, 31) == w
    declined(ctx, reqs)
    # an edge chunk of stored blocks is what the chunk decoder declines; a patch over exactly one whole chunk needs
    # no decode and is served
    r, mr = by[RANDOM_NAME]
    declined(ctx, [(mr, 10, b"abc"), (mr, C - 1, b"ab")], decoded=3)
    check_served(ctx, [(r, mr, C, bytes(range(256)) * (C // 256)), (r, mr, 0, b"a" * C), (r, mr, 2 * C, r[:len(r) - 2 * C])])


_FRESH = {}


def lib_span_of(ctx, new_value):
    """fresh_span_of for patch_model.rewrite: the span the library's compress gives a chunk of new_value."""
    if new_value not in _FRESH:
        _FRESH[new_value] = device_compress(ctx, [new_value])[0]
    f = _FRESH[new_value]
    k = parse_index(f)[1]
    table = {}
    for j in range(k):
        s, e, _, _ = chunk_span(f, j)
        table[(new_value[j * C:(j + 1) * C], j == k - 1)] = f[s:e]
    return lambda part, last: table[(part, last)]


def test_damage_is_not_laundered(ctx, golden):
    import pmc_codec
    from test_gpu_range_crc import FLIP_SEED, flips_of
    v = (golden.corpus * 4)[100:100 + 2 * C + 3]
    m = assemble_crc(v)
    flips, per = flips_of(m, np.random.default_rng(FLIP_SEED))
    assert all(x >= 50 for x in per), per
    flips = flips[::9]
    patch = b"[ranged write]"
    # a foreign member: untouched chunks verbatim, touched chunks the library's, header and trailer by the format
    for off in (100, C - 4, 2 * C + 1, C):
        p = patch[:min(len(patch), len(v) - off)]
        want, figures = rewrite(m, off, p, lib_span_of(ctx, patched(v, off, p)))
        (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(ctx, [(m, off, p)]))
        assert rc[0] == 0 and slots[0][:dlen[0]] == want and got == (1, 0) + figures, (off, got, figures)
        assert zlib.decompress(want, 31) == patched(v, off, p)
    # the flip in the edge chunk: declined.  The same flip in an untouched chunk: served, the damaged span is in the
    # output verbatim, and the new member fails its full read on the CRC
    reqs, want = [], []
    for j, b in flips:
        for q in range(3):
            off = q * C + (7 if q < 2 else 1)
            p = patch[:min(len(patch), len(v) - off)]
            reqs.append((b, off, p))
            want.append(None if q == j else rewrite(b, off, p, lib_span_of(ctx, patched(v, off, p)))[0])
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(ctx, reqs))
    nd = sum(1 for w in want if w is None)
    assert nd == len(flips) and got == (len(reqs) - nd, nd, len(reqs), len(reqs) - nd, 2 * (len(reqs) - nd)), got
    carried = []
    for i, w in enumerate(want):
        if w is None:
            assert (rc[i], dlen[i]) == (pmc_codec.E_NO_INDEX, 0), i
            continue
        assert isinstance(w, bytes) and rc[i] == 0 and slots[i][:dlen[i]] == w, i
        j = flips[i // 3][0]
        s0, e0, _, _ = chunk_span(reqs[i][0], j)
        s1, e1, _, _ = chunk_span(w, j)
        assert w[s1:e1] == reqs[i][0][s0:e0]
        with pytest.raises(zlib.error):
            zlib.decompress(w, 31)
        carried.append(w)
    res = ctx.decompress_many(carried[:12], caps=[len(v)] * len(carried[:12]))
    assert [r[0] for r in res] == [pmc_codec.Z_DATA_ERROR] * len(res)
    # a flipped CRC entry is declined at the scan, touched or not; so is a flipped trailer CRC
    at = 16 + 4 * 3 + 8
    reqs = []
    for j in range(3):
        b = m[:at + 4 * j + 2] + bytes([m[at + 4 * j + 2] ^ 4]) + m[at + 4 * j + 3:]
        reqs += [(b, q * C + 1, b"ab") for q in range(3)] + [(b, 0, b"")]
    b = m[:-7] + bytes([m[-7] ^ 0x80]) + m[-6:]
    reqs += [(b, 5, b"ab"), (b, 0, b"")]
    declined(ctx, reqs)


def test_one_mebibyte_value(ctx, by):
    v, m = by[BIG_NAME]
    k = -(-len(v) // C)
    assert k >= 32
    p = bytes(range(65, 91)) * 200
    _, got = counted(ctx, lambda: check_served(ctx, [(v, m, 17 * C + 5000, p[:64]), (v, m, 9 * C - 2048, p[:4096]),
                                                    (v, m, len(v) - 10, p[:10])]))
    assert got == (3, 0, 1 + 2 + 1, 1 + 2 + 1, 3 * k - 4), got


def test_rounds_of_touched_chunks(ctx, by):
    """More touched chunks than one round holds (csrc/pmc_plan.hpp kPatchRoundChunks = 8192): 2100 requests that
    rewrite all four chunks of the same member with the same patch bytes."""
    v, m = by["json100000"]
    new = bytes(reversed(v))
    fresh = device_compress(ctx, [new])[0]
    n = 2100
    (rc, dlen, slots), got = counted(ctx, lambda: rewrite_call(ctx, [(m, 0, new)] * n, caps=[len(fresh)] * n))
    assert not rc.any() and (dlen == len(fresh)).all() and got == (n, 0, 0, 4 * n, 0), got
    assert all(s == fresh for s in slots)


def test_unchanged_ground(ctx, vals, members):
    """After the rewrite calls above, compress and decompress of the module's values give the bytes from before."""
    assert device_compress(ctx, [v for _, v in vals]) == members
    assert ctx.decompress_many(members) == [(0, v) for _, v in vals]

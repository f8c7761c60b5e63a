"""CPU: tests/grow_model.py, the plain-Python statement of growing writes (include/pmc_codec.h "growing writes").
On fixed-block members a member grown by its chunks -- old spans before the first touched chunk, fresh spans from
there on, the member index header for the new number of chunks, the folded trailer -- is the member assembled afresh
from the grown value, and zlib reads it; the untouched chunks keep their spans; what the contract declines is
declined, and damage is carried, not laundered."""
import zlib

import pytest

from fast_large_model import fast_large_tokens
from grow_model import MAX_CHUNKS, grow, grow_of, grown
from indexed_crc_model import assemble_crc, chunk_crcs, crc_defects, parse_chunk_crcs
from indexed_model import C, parse_index
from patch_model import ARG, NO_INDEX, fixed_span, rewrite
from range_model import chunk_span


@pytest.fixture(scope="module")
def corpus(golden):
    return golden.corpus * 4


@pytest.fixture(scope="module")
def span():
    return fixed_span(fast_large_tokens)


_MEMBERS = {}


def member_of(v):
    if v not in _MEMBERS:
        _MEMBERS[v] = assemble_crc(v)
    return _MEMBERS[v]


def text(corpus, n, at=7000):
    return corpus[at:at + n]


def shapes(S):
    """(off, patch length) by the value's length: what lies behind the end, across it, in a gap, on a chunk's first
    byte, and over everything."""
    K = -(-S // C)
    return {
        C + 1: [(S, 1), (S, 2), (S, C - 1), (S, C), (S - 5, 10), (S + 1, 1), (C, 9), (0, S + 10)],
        2 * C: [(S, 1), (S, 2), (S, 3), (S, C), (S, C + 1), (S + 2 * C + 7, 5), ((K - 1) * C, C + 40)],
        2 * C + 3: [(S, 64), (S - 5, 10), (S + 1, 1), (S + C - 3, 3), (C, S), (2 * C, 10)],
        3 * C - 1: [(S, 1), (S, 2), (S, C + 1), (S + 2 * C + 7, 5), (C + 5, 2 * C + 100)],
    }[S]


@pytest.mark.parametrize("S", [C + 1, 2 * C, 2 * C + 3, 3 * C - 1])
def test_grown_members_are_the_fresh_ones(corpus, span, S):
    v = corpus[100:100 + S]
    m = member_of(v)
    K = -(-S // C)
    for off, ln in shapes(S):
        p = text(corpus, ln)
        want = grown(v, off, p)
        assert len(want) == max(S, off + ln) and want[:min(off, S)] == v[:min(off, S)] and want[off:] == p
        assert want[S:off] == bytes(max(0, off - S))
        got, counts = grow(m, off, p, span)
        assert isinstance(got, bytes), (off, ln, got)
        assert got == assemble_crc(want), (off, ln)
        assert zlib.decompress(got, 31) == want, (off, ln)
        K2 = -(-len(want) // C)
        assert parse_index(got)[:2] == (C, K2) and parse_chunk_crcs(got) == chunk_crcs(want), (off, ln)
        _, grows, s2, k2, a, b, items, ea, eb = grow_of(S, 15, off, ln)
        assert grows and (s2, k2) == (len(want), K2) and a <= K - 1 and not eb, (off, ln)
        assert counts == (int(ea), K2 - a, a), (off, ln, counts)
        for k in range(a):  # untouched chunks keep their spans verbatim
            s0, e0, _, _ = chunk_span(m, k)
            s1, e1, _, _ = chunk_span(got, k)
            assert m[s0:e0] == got[s1:e1], (off, ln, k)


def test_superset_and_verdicts(corpus, span):
    S = 2 * C + 3
    v = corpus[100:100 + S]
    m = member_of(v)
    # within the value: the rewrite's answer
    for off, ln in ((5, 64), (C - 1, 2), (2 * C + 1, 2)):
        p = text(corpus, ln)
        assert grow(m, off, p, span) == rewrite(m, off, p, span), (off, ln)
    # an empty patch gives the member itself, wherever it points; the rewrite refuses it behind the end
    assert grow(m, S + 9, b"", span) == (m, (0, 0, 3)) and grow(m, 0xFFFFFFFF, b"", span)[0] == m
    assert rewrite(m, S + 9, b"", span)[0] == ARG
    # ISIZE would wrap; a fresh compress would carry no chunk CRCs
    assert grow(m, 0xFFFFFFFF, b"xy", span) == (ARG, (0, 0, 0))
    assert grow(m, MAX_CHUNKS * C, b"x", span) == (NO_INDEX, (0, 0, 0))
    assert grow_of(S, 15, MAX_CHUNKS * C - 1, 1)[:4] == ("serve", True, MAX_CHUNKS * C, MAX_CHUNKS)
    assert grow_of(S, 15, MAX_CHUNKS * C - 1, 2)[0] == NO_INDEX


def test_declined_members_and_carried_damage(corpus, span):
    S = 2 * C + 3
    v = corpus[100:100 + S]
    m = member_of(v)
    for name, sub in crc_defects(v).items():
        d = assemble_crc(v, sub=sub)
        assert zlib.decompress(d, 31) == v and parse_index(d) is not None, name
        assert grow(d, S, b"abc", span)[0] == NO_INDEX, name
    at = 16 + 4 * 3 + 8
    for j in range(3):  # a flipped entry fails the fold of the old member
        b = bytearray(m)
        b[at + 4 * j + 1] ^= 0x10
        assert grow(bytes(b), S, b"abc", span)[0] == NO_INDEX, j
        assert grow(bytes(b), S + 9, b"", span)[0] == NO_INDEX, j
    assert grow(assemble_crc(v, chunk=1 << 14), S, b"abc", span)[0] == NO_INDEX
    co = zlib.compressobj(9, zlib.DEFLATED, 31)
    assert grow(co.compress(v) + co.flush(), S, b"abc", span)[0] == NO_INDEX
    # damage in the old last chunk -- the edge chunk of an append -- is declined
    s, e, _, _ = chunk_span(m, 2)
    b = bytearray(m)
    b[s + 1] ^= 0x20
    assert grow(bytes(b), S, b"abc", span) == (NO_INDEX, (1, 0, 0))
    # ... but not where the patch covers that chunk from its first byte: it is not looked at
    got, counts = grow(bytes(b), 2 * C, b"0123456789", span)
    assert counts == (0, 1, 2) and zlib.decompress(got, 31) == v[:2 * C] + b"0123456789"
    # damage in chunk 0 is carried along: served, the span verbatim, and the new member fails its full read
    s, e, _, _ = chunk_span(m, 0)
    b = bytearray(m)
    b[(s + e) // 2] ^= 0x20
    b = bytes(b)
    got, counts = grow(b, S, b"abc", span)
    assert isinstance(got, bytes) and counts == (1, 1, 2)
    s1, e1, _, _ = chunk_span(got, 0)
    assert got[s1:e1] == b[s:e]
    with pytest.raises(zlib.error):
        zlib.decompress(got, 31)

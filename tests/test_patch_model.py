"""CPU: tests/patch_model.py, the plain-Python statement of ranged writes (include/pmc_codec.h "ranged writes").
The fold of chunk CRCs is zlib.crc32 of the whole; a member spliced from old spans, fresh spans, the member index
header and the folded trailer is read by zlib as the patched value; and every member the contract declines is
declined."""
import zlib

import numpy as np
import pytest

from fast_large_model import fast_large_tokens
from indexed_crc_model import assemble_crc, chunk_crcs, crc_defects, parse_chunk_crcs
from indexed_model import C, parse_index
from patch_model import ARG, NO_INDEX, fixed_span, fold, member_check, multmodp, patch_of, rewrite, x8n
from range_model import chunk_span


@pytest.fixture(scope="module")
def value(golden):
    return (golden.corpus * 4)[100:100 + 2 * C + 3]


@pytest.fixture(scope="module")
def member(value):
    return assemble_crc(value)


def test_fold_is_crc32():
    rng = np.random.default_rng(11)
    assert x8n(0) == 0x80000000 and multmodp(0x80000000, 0x12345678) == 0x12345678
    for tail in (C, 1, 2, 3, 1696):
        for k in (1, 2, 5):
            v = rng.integers(0, 256, (k - 1) * C + tail, dtype=np.uint8).tobytes()
            crcs = chunk_crcs(v)
            assert len(crcs) == k and fold(crcs, len(v)) == zlib.crc32(v), (tail, k)
    # a flipped entry changes the fold
    v = rng.integers(0, 256, 2 * C + 1696, dtype=np.uint8).tobytes()
    crcs = chunk_crcs(v)
    for j in range(3):
        bad = list(crcs)
        bad[j] ^= 1 << (7 * j)
        assert fold(bad, len(v)) != zlib.crc32(v)


def test_patch_of():
    S = 2 * C + 3
    assert patch_of(S, 15, 0, 0) == (True, 0, 0, 0, False, False)
    assert patch_of(S, 15, S, 0)[0] and not patch_of(S, 15, S, 1)[0] and not patch_of(S, 15, 0xFFFFFFFF, 2)[0]
    assert patch_of(S, 15, 5, 10) == (True, 0, 0, 1, True, False)
    assert patch_of(S, 15, 0, C) == (True, 0, 0, 1, False, False)
    assert patch_of(S, 15, C, C) == (True, 1, 1, 1, False, False)
    assert patch_of(S, 15, C - 1, 2) == (True, 0, 1, 2, True, True)
    assert patch_of(S, 15, C - 5, C + 6) == (True, 0, 2, 3, True, True)
    assert patch_of(S, 15, 2 * C, 3) == (True, 2, 2, 1, False, False)      # the 3-byte tail chunk, whole
    assert patch_of(S, 15, 2 * C, 2) == (True, 2, 2, 1, True, False)
    assert patch_of(S, 15, C, C + 3) == (True, 1, 2, 2, False, False)
    assert patch_of(S, 15, 0, S) == (True, 0, 2, 3, False, False)
    assert patch_of(S, 15, 1, S - 1) == (True, 0, 2, 3, True, False)


PATCHES = [(5, 64), (0, C), (C, C), (C - 1, 2), (C - 5, C + 6), (2 * C, 3), (2 * C + 1, 2), (2 * C + 2, 1),
           (0, 2 * C + 3), (C + 100, 0), (2 * C + 3, 0), (1, 2 * C + 2)]


def test_spliced_members_read_as_the_patched_value(value, member):
    rng = np.random.default_rng(12)
    span = fixed_span(fast_large_tokens)
    assert member_check(member) == (3, chunk_crcs(value), len(value))
    for off, ln in PATCHES:
        patch = rng.integers(97, 123, ln, dtype=np.uint8).tobytes()
        want = value[:off] + patch + value[off + ln:]
        got, counts = rewrite(member, off, patch, span)
        assert isinstance(got, bytes), (off, ln, got)
        assert zlib.decompress(got, 31) == want, (off, ln)
        assert parse_index(got)[:2] == (C, 3) and parse_chunk_crcs(got) == chunk_crcs(want), (off, ln)
        # the model's member is the one assembled afresh from the patched value
        assert got == (member if ln == 0 else assemble_crc(want)), (off, ln)
        ok, a, b, items, ea, eb = patch_of(len(value), 15, off, ln)
        assert counts == (int(ea) + int(eb), items, 3 - items), (off, ln, counts)
        # untouched chunks keep their spans verbatim
        for k in range(3):
            if ln and not a <= k <= b:
                s0, e0, _, _ = chunk_span(member, k)
                s1, e1, _, _ = chunk_span(got, k)
                assert member[s0:e0] == got[s1:e1]
    # a patch equal to the old bytes gives the member back
    assert rewrite(member, C - 9, value[C - 9:C + 40], span)[0] == member
    # bounds: no growth, no wrap
    assert rewrite(member, len(value), b"x", span)[0] == ARG
    assert rewrite(member, len(value) - 1, b"xy", span)[0] == ARG
    assert rewrite(member, 0xFFFFFFFF, b"xy", span)[0] == ARG
    assert isinstance(rewrite(member, len(value) - 1, b"x", span)[0], bytes)


def test_declined_members(value, member):
    span = fixed_span(fast_large_tokens)
    for name, sub in crc_defects(value).items():
        m = assemble_crc(value, sub=sub)
        assert zlib.decompress(m, 31) == value and parse_index(m) is not None, name
        assert rewrite(m, 5, b"abc", span)[0] == NO_INDEX, name
    at = 16 + 4 * 3 + 8
    for j in range(3):  # a flipped entry fails the fold, whichever chunk the patch touches
        b = bytearray(member)
        b[at + 4 * j + 1] ^= 0x10
        for off in (5, C + 5, 2 * C):
            assert rewrite(bytes(b), off, b"abc", span)[0] == NO_INDEX, (j, off)
        assert rewrite(bytes(b), 5, b"", span)[0] == NO_INDEX
    b = bytearray(member)
    b[-6] ^= 1  # the trailer's CRC-32
    assert rewrite(bytes(b), 5, b"abc", span)[0] == NO_INDEX
    # a foreign chunk size, a plain gzip member
    assert rewrite(assemble_crc(value, chunk=1 << 14), 5, b"abc", span)[0] == NO_INDEX
    co = zlib.compressobj(9, zlib.DEFLATED, 31)
    assert rewrite(co.compress(value) + co.flush(), 5, b"abc", span)[0] == NO_INDEX
    # an edge chunk whose stream is damaged is declined; the same damage in an untouched chunk is carried along,
    # and the new member fails its full read
    s, e, _, _ = chunk_span(member, 1)
    b = bytearray(member)
    b[(s + e) // 2] ^= 0x20
    b = bytes(b)
    assert rewrite(b, C + 5, b"abc", span)[0] == NO_INDEX
    got, counts = rewrite(b, 5, b"abc", span)
    assert isinstance(got, bytes) and counts == (1, 1, 2)
    s1, e1, _, _ = chunk_span(got, 1)
    assert got[s1:e1] == b[s:e]
    with pytest.raises(zlib.error):
        zlib.decompress(got, 31)
    # ... while a patch over the whole damaged chunk replaces it without looking at it
    got, counts = rewrite(b, C, b"z" * C, span)
    assert counts == (0, 1, 2) and zlib.decompress(got, 31) == value[:C] + b"z" * C + value[2 * C:]

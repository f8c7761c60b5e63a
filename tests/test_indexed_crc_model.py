"""CPU: the model of chunk CRCs (tests/indexed_crc_model.py; include/pmc_codec.h "member index", chunk CRCs).
A member with the 'P' 'C' subfield is still one gzip member that zlib reads, the 'P' 'I' parser reads it
unchanged with every offset 8 + 4 K larger, the ranged model gives the same bytes, every single defect of the
subfield leaves an indexed member that carries no CRCs, pmc_gzip_index_crc_info agrees with the Python parser
on all of them, the plan's K boundary is the library's, and the switches are public and refuse bad arguments
without a context or a device."""
import ctypes
import os
import zlib

import pytest

import pmc_codec
from indexed_crc_model import (CRC_FIXED, CRC_MAX_CHUNKS, assemble_crc, chunk_crcs, crc_defects, parse_chunk_crcs, plan,
                               read_range_verified)
from indexed_model import C, MAX_CHUNKS, assemble, parse_index
from range_model import chunk_span, ranges_for, read_range

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)


@pytest.fixture(scope="module")
def value(golden):
    return (golden.corpus * 4)[100:100 + 2 * C + 3]


def both(m):
    """pmc_gzip_index_crc_info and the Python parser on one byte string; they must agree."""
    got, want = pmc_codec.index_crc_info(m), parse_chunk_crcs(m)
    assert got == want, (got, want)
    return want


def test_model_constants_match_the_library():
    src = open(os.path.join(ROOT, "poor-man-s-cache_amd", "csrc", "pmc_plan.hpp")).read()
    assert f"constexpr uint32_t kIdxCrcMaxChunks = {CRC_MAX_CHUNKS};" in src
    assert f"constexpr uint32_t kIdxCrcFixed = {CRC_FIXED};" in src
    assert 8 * CRC_MAX_CHUNKS + 12 <= 65535 < 8 * (CRC_MAX_CHUNKS + 1) + 12


def test_a_member_with_chunk_crcs_is_the_indexed_member_shifted(value):
    for v, chunk in ((value, C), (value[:C + 1], C), (value[:2 * C], C), (value, 4096), (value[:3 * 4096], 4096)):
        m, plain = assemble_crc(v, chunk), assemble(v, chunk)
        k = -(-len(v) // chunk)
        assert zlib.decompress(m, 31) == v
        cb, kk, offs, hdr = parse_index(m)
        pcb, pk, poffs, phdr = parse_index(plain)
        assert (cb, kk) == (pcb, pk) == (chunk, k) and hdr == phdr + 8 + 4 * k == plan(len(v), chunk)[2]
        assert offs == [o + 8 + 4 * k for o in poffs]
        # the 'P' 'I' subfield but for the offsets, and the stream behind the header, are the plain member's
        assert m[:10] == plain[:10] and m[12:20] == plain[12:20] and m[hdr:] == plain[phdr:]
        assert int.from_bytes(m[10:12], "little") == 8 * k + 12 and len(m) == len(plain) + 8 + 4 * k
        assert both(m) == chunk_crcs(v, chunk) and both(plain) is None
        assert plan(len(v), chunk)[4] == 16 + 4 * k + 8
        for off, ln in ranges_for(len(v), chunk):
            want = read_range(plain, off, ln)
            assert want == v[off:off + ln]
            assert read_range(m, off, ln) == want
            for require in (False, True):
                assert read_range_verified(m, off, ln, require=require) == want
            assert read_range_verified(plain, off, ln) == want and read_range_verified(plain, off, ln, require=True) is None
        assert read_range_verified(m, 0, 100, cap=99) == ("capacity", 100)
        assert read_range_verified(plain, 0, 100, cap=99, require=True) is None  # (declined before the capacity verdict)


def test_every_single_defect_of_the_subfield(value):
    v = value
    good = assemble_crc(v)
    assert both(good) == chunk_crcs(v)
    for name, sub in crc_defects(v).items():
        m = assemble_crc(v, sub=sub)
        assert zlib.decompress(m, 31) == v, name
        assert parse_index(m) is not None and parse_index(m)[:2] == (C, 3), name
        assert both(m) is None, name
        assert read_range(m, C - 1, 2) == v[C - 1:C + 1], name
        assert read_range_verified(m, C - 1, 2) == v[C - 1:C + 1] and read_range_verified(m, C - 1, 2, require=True) is None
    assert assemble_crc(v, sub=b"") == assemble(v)
    # a defect of the index itself takes the CRCs with it
    for at, b in ((12, b"PJ"), (16, b"\x02"), (17, b"\x0e"), (3, b"\x00")):
        assert both(good[:at] + b + good[at + len(b):]) is None
    for junk in (b"", good[:10], good[:43], bytes(80)):
        assert both(junk) is None
    # what the rules do not see: a wrong entry, a damaged stream, bytes behind the subfield inside FEXTRA
    at = 16 + 4 * 3 + CRC_FIXED
    wrong = good[:at] + bytes([good[at] ^ 1]) + good[at + 1:]
    assert both(wrong) == [chunk_crcs(v)[0] ^ 1] + chunk_crcs(v)[1:]
    assert read_range_verified(wrong, 5, 10) is None and read_range_verified(wrong, C, 10) == v[C:C + 10]
    from indexed_crc_model import crc_subfield
    longer = assemble_crc(v, sub=crc_subfield(chunk_crcs(v)) + b"ZZ\x01\x00!")
    assert zlib.decompress(longer, 31) == v and both(longer) == chunk_crcs(v)
    s, e, _, _ = chunk_span(good, 1)
    dam = good[:s + 40] + bytes([good[s + 40] ^ 0x10]) + good[s + 41:]
    assert both(dam) == chunk_crcs(v)


def test_plan_boundaries():
    for k in (2, 3, CRC_MAX_CHUNKS - 1, CRC_MAX_CHUNKS):
        assert plan(k * C) == (True, k, 20 + 4 * (k - 1) + 8 + 4 * k, True, 20 + 4 * (k - 1) + 8)
        assert plan(k * C)[2] - 12 == 8 * k + 12 <= 65535
    for k in (CRC_MAX_CHUNKS + 1, MAX_CHUNKS):  # the plain indexed member of today
        assert plan(k * C) == (True, k, 20 + 4 * (k - 1), False, 0) == plan(k * C, crc=False)
    assert plan(MAX_CHUNKS * C + 1) == (False, 1, 10, False, 0)
    assert plan(C) == (False, 1, 10, False, 0) and plan(C + 1, crc=False) == (True, 2, 24, False, 0)
    assert plan(C + 1) == (True, 2, 40, True, 32) and plan(C + 1, chunk=0) == (False, 1, 10, False, 0)


def test_the_switches_are_public_and_refused_without_a_context():
    L = pmc_codec.lib()
    for on in (0, 1, 2):
        assert L.pmc_ctx_set_index_crc(None, on) == pmc_codec.E_ARG
        assert L.pmc_ctx_set_range_verify(None, on) == pmc_codec.E_ARG
        assert L.pmc_group_set_index_crc(None, on) == pmc_codec.E_ARG
    assert L.pmc_ctx_get_index_crc(None, None) == pmc_codec.E_ARG
    assert L.pmc_ctx_get_range_verify(None, None) == pmc_codec.E_ARG
    assert L.pmc_ctx_range_verify_counts(None, None) == pmc_codec.E_ARG
    hdr = open(os.path.join(ROOT, "include", "pmc_codec.h")).read()
    for decl in ("int pmc_ctx_set_index_crc(pmc_ctx *ctx, int on);", "int pmc_ctx_get_index_crc(pmc_ctx *ctx, int *on);",
                 "int pmc_group_set_index_crc(pmc_group *g, int on);",
                 "int pmc_ctx_set_range_verify(pmc_ctx *ctx, int mode);", "int pmc_ctx_get_range_verify(pmc_ctx *ctx, int *mode);",
                 "int pmc_ctx_range_verify_counts(pmc_ctx *ctx, uint64_t counts[2]);",
                 "int pmc_gzip_index_crc_info(const void *member, size_t len, uint32_t *crcs, uint32_t cap, uint32_t *nchunks);",
                 "int pmc_ctx_range_counts(pmc_ctx *ctx, uint64_t counts[3]);",
                 "int pmc_gzip_index_info(const void *member, size_t len, uint32_t *chunk_bytes, uint32_t *nchunks);"):
        assert decl in hdr, decl
    assert "CHUNK CRCS" in hdr and "PMC_INDEX_CRC" in hdr
    for name in ("index_crc", "range_verify"):
        assert isinstance(getattr(pmc_codec.Context, name), property)
    assert callable(pmc_codec.Context.range_verify_counts)


def test_index_crc_info_arguments(value):
    L = pmc_codec.lib()
    m = assemble_crc(value)
    k = ctypes.c_uint32(99)
    assert L.pmc_gzip_index_crc_info(None, 100, None, 0, ctypes.byref(k)) == pmc_codec.E_ARG and k.value == 99
    assert L.pmc_gzip_index_crc_info(assemble(value), len(assemble(value)), None, 0, ctypes.byref(k)) == pmc_codec.E_ARG
    out = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    assert L.pmc_gzip_index_crc_info(m, len(m), out, 2, ctypes.byref(k)) == pmc_codec.E_CAPACITY
    assert k.value == 3 and list(out) == [7, 7, 7, 7]
    assert L.pmc_gzip_index_crc_info(m, len(m), out, 2, None) == pmc_codec.E_CAPACITY
    assert L.pmc_gzip_index_crc_info(m, len(m), out, 4, ctypes.byref(k)) == 0
    assert list(out) == chunk_crcs(value) + [7] and k.value == 3
    assert L.pmc_gzip_index_crc_info(m, len(m), out, 3, None) == 0


@pytest.mark.parametrize("bad", ["2", "on", "", "01"])
def test_a_bad_pmc_index_crc_fails_create(monkeypatch, bad):
    """PMC_INDEX_CRC takes 1 or 0; anything else is refused with a text, and no device is touched."""
    L = pmc_codec.lib()
    monkeypatch.setenv("PMC_INDEX_CRC", bad)
    h = ctypes.c_void_p()
    assert L.pmc_ctx_create(0, ctypes.byref(h)) == pmc_codec.E_ARG and not h.value
    assert "PMC_INDEX_CRC" in pmc_codec.last_error() and "1 or 0" in pmc_codec.last_error()

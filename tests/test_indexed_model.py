"""CPU: the model of indexed members (tests/indexed_model.py; include/pmc_codec.h "member index") is a
lossless parse of every listed value whose chunks replay behind nothing, its constants are the library's,
up to one chunk it is the segmented fast parse, the switch is public and refused without a context, a bad
PMC_INDEX fails pmc_ctx_create, and pmc_gzip_index_info agrees with the Python parser on hand-assembled
headers, good and bad."""
import ctypes
import os
import zlib

import pytest

import pmc_codec
from fast_large_model import G, H, fast_large_tokens
from fast_large_values import BIG_NAME
from indexed_model import (C, LOG2C, MAX_CHUNKS, assemble, header, header_len, indexed_chunks, is_indexed,
                           parse_index, replay)
from indexed_values import JSON_SIZES, LAST_MATCH_NAME, PERIOD, RANDOM_NAME, indexed_values

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)


@pytest.fixture(scope="module")
def values(golden):
    vals = indexed_values(golden.corpus)
    assert vals[-1][0] == BIG_NAME and len(vals[-1][1]) == 1 << 20
    assert len({n for n, _ in vals}) == len(vals)
    return vals[:-1]


def test_model_constants_match_the_library():
    plan = open(os.path.join(ROOT, "poor-man-s-cache_amd", "csrc", "pmc_plan.hpp")).read()
    assert f"#define PMC_IDX_CHUNK {C}\n" in plan
    assert f"constexpr uint32_t kIdxMaxChunks = {MAX_CHUNKS};" in plan
    assert "constexpr uint32_t kIdxHdrFixed = 20;" in plan
    assert f"constexpr uint32_t kIdxSeg = {G};" in plan
    fl = open(os.path.join(ROOT, "poor-man-s-cache_amd", "csrc", "pmc_deflate_fast_large.hip")).read()
    assert "static_assert(kIdxSeg == kFlSeg && kIdxChunk % kFlSeg == 0" in fl
    assert C == 1 << LOG2C and C % G == 0


def test_value_list_is_the_one_the_format_is_stated_on(values):
    by = dict(values)
    assert JSON_SIZES == [C, C + 1, 2 * C, 2 * C + 1, 2 * C + 2, 2 * C + 3, 3 * C - 1, C + G, C + G + 1, 100000, 4 * C]
    assert [len(by[f"json{n}"]) for n in JSON_SIZES] == JSON_SIZES
    assert by["a_run"] == b"a" * (2 * C + 5000)
    p = by["period"]
    assert PERIOD > H and len(p) > 2 * C and p[PERIOD:] == p[:-PERIOD]
    s = by["across"]
    assert s[C - 150:C + 150] == s[C - 1174:C - 874]
    assert len(by[RANDOM_NAME]) == 70000


def test_every_chunk_replays_behind_nothing(values):
    for name, v in values:
        chunks = indexed_chunks(v)
        assert len(chunks) == -(-len(v) // C), name
        for k, toks in enumerate(chunks):
            assert replay(toks) == v[k * C:(k + 1) * C], (name, k)  # (replay asserts dist <= position)
            p = 0
            for t in toks:
                if isinstance(t, tuple):
                    assert 3 <= t[0] <= 258 and 1 <= t[1] <= min(p, G + H - 1), (name, k, p, t)
                    p += t[0]
                else:
                    p += 1


def test_values_hit_the_rules_they_are_built_for(values):
    by = dict(values)
    # tail chunks of one, two and three bytes: literals
    for n in (C + 1, 2 * C + 1, 2 * C + 2, 2 * C + 3):
        v = by[f"json{n}"]
        tail = indexed_chunks(v)[-1]
        assert tail == list(v[(len(v) - 1) // C * C:]), n
    # a run of one byte starts over with two literals in every chunk
    for toks in indexed_chunks(by["a_run"]):
        assert toks[:3] == [97, 97, (258, 1)] or len(toks) < 3
    # the repeat across C: cut at the chunk's end, and its second half is not found from before C
    s = by["across"]
    c0, c1 = indexed_chunks(s)
    assert c0[-1] == (150, 1024)
    assert c1[:150] == list(s[C:C + 150])
    assert fast_large_tokens(s[:C + G])[len(c0)] == (150, 1024)  # (the unchunked parse does find it)
    # the last chunk is one block's worth of symbols, the last of them a match
    last = indexed_chunks(by[LAST_MATCH_NAME])[-1]
    assert len(indexed_chunks(by[LAST_MATCH_NAME])) == 2 and len(last) == 16383 and last[-1] == (40, 300)
    # the period's copy lies further back than the history, and never before the chunk
    for toks in indexed_chunks(by["period"]):
        long_d = {t[1] for t in toks if isinstance(t, tuple) and t[0] >= 32}
        assert long_d == {PERIOD}


def test_up_to_one_chunk_the_model_is_the_segmented_fast_parse(golden):
    for n in (1, 2, 3, G, G + 1, 20000, C - 1, C):
        v = (golden.corpus * 2)[700:700 + n]
        assert not is_indexed(n) and header_len(n) == 10
        assert indexed_chunks(v) == [fast_large_tokens(v)], n
    assert is_indexed(C + 1) and header_len(C + 1) == 24 and header_len(4 * C) == 32 and header_len(4 * C + 1) == 36
    assert is_indexed(MAX_CHUNKS * C) and not is_indexed(MAX_CHUNKS * C + 1)
    assert header_len(MAX_CHUNKS * C) - 12 == 8 + 4 * (MAX_CHUNKS - 1) <= 65535


def test_the_switch_is_public_and_refused_without_a_context():
    L = pmc_codec.lib()
    assert L.pmc_ctx_set_index(None, 1) == pmc_codec.E_ARG
    assert L.pmc_ctx_get_index(None, None) == pmc_codec.E_ARG
    assert L.pmc_group_set_index(None, 1) == pmc_codec.E_ARG
    assert L.pmc_ctx_index_counts(None, None) == pmc_codec.E_ARG
    hdr = open(os.path.join(ROOT, "include", "pmc_codec.h")).read()
    for decl in ("int pmc_ctx_set_index(pmc_ctx *ctx, int on);", "int pmc_ctx_get_index(pmc_ctx *ctx, int *on);",
                 "int pmc_group_set_index(pmc_group *g, int on);", "int pmc_ctx_index_counts(pmc_ctx *ctx, uint64_t counts[2]);",
                 "int pmc_gzip_index_info(const void *member, size_t len, uint32_t *chunk_bytes, uint32_t *nchunks);"):
        assert decl in hdr, decl
    assert "member index" in hdr
    assert isinstance(pmc_codec.Context.index, property)


@pytest.mark.parametrize("bad", ["2", "on", "", "01"])
def test_a_bad_pmc_index_fails_create(monkeypatch, bad):
    """PMC_INDEX takes 1 or 0; anything else is refused with a text, and no device is touched."""
    L = pmc_codec.lib()
    monkeypatch.setenv("PMC_INDEX", bad)
    h = ctypes.c_void_p()
    assert L.pmc_ctx_create(0, ctypes.byref(h)) == pmc_codec.E_ARG and not h.value
    assert "PMC_INDEX" in pmc_codec.last_error() and "1 or 0" in pmc_codec.last_error()


def gz6(v):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(v) + c.flush()


def both(m):
    """pmc_gzip_index_info and the Python parser on one byte string; they must agree."""
    got, want = pmc_codec.index_info(m), parse_index(m)
    assert got == (None if want is None else want[:2]), (got, want)
    return want


def test_index_info_agrees_with_the_parser_on_assembled_headers(golden):
    v = (golden.corpus * 2)[100:100 + 2 * C + 3]
    m = assemble(v)
    assert zlib.decompress(m, 31) == v
    cb, k, offs, hdr = both(m)
    assert (cb, k, hdr) == (C, 3, 28) and len(offs) == 2 and m[:20] == header(len(v), offs)[:20]
    for o in offs:  # every offset follows an empty stored block
        assert m[o - 4:o] == b"\x00\x00\xff\xff"
    # other chunk sizes the decoder reads
    small = assemble(v, chunk=4096)
    assert zlib.decompress(small, 31) == v and both(small)[:2] == (4096, 17)
    assert both(assemble(v[:3 * 4096], chunk=4096))[:2] == (4096, 3)
    # not indexed at all
    for plain in (gz6(v), b"", m[:10], m[:31], bytes(64)):
        assert both(plain) is None
    # every single defect
    def put(at, b):
        return m[:at] + bytes(b) + m[at + len(b):]
    bad = {
        "flg": put(3, [0]), "flg+name": put(3, [12]), "id": put(12, b"PJ"), "id2": put(12, b"QI"), "version": put(16, [2]),
        "version0": put(16, [0]), "reserved": put(18, [1]), "reserved2": put(19, [1]), "log2c_low": put(17, [11]),
        "log2c_high": put(17, [25]), "log2c_other": put(17, [14]), "len-4": put(14, (8).to_bytes(2, "little")),
        "len+4": put(14, (16).to_bytes(2, "little")), "len_odd": put(14, (13).to_bytes(2, "little")),
        "xlen_short": put(10, (15).to_bytes(2, "little")), "isize": m[:-4] + (len(v) + C).to_bytes(4, "little"),
        "isize_small": m[:-4] + (C).to_bytes(4, "little"), "off0": put(20, bytes(4)),
        "off_at_header": put(20, (28).to_bytes(4, "little")), "off_swapped": put(20, m[24:28] + m[20:24]),
        "off_equal": put(24, m[20:24]), "off_beyond": put(24, (len(m) - 8).to_bytes(4, "little")),
        "off_huge": put(24, b"\xff\xff\xff\xff"), "truncated": m[:40],
    }
    for name, b in bad.items():
        assert both(b) is None, name
    # defects the rules do not see: the index is reported, the stream is not checked
    ok = {"off+1": put(20, (offs[0] + 1).to_bytes(4, "little")), "off-1": put(24, (offs[1] - 1).to_bytes(4, "little")),
          "xlen_longer": m[:10] + (17).to_bytes(2, "little") + m[12:28] + b"\0" + m[28:], "stream": put(40, [m[40] ^ 0x55]),
          "crc": put(len(m) - 8, [m[-8] ^ 1]), "last_below_end": put(24, (len(m) - 9).to_bytes(4, "little"))}
    for name, b in ok.items():
        assert both(b) is not None, name
    assert pmc_codec.lib().pmc_gzip_index_info(None, 100, None, None) == pmc_codec.E_ARG
    assert pmc_codec.lib().pmc_gzip_index_info(m, len(m), None, None) == 0

"""CPU: tests/range_model.py, the statement of ranged reads, on members put together on the CPU
(tests/indexed_model.py assemble): every range of the list gives the value's bytes, at the library's chunk size
and at 4 KiB; a member without a usable index is declined; and on every corruption of two members the model
either declines or returns bytes -- the value's, where the chunks it read and their index entries are
untouched."""
import zlib

import pytest

from indexed_model import C, assemble, parse_index
from indexed_values import indexed_values
from range_model import chunk_span, covered, range_of, ranges_for, read_range
from test_gpu_indexed import corruptions

NAMES = [f"json{C + 1}", f"json{2 * C + 3}", "json100000", "across"]


@pytest.fixture(scope="module")
def built(golden):
    by = dict(indexed_values(golden.corpus))
    return {(n, ch): (by[n], assemble(by[n], chunk=ch)) for n in NAMES for ch in (C, 4096)}


def test_range_of():
    assert range_of(100000, 15, 0, 1) == (0, 1, 0, 1)
    assert range_of(100000, 15, C - 1, 2) == (C - 1, 2, 0, 2)
    assert range_of(100000, 15, C, C) == (C, C, 1, 1)
    assert range_of(100000, 15, 99997, 10) == (99997, 3, 3, 1)
    assert range_of(100000, 15, 100000, 5) == (100000, 0, 0, 0)
    assert range_of(100000, 15, 0xFFFFFFFF, 0xFFFFFFFF) == (100000, 0, 0, 0)
    assert range_of(0xFFFFFFFF, 16, 1, 0xFFFFFFFF) == (1, 0xFFFFFFFE, 0, 65536)
    assert range_of(100000, 15, 5, 0)[1] == 0


def test_ranges_give_the_values_bytes(built):
    for (name, ch), (v, m) in built.items():
        assert zlib.decompress(m, 31) == v
        for off, ln in ranges_for(len(v), ch):
            assert read_range(m, off, ln) == v[off:off + ln], (name, ch, off, ln)
        ks = covered(m, ch, 1)
        assert ks == [1], (name, ch)
        assert read_range(m, 0, len(v), cap=len(v) - 1) == ("capacity", len(v))
        assert read_range(m, len(v), 5, cap=0) == b""


def test_members_without_a_usable_index(built):
    v, _ = built[(NAMES[0], C)]
    z = zlib.compressobj(6, zlib.DEFLATED, 31)
    assert read_range(z.compress(v) + z.flush(), 0, 1) is None
    big = v * 5
    m17 = assemble(big, chunk=1 << 17)
    assert parse_index(m17)[0] == 1 << 17 and zlib.decompress(m17, 31) == big
    assert read_range(m17, 0, 1) is None and covered(m17, 0, 1) is None


def test_corruptions_decline_or_give_bytes(built):
    for name in (f"json{2 * C + 3}", "json100000"):
        v, m = built[(name, C)]
        served = 0
        for cname, b in corruptions(m):
            for off, ln in ((5, 100), (C - 3, 9), (len(v) - 50, 50)):
                got = read_range(b, off, ln)
                assert got is None or isinstance(got, bytes), (name, cname)
                ks = covered(b, off, ln)
                if ks is None or covered(m, off, ln) != ks or len(b) != len(m):
                    continue
                spans = [chunk_span(m, k)[:2] for k in ks]
                if (parse_index(b)[:2] == parse_index(m)[:2] and b[-4:] == m[-4:]
                        and [chunk_span(b, k)[:2] for k in ks] == spans
                        and all(b[s:e] == m[s:e] for s, e in spans)):
                    assert got == v[off:off + ln], (name, cname, off, ln)
                    served += 1
        # (100 of the mutations fall anywhere in a member of three or four chunks: each of them leaves at least
        # one of the three ranges' chunks alone, unless it hits an index entry or the trailer)
        assert served >= 50, served

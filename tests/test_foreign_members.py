"""CPU: the oracle's inflate against zlib itself on members this project did not write.

The oracle (oracle/inflate.c) is the ruler every GPU decoder is measured with, and it claims zlib 1.2.11's
verdict for every member.  Here zlib's own gzip inflate (zlib.decompressobj(31)) and the oracle decode the
whole corpus of tests/foreign_members.py -- zlib's members at every level, strategy, memLevel and flush,
hand-assembled valid and invalid streams, and mutations of both -- and must agree on every verdict and
every byte, none left out.  Where they differ, zlib is right."""
import collections
import zlib

import pytest

import deflate_builder as B
import foreign_members as F


@pytest.fixture(scope="module")
def verdicts(golden):
    """[(entry, zlib's (rc, bytes), the oracle's (rc, bytes))] over the whole corpus, computed once."""
    from oracle import pyoracle as O
    return [(e, F.zlib_verdict(e.member), O.decompress(e.member)) for e in F.entries(golden.corpus)]


def test_corpus_is_deterministic_and_named(golden):
    a = F.corpus(golden.corpus)
    F._cache.clear()
    b = F.corpus(golden.corpus)
    assert a == b
    assert len({n for n, _, _ in a}) == len(a)
    assert {c for _, c, _ in a} == {"zlib", "crafted-valid", "crafted-invalid", "crafted-truncated", "mutated"}
    assert sum(1 for _, c, _ in a if c == "zlib") <= 1500


def test_oracle_agrees_with_zlib_on_every_member(verdicts):
    counts = collections.Counter(e.category for e, _, _ in verdicts)
    print(f"zlib {zlib.ZLIB_RUNTIME_VERSION}; members per category: {dict(sorted(counts.items()))}; "
          f"total {len(verdicts)}")
    bad = [(e.name, z[0], o[0], len(z[1]), len(o[1])) for e, z, o in verdicts if z != o]
    print(f"disagreements: {len(bad)} of {len(verdicts)}")
    assert not bad, bad[:10]


def test_valid_members_decode_to_what_was_meant(verdicts):
    for e, z, o in verdicts:
        if e.category in ("zlib", "crafted-valid"):
            assert z == (0, e.value) and o == (0, e.value), e.name


def test_invalid_members_are_data_errors(verdicts):
    n = 0
    for e, z, o in verdicts:
        if e.category == "crafted-invalid":
            n += 1
            assert z[0] == -3 and o[0] == -3, (e.name, z[0], o[0])
        if e.category == "crafted-truncated":
            assert z[0] == -5 and o[0] == -5, (e.name, z[0], o[0])
    assert n >= 100


def test_mutations_cover_every_verdict(verdicts):
    mix = collections.Counter(z[0] for e, z, _ in verdicts if e.category == "mutated")
    large = sum(1 for e, z, _ in verdicts if e.category == "mutated" and z[0] == -3 and e.size > 4096)
    print(f"mutated verdicts: {dict(mix)}; data errors in members of more than 4096 bytes: {large}")
    assert set(mix) == {0, -3, -5}
    assert min(mix.values()) >= 20, mix
    assert large >= 50


def test_builder_writes_what_zlib_reads():
    """The assembler's own pieces, each against zlib's raw inflate."""
    toks = [104, 101, 108, 108, 111, (3, 1), (258, 5), (258, 2, 284), 33]
    want = B.apply_tokens(toks)
    for final_kind in ("fixed", "dynamic", "plain-lengths"):
        w = B.BitWriter()
        B.stored_block(w, b"ab", False)
        if final_kind == "fixed":
            B.fixed_block(w, toks, True)
        else:
            ll, dl = B.lengths_for(toks)
            cl = B.cl_symbols_plain(ll + dl) if final_kind == "plain-lengths" else None
            B.dynamic_block(w, toks, ll, dl, True, cl_symbols=cl)
        assert zlib.decompress(w.getvalue(), -15) == b"ab" + want, final_kind
    lens = [3, 3, 3, 3, 3, 2, 4, 4]  # RFC 1951 3.2.2's example
    assert B.canonical_codes(lens) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    assert B.expand_cl(B.cl_symbols_rle([0] * 150 + [7] * 9 + [0, 0, 5])) == [0] * 150 + [7] * 9 + [0, 0, 5]
    m = B.gzip_member(zlib.compress(b"x" * 50)[2:-4], b"x" * 50, extra=b"\x00" * 4, name=b"n\x00", comment=b"c\x00",
                      hcrc=True, mtime=7, xfl=2, os=9)
    assert zlib.decompress(m, 31) == b"x" * 50 and m[3] == 0x1E

"""CPU: what tests/test_gpu_back.py relies on, checked without a GPU.

The corpus of tests/back_values.py meets every class of the table below: the classes are read off the oracle's member
of each value by back_values.dissect (the bit position and width of every token, the code lengths, the tree header's
runs) and off its block facts, never off device output.  S: values of at most kHdrMinLen bytes (the back's own
send_runs_fused writes the tree header), L: longer ones (the trees kernel's emit_header does); both constants are
read from csrc/pmc_kernels.hpp.  A count is the number of values that meet the class; "-" marks a class of
back_values.unreached(), which no value may meet (else the entry is stale); classes that are not per side have
their count under "all".

  class                                   S    L  all
  code:bl-len=7                                    13
  code:d-len=1                                     19
  code:d-len=2                                     30
  code:d-len=3                                     45
  code:d-len=4                                     33
  code:d-len=5                                     28
  code:d-len=6                                     19
  code:d-len=7                                     10
  code:d-len=8                                      5
  code:d-len=9                                      4
  code:d-len=10                                     2
  code:d-len=11                                     1
  code:d-len=12                                     1
  code:d-len=13                                     -
  code:d-len=14                                     -
  code:d-len=15                                     -
  code:group-in-3-chunks                           33
  code:group>=65                                   18
  code:ll-len=1                                     1
  code:ll-len=2                                    19
  code:ll-len=3                                    31
  code:ll-len=4                                    41
  code:ll-len=5                                    49
  code:ll-len=6                                    51
  code:ll-len=7                                    45
  code:ll-len=8                                    32
  code:ll-len=9                                    22
  code:ll-len=10                                    7
  code:ll-len=11                                    4
  code:ll-len=12                                    4
  code:ll-len=13                                    3
  code:ll-len=14                                    1
  code:ll-len=15                                    -
  code:nomatch,HDIST=1                              7
  crc:513..1024:mod16=0                             2
  crc:513..1024:mod16=1                             2
  crc:513..1024:mod16=2                             1
  crc:513..1024:mod16=3                             2
  crc:513..1024:mod16=4                             2
  crc:513..1024:mod16=5                             1
  crc:513..1024:mod16=6                             1
  crc:513..1024:mod16=7                             1
  crc:513..1024:mod16=8                             4
  crc:513..1024:mod16=9                             2
  crc:513..1024:mod16=10                            1
  crc:513..1024:mod16=11                            1
  crc:513..1024:mod16=12                            1
  crc:513..1024:mod16=13                            3
  crc:513..1024:mod16=14                            1
  crc:513..1024:mod16=15                            1
  crc:<=512:mod16=0                                 3
  crc:<=512:mod16=1                                 4
  crc:<=512:mod16=2                                 2
  crc:<=512:mod16=3                                 1
  crc:<=512:mod16=4                                 3
  crc:<=512:mod16=5                                 4
  crc:<=512:mod16=6                                 3
  crc:<=512:mod16=7                                 3
  crc:<=512:mod16=8                                 5
  crc:<=512:mod16=9                                 2
  crc:<=512:mod16=10                                2
  crc:<=512:mod16=11                                1
  crc:<=512:mod16=12                                5
  crc:<=512:mod16=13                                2
  crc:<=512:mod16=14                                2
  crc:<=512:mod16=15                                4
  crc:>1024:mod16=0                                 1
  crc:>1024:mod16=1                                 1
  crc:>1024:mod16=2                                 1
  crc:>1024:mod16=3                                 1
  crc:>1024:mod16=4                                 1
  crc:>1024:mod16=5                                 1
  crc:>1024:mod16=6                                 1
  crc:>1024:mod16=7                                 1
  crc:>1024:mod16=8                                 1
  crc:>1024:mod16=9                                 1
  crc:>1024:mod16=10                                2
  crc:>1024:mod16=11                                1
  crc:>1024:mod16=12                                3
  crc:>1024:mod16=13                                1
  crc:>1024:mod16=14                                4
  crc:>1024:mod16=15                                1
  crc:len=1                                         1
  crc:len=2                                         1
  crc:len=3                                         1
  crc:len=4                                         1
  crc:len=5                                         1
  crc:len=6                                         1
  crc:len=7                                         1
  crc:len=8                                         1
  crc:len=9                                         1
  crc:len=10                                        1
  crc:len=11                                        1
  crc:len=12                                        1
  crc:len=13                                        1
  crc:len=14                                        1
  crc:len=15                                        1
  crc:len=1024                                      1
  crc:len=1025                                      1
  crc:len=16382                                     3
  d:last-run-from-earlier-chunk           -    -
  d:run-into-next-chunk                   -    -
  d:run-over-whole-chunk                  -    -
  d:run-starts@lane0                      -    -
  d:run-starts@lane63                     -    -
  d:run=1                                16   36
  d:run=2                                 9   31
  d:run=3                                 4   17
  d:run=4                                 1    7
  d:run=6                                 1    1
  d:run=7                                 1    1
  d:run=8                                 1    1
  d:run>=13                               -    -
  d:zrun=1                                8   23
  d:zrun=2                                7    9
  d:zrun=3                                1    4
  d:zrun=10                               2    3
  d:zrun=11                               1    1
  d:zrun=138                              -    -
  d:zrun=139                              -    -
  d:zrun>=277                             -    -
  dcode=0:base                           22   20
  dcode=0:top                            22   20
  dcode=1:base                            5   14
  dcode=1:top                             5   14
  dcode=2:base                           10   14
  dcode=2:top                            10   14
  dcode=3:base                            9   12
  dcode=3:top                             9   12
  dcode=4:base                            8   13
  dcode=4:top                             9   18
  dcode=5:base                            9   12
  dcode=5:top                             7   16
  dcode=6:base                            8   11
  dcode=6:top                             9   14
  dcode=7:base                            8   13
  dcode=7:top                             8   18
  dcode=8:base                            8   13
  dcode=8:top                             5   15
  dcode=9:base                            4   16
  dcode=9:top                             6   14
  dcode=10:base                           5    8
  dcode=10:top                            3    8
  dcode=11:base                           4    9
  dcode=11:top                            3   10
  dcode=12:base                           5   12
  dcode=12:top                            2   11
  dcode=13:base                           1   11
  dcode=13:top                            1    8
  dcode=14:base                           5    9
  dcode=14:top                            3   10
  dcode=15:base                           3    9
  dcode=15:top                            2    5
  dcode=16:base                           1    6
  dcode=16:top                            2    2
  dcode=17:base                           1    7
  dcode=17:top                            -    5
  dcode=18:base                           -    2
  dcode=18:top                            -    3
  dcode=19:base                           -    2
  dcode=19:top                            -    3
  dcode=20:base                           -    4
  dcode=20:top                            -    4
  dcode=21:base                           -    3
  dcode=21:top                            -    3
  dcode=22:base                           -    2
  dcode=22:top                            -    3
  dcode=23:base                           -    2
  dcode=23:top                            -    2
  dcode=24:base                           -    2
  dcode=24:top                            -    2
  dcode=25:base                           -    2
  dcode=25:top                            -    2
  dcode=26:base                           -    2
  dcode=26:top                            -    1
  dcode=27:base                           -    1
  dcode=27:top                            -    -
  dcode=28:base                           -    -
  dcode=28:top                            -    -
  dcode=29:base                           -    -
  dcode=29:top                            -    -
  fixed:dext=12                           -    1
  fixed:lcode>=23                         8    5
  fixed:lit>=144                         15    5
  hdr-bits%32=0                           1    1
  hdr-bits%32=1                           2    3
  hdr-bits%32=31                          1    1
  lcode=0:base                           22   38
  lcode=0:top                            22   38
  lcode=1:base                           23   32
  lcode=1:top                            23   32
  lcode=2:base                           18   25
  lcode=2:top                            18   25
  lcode=3:base                           14   21
  lcode=3:top                            14   21
  lcode=4:base                            7   18
  lcode=4:top                             7   18
  lcode=5:base                            7   13
  lcode=5:top                             7   13
  lcode=6:base                            5   12
  lcode=6:top                             5   12
  lcode=7:base                            5   12
  lcode=7:top                             5   12
  lcode=8:base                            2    5
  lcode=8:top                             6   12
  lcode=9:base                            3    3
  lcode=9:top                             1    3
  lcode=10:base                           3    3
  lcode=10:top                            1    2
  lcode=11:base                           1    3
  lcode=11:top                            1    1
  lcode=12:base                           1    3
  lcode=12:top                            1    2
  lcode=13:base                           2    2
  lcode=13:top                            1    1
  lcode=14:base                           1    1
  lcode=14:top                            2    1
  lcode=15:base                           1    2
  lcode=15:top                            1    2
  lcode=16:base                           1    3
  lcode=16:top                            1    2
  lcode=17:base                           1    1
  lcode=17:top                            1    1
  lcode=18:base                           1    1
  lcode=18:top                            1    1
  lcode=19:base                           1    2
  lcode=19:top                            1    2
  lcode=20:base                           1    1
  lcode=20:top                            1    1
  lcode=21:base                           1    1
  lcode=21:top                            1    4
  lcode=22:base                           1    4
  lcode=22:top                            1    3
  lcode=23:base                           1    1
  lcode=23:top                            1    3
  lcode=24:base                           1    2
  lcode=24:top                            1    3
  lcode=25:base                           1    2
  lcode=25:top                            1    2
  lcode=26:base                           1    3
  lcode=26:top                            1    4
  lcode=27:base                           1    2
  lcode=27:top                            1    3
  lcode=28:base                           1    2
  lcode=28:top                            1    2
  ll:last-run-from-earlier-chunk          1    1
  ll:run-into-next-chunk                 13   30
  ll:run-over-whole-chunk                14   22
  ll:run-starts@lane0                    17   40
  ll:run-starts@lane63                    9   23
  ll:run=1                               19   41
  ll:run=2                               17   37
  ll:run=3                               13   29
  ll:run=4                                4   21
  ll:run=6                                3    9
  ll:run=7                                3    7
  ll:run=8                                3    7
  ll:run>=13                              1    7
  ll:zrun=1                              15   26
  ll:zrun=2                              10   24
  ll:zrun=3                               8   20
  ll:zrun=10                              3    5
  ll:zrun=11                              2    5
  ll:zrun=138                             2    3
  ll:zrun=139                             2    4
  ll:zrun=141                             1    1
  ll:zrun=149                             1    1
  ll:zrun>=277                            -    -
  ntok%64=0                               1    4
  ntok%64=1                               1    1
  ntok%64=63                              1    2
  ntok=1                                  1    -
  ntok=2                                  1    -
  tok-3words                              -    1
  tok-end@31                             29   46
  tok-start@0                            29   46
  tok-width>=24                           2
  tok-width>=40                                1
  trailer:size%4=0                                 22
  trailer:size%4=1                                 23
  trailer:size%4=2                                 21
  trailer:size%4=3                                 28
  type=dynamic                           19   41
  type=fixed                             26    6
  type=stored                             1    1

(printed by `pytest -s tests/test_back_model.py::test_corpus_covers_every_emission_arm`; the test fails if the table
above is not the one it prints.)

Routes: the batch shapes of the GPU test go through tests/host/plan_check's `route` mode: "512" must reach the
split pipeline with a pass cap of at most kNostageMaxLen (the unstaged back), "1k" and "16k" with caps 1024 and 16382
(the staged back), "mono", the host entry's two routes and the switches theirs, big() the large-value pipeline.

Reference members: the oracle, greedy walk and dynamic-programming walk alike, reproduces the reference's own member
of every value of values() and big() (tests/golden/back_golden.json).

The large-value route (deflate_lv_emit_kernel's own token_bits and send_all_trees): what the classifier finds in
tests/large_values.py's sets, values above 16382 bytes (back_values.LARGE_WITNESS names the shortest value per class,
and test_large_route_classes holds it to the class):

  class                      values  shortest witness
  lv:dcode=26:base                8  segment_boundaries_json #5, 49153 B
  lv:dcode=26:top                 3  binary_and_stored #6, 140000 B
  lv:dcode=27:base                2  binary_and_stored #6, 140000 B
  lv:dcode=27:top                 1  multi_megabyte #1, 2 MiB
  lv:dcode=28:base                3  binary_and_stored #3, 70001 B
  lv:dcode=28:top                 1  multi_megabyte #1, 2 MiB
  lv:dcode=29:base                3  binary_and_stored #9, 300007 B
  lv:dcode=29:top                 -  distance 32768 > 32506, the farthest match of zlib's window
  lv:block>0-start%8=0 .. 7  7 to 22  block_edges #34, #14, #9, #15, #20, #8; binary_and_stored #2, #8
  lv:tok-3words:block>0           0  none: met by both values of back_values.big() (34000 and 36000 B)"""
import re

import pytest

import back_values as BV
import large_values as LV
import trees_values as TV
from test_host_plan import EXACT, plan_bin, routes, row  # noqa: F401  (plan_bin: a fixture)


@pytest.fixture(scope="module")
def corpus():
    """[(value, the oracle's member, its block facts, its classes)], computed once."""
    out = []
    for v in BV.values():
        m, f = TV.facts_of(v)
        out.append((v, m, f, BV.classes_of(v, m, f)))
    return out


def test_constants_come_from_the_build():
    hdr, nostage = BV.constants()
    # the sides and the "512" row are cut at these; the length bands of the CRC classes restate them
    assert hdr == 512 and nostage == 512 and BV.LEN_BANDS[0][2] == nostage and BV.ONE_K == 1024
    assert BV.side_of(hdr) == "S" and BV.side_of(hdr + 1) == "L"


def test_every_value_is_one_block(corpus):
    assert len(corpus) == len(BV.PARAMS)
    for k, (v, m, f, _) in enumerate(corpus):
        assert 1 <= len(v) <= BV.MAX_LEN and b"\0" not in v, k
        assert f["stored_len"] == len(v) and f["symbols"] < 16383, k
    assert sum(len(v) for v, _, _, _ in corpus) < 160_000  # (a small corpus: most values are short)


def test_dissector_agrees_with_deflate_dissect(corpus):
    """The bit-position dissector sees the blocks, code lengths and tokens deflate_dissect sees (on the values up to
    1200 bytes: that one decodes bit by bit), its token widths tile the block, and an altered byte is explained."""
    import deflate_dissect as DD
    for k, (v, m, f, _) in enumerate(corpus):
        (b,) = BV.dissect(m)
        if len(v) <= 1200:
            (w,) = DD.dissect(m)
            (g,) = BV.plain([b])
            assert {x: w.get(x) for x in g} == g, k
        if b["type"]:
            at = b["start_bit"] + 3 + b.get("hdr_bits", 0)
            for t in b["tokens"]:
                assert t[0] == at, k
                at += t[1]
            assert b["end_bit"] == at + b["ll"][256] and (b["end_bit"] + 7) // 8 + 8 == len(m), k
    v, m, f, _ = next(c for c in corpus if c[2]["type"] == 2 and len(c[0]) > 300)
    bad = bytearray(m)
    bad[len(m) - 12] ^= 0x10
    assert "lies in token #" in BV.explain(bytes(bad), m) or "end-of-block" in BV.explain(bytes(bad), m)


def table(corpus):
    need, un = BV.required(), BV.unreached()
    have = {}
    for k, (_, _, _, cl) in enumerate(corpus):
        for c in cl:
            have.setdefault(c, []).append(k)
    rows = {}
    for c in list(need) + list(un) + list(have):
        side, name = (c[0], c[2:]) if c[:2] in ("S:", "L:") else ("all", c)
        rows.setdefault(name, {})[side] = "-" if c in un else str(len(have.get(c, [])))
    key = lambda n: [int(x) if x.isdigit() else x for x in re.split(r"(\d+)", n)]  # noqa: E731
    lines = [f"  {'class':<36}{'S':>5}{'L':>5}{'all':>5}"]
    for name in sorted(rows, key=key):
        r = rows[name]
        lines.append(f"  {name:<36}{r.get('S', ''):>5}{r.get('L', ''):>5}{r.get('all', ''):>5}".rstrip())
    return "\n".join(lines), have


def test_corpus_covers_every_emission_arm(corpus):
    text, have = table(corpus)
    print("\n" + text)
    need, un = BV.required(), BV.unreached()
    short = {c: (len(have.get(c, [])), n) for c, n in need.items() if len(have.get(c, [])) < n}
    assert not short, short
    stale = sorted(c for c in un if c in have)
    assert not stale, stale   # an unreached class that a value meets: the entry is stale
    assert not set(need) & set(un)
    assert text in __doc__, "the table of the docstring is not the one printed"


def test_the_repaired_gaps_are_met_by_named_values(corpus):
    """The classes no earlier corpus met, on the sides stated."""
    have = set().union(*(cl for _, _, _, cl in corpus))
    want = ["L:tok-3words", "L:type=fixed", "S:hdr-bits%32=0", "L:hdr-bits%32=0"]
    want += [f"L:dcode={dc}:base" for dc in range(19, 28)] + [f"L:dcode={dc}:top" for dc in range(19, 27)]
    want += [f"{sd}:lcode={lc}:{e}" for sd in BV.SIDES for lc, e in ((25, "base"), (26, "base"), (23, "top"), (27, "top"))]
    want += [f"crc:{band}:mod16={m}" for band, _, _ in BV.LEN_BANDS for m in range(16)]
    assert not [c for c in want if c not in have]
    i = next(k for k, (_, _, _, cl) in enumerate(corpus) if "L:tok-3words" in cl)
    assert BV.PARAMS[i][:4] == ("g", 100, 16382, 4) and BV.PARAMS[i][9] == ((226, 16124),)


def test_distance_base_mutation_changes_no_byte():
    """DESIGN.md, "Back conformance", mutation 3: dist_base_cf with `2 + (dc & 1)` replaced by 2 for dc >= 24 gives
    every distance the same extra value, because emit_symbols masks dm - base to the code's extra bits and the
    bases differ by a multiple of 1 << extra.  (So that build must pass the GPU test, and no class can catch it.)"""
    import deflate_dissect as DD
    for dist in range(1, 32769):
        dm = dist - 1
        dc = dm if dm < 4 else 2 * (dm.bit_length() - 1) + ((dm >> (dm.bit_length() - 2)) & 1)
        xd = 0 if dc < 4 else (dc >> 1) - 1
        base = dc if dc < 4 else (2 + (dc & 1)) << xd
        assert (dc, base, xd) == (max(c for c in range(30) if DD.DBASE[c] <= dist), DD.DBASE[dc] - 1, DD.DEXT[dc])
        mutant = base if dc < 24 else 2 << xd
        assert (dm - base) & ((1 << xd) - 1) == (dm - mutant) & ((1 << xd) - 1) == dist - DD.DBASE[dc]


def test_gpu_batches_hold_what_they_are_meant_for(corpus):
    vs = BV.values()
    hdr, nostage = BV.constants()
    cls = [cl for _, _, _, cl in corpus]
    for name, lim in (("512", hdr), ("1k", BV.ONE_K), ("16k", BV.MAX_LEN)):
        idx = BV.batch(name)
        # above the one-kernel path's 1024 values; from 4096 values a chunk is visited in cO order
        assert len(idx) == BV.N_SPLIT >= 4096 and idx == BV.batch(name)
        assert set(idx) == {i for i, v in enumerate(vs) if len(v) <= lim}
        assert lim - 63 <= max(len(vs[i]) for i in idx) <= lim  # (the pass cap, the next multiple of 64, is the row's)
        if name == "16k":  # the long values once: the row stays short
            assert all(idx.count(i) == 1 for i in set(idx) if len(vs[i]) > BV.LONG)
            assert sum(len(vs[i]) for i in idx) < 8 << 20
        for align in (4, 1):
            vals, offs = BV.packed(idx, align)
            assert vals[-len(idx):] == [vs[i] for i in idx] and (align == 4) == (len(vals) == len(idx))
            mods = {o % 16 for o in offs[1:]}
            if align == 4:
                assert mods == {0, 4, 8, 12}
            else:  # sources at offsets = 0 (mod 16), = 4 (mod 16) and odd
                assert 0 in mods and 4 in mods and any(o & 1 for o in offs)
    # the "512" row alone runs the unstaged back: it holds every side-S class, the other rows every class
    s_classes = {c for c in BV.required() if c.startswith("S:")}
    assert s_classes <= set().union(*(cls[i] for i in BV.batch("512")))
    assert set(BV.required()) <= set().union(*(cls[i] for i in BV.batch("16k")))
    mono = BV.batch("mono")
    assert 50 <= len(mono) <= 1024 and max(len(vs[i]) for i in mono) <= 4096
    assert BV.batch("all") == list(range(len(vs))) and len(vs) <= 1024


def test_every_batch_reaches_its_route(plan_bin):  # noqa: F811
    vs = BV.values()
    hdr, nostage = BV.constants()
    n_mono, max_mono = len(BV.batch("mono")), max(len(vs[i]) for i in BV.batch("mono"))
    n_all = len(vs)
    big = BV.big()
    rows = {}
    longest = {name: max(len(vs[i]) for i in BV.batch(name)) for name in ("512", "1k", "16k")}
    assert longest["1k"] == 1024 and longest["16k"] == 16382
    for extra in (0, 1):  # (the unaligned rows hold one value more)
        for name in longest:
            rows[f"{name}+{extra}"] = row(BV.N_SPLIT + extra, longest[name], EXACT)
    rows.update({
        "mono": row(n_mono, max_mono, EXACT, small=True),
        "v1": row(n_all, BV.MAX_LEN, EXACT, force_v1=1),
        "mono-env": row(n_all, BV.MAX_LEN, EXACT, mono_env=1),
        "latency": row(n_mono, max_mono, EXACT, latency=True),
        "host-all": row(n_all, BV.MAX_LEN, EXACT),
        "big": row(len(big), max(len(v) for v in big), EXACT),
    })
    got = dict(zip(rows, routes(plan_bin, list(rows.values()))))
    for extra in (0, 1):
        # the split pipeline; a pass cap of at most kNostageMaxLen runs the unstaged back, any other the staged one
        a, b, c = got[f"512+{extra}"], got[f"1k+{extra}"], got[f"16k+{extra}"]
        assert (a["kind"], a["passes"]) == ("split", [[0, longest["512"], 512, 0, 0]]) and a["passes"][0][2] <= nostage, a
        assert (b["kind"], b["passes"]) == ("split", [[0, 1024, 1024, 0, 0]]) and b["passes"][0][2] > nostage, b
        assert (c["kind"], c["passes"]) == ("split", [[0, 16382, 16382, 0, 0]]), c
    assert (got["host-all"]["kind"], got["host-all"]["passes"]) == ("split", [[0, 16382, 16382, 0, 0]]), got["host-all"]
    assert (got["mono"]["kind"], got["mono"]["lds_cut"]) == ("mono", max_mono), got["mono"]
    assert (got["latency"]["kind"], got["latency"]["lds_cut"]) == ("mono", max_mono), got["latency"]
    assert (got["mono-env"]["kind"], got["mono-env"]["cap"]) == ("mono", 16382), got["mono-env"]
    assert (got["v1"]["kind"], got["v1"]["gated"]) == ("v1", 0), got["v1"]
    # big(): above the large pass's limit, so the large-value pipeline (deflate_lv_emit_kernel) takes them
    assert got["big"]["lv"] == 1 and got["big"]["hbm_cut"] == 16382 and len(got["big"]["passes"]) == 1, got["big"]


def test_oracle_reproduces_the_reference_members(corpus):
    from oracle import pyoracle as O
    G = BV.BackGolden()
    vals = [v for v, _, _, _ in corpus] + BV.big()
    assert len(G.vectors) == len(vals)
    assert G.mismatches(vals, [m for _, m, _, _ in corpus] + [O.compress(v) for v in BV.big()]) == []
    assert G.mismatches(vals, [O.compress(v, dp=True) for v in vals]) == [], "dp"


def test_large_route_classes(golden):
    """Every class of LARGE_CLASSES is met by its witness in tests/large_values.py's sets (a value the large-value
    pipeline takes: longer than 16382 bytes), is excluded by arithmetic, or is met by every value of big()."""
    from oracle import pyoracle as O
    sets = LV.all_sets(golden.corpus)
    assert set(BV.LARGE_CLASSES) == set(BV.LARGE_WITNESS) | set(BV.LARGE_UNREACHED) | set(BV.LARGE_MISSING)
    seen = {}
    for c, (name, i) in BV.LARGE_WITNESS.items():
        v = sets[name][i]
        assert len(v) > BV.MAX_LEN, c
        if (name, i) not in seen:
            seen[(name, i)] = BV.large_classes_of(O.compress(v))
        assert c in seen[(name, i)], c
    assert len(BV.big()) >= 1
    for v in BV.big():
        assert 33_000 <= len(v) <= 70_000 and b"\0" not in v
        got = BV.large_classes_of(O.compress(v))
        assert set(BV.LARGE_MISSING) <= got and not got & set(BV.LARGE_UNREACHED)

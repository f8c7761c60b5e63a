"""CPU: what tests/test_gpu_trees.py relies on, checked without a GPU.

The corpus of tests/trees_values.py covers every arm of block planning (zlib's build_tree, gen_bitlen, scan_tree,
build_bl_tree and the stored/fixed/dynamic choice, restated one lane per value by deflate_trees_kernel): the table
below is asserted from the oracle's block facts (oracle/pmc_oracle.h: oracle_block_facts) and the dissected tree
headers of the oracle's members, class by class, with the counts of tests/trees_values.py required().  CAP is the
first-pass heap capacity the value's size class meets (kTreesCap1K up to 1024 bytes, kTreesCap above), read from
csrc/pmc_kernels.hpp; nz the literal/length symbols in use, end-of-block included.

  class                  values  dynamic  example (index, bytes)
  bl-overflow                 5        4  #63, 400
  dcode>=26                   7        7  #155, 12000
  depth-tie                 154      145  #3, 16
  depth-tie-ll              136      129  #4, 18
  dleaves=0                  20        9  #0, 1
  dleaves=1                  19       18  #8, 26
  dleaves=2                  22       21  #9, 30
  dleaves>=20                14       14  #130, 1500
  dyn-len=511                 3        3  #70, 511
  dyn-len=512                 4        4  #73, 512
  dyn-len=513                 3        3  #77, 513
  dyn-len=514                 4        4  #80, 514
  dyn-static+1                8        8  #9, 30
  dyn-stored+1                3        3  #10, 32
  fixed-tie                   3        0  #3, 16
  fixed<                      4        0  #0, 1
  hclen=14                    9        9  #57, 300
  hclen=15                    4        4  #154, 9000
  hclen=16                   65       65  #14, 46
  hclen=17                    3        3  #158, 16382
  hclen=18                   68       68  #9, 30
  hlit=257                    9        9  #10, 32
  hlit=258                   36       36  #9, 30
  hlit=286                    3        3  #153, 5000
  nz16k=CAP+0                 5        5  #115, 1025
  nz16k=CAP+1                 5        5  #117, 1025
  nz16k=CAP+2                 3        3  #119, 1025
  nz16k=CAP-1                 4        4  #114, 1025
  nz1k=CAP+0                  4        3  #50, 100
  nz1k=CAP+1                  6        6  #84, 600
  nz1k=CAP+2                  5        4  #52, 120
  nz1k=CAP-1                  4        4  #90, 700
  nz=2                        3        0  #0, 1
  nz>=200                     6        5  #69, 400
  run=3                      82       82  #14, 46
  run=4                      39       39  #56, 300
  run=7                      10       10  #58, 300
  run=8                       6        6  #57, 300
  stored-tie                  3        0  #4, 18
  stored<                     3        0  #52, 120
  zrun=10                    54       54  #11, 38
  zrun=11                    37       37  #16, 49
  zrun=138                    4        4  #58, 300
  zrun=139                    3        3  #56, 300
  zrun=2                    109      109  #12, 41
  zrun=3                     99       99  #9, 30
  wanted: ll-overflow: 0 values (not reached: DESIGN.md, "Trees kernel conformance")
  wanted: d-overflow: 0 values
  wanted: hclen=other: 4 values (hclen=15)

nz = 2 (one to three equal bytes) cannot be a dynamic block, nor can a stored or fixed block show one: dynamic 0.
(printed by `pytest -s tests/test_trees_model.py::test_corpus_covers_every_block_plan_arm`.)

Routes: the batch shapes of the GPU test go through tests/host/plan_check's `route` mode and must reach the split
pipeline with the pass capacity that selects the trees instance they are meant for (run_split_pass, pmc_capi.hip:
pcap <= 1024 launches the kTreesCap1K instance, any other the kTreesCap one), the one-kernel path and the
switches' routes -- a shape that no longer reaches its route fails here instead of passing on another route there.

Reference members: the oracle, greedy walk and dynamic-programming walk alike, reproduces the reference's own member
of every value (tests/golden/trees_golden.json)."""
import pytest

import trees_values as TV
from test_host_plan import EXACT, plan_bin, routes, row  # noqa: F401  (plan_bin: a fixture)


@pytest.fixture(scope="module")
def corpus():
    """[(value, the oracle's member, its block facts, its classes)], computed once."""
    caps = TV.capacities()
    out = []
    for v in TV.values():
        m, f = TV.facts_of(v)
        out.append((v, m, f, TV.classes_of(v, m, f, caps)))
    return out


def test_capacities_come_from_the_build():
    cap1k, cap, hdr = TV.capacities()
    # the staged lengths row needs 80 heap slots (static_assert in trees_value), the large heap holds every symbol
    assert 79 <= cap1k <= cap < 286 and cap - cap1k >= 4  # (>= 4 apart: CAP - 1 .. CAP + 2 of the two do not overlap)
    assert hdr == 512 and set(TV.DYN_LENGTHS) == {hdr - 1, hdr, hdr + 1, hdr + 2}


def test_every_value_is_one_block(corpus):
    assert len(corpus) == len(TV.PARAMS) >= 100
    for k, (v, m, f, _) in enumerate(corpus):
        assert 1 <= len(v) <= TV.MAX_LEN and b"\0" not in v, k
        assert f["symbols"] < TV.MAX_SYMBOLS and f["stored_len"] == len(v), k  # (facts_of: exactly one block)
    assert max(len(v) for v, _, _, _ in corpus) == TV.MAX_LEN


def test_facts_agree_with_the_members(corpus):
    """The facts are what the member shows: block type, and for a dynamic block hlit, hdist and hclen
    (classes_of asserts those three)."""
    import deflate_dissect
    from oracle import pyoracle as O
    for k, (v, m, f, _) in enumerate(corpus):
        assert (m[10] >> 1) & 3 == f["type"] and m[10] & 1 == 1, k
        if len(v) <= 600:  # (the dissector decodes bit by bit: the short values suffice for the token count)
            (blk,) = deflate_dissect.dissect(m)
            assert f["type"] == 0 or len(blk["tokens"]) == f["symbols"], k
    # both walks leave the same facts
    for k in (0, len(corpus) // 2, len(corpus) - 1):
        v, m, f, _ = corpus[k]
        assert O.compress(v, dp=True) == m and O.last_block_facts() == [f], k


def test_corpus_covers_every_block_plan_arm(corpus):
    need = TV.required()
    have = {}
    for k, (v, _, _, cl) in enumerate(corpus):
        for c in cl:
            have.setdefault(c, []).append(k)
    other = sorted(c for c in have if c.startswith("hclen=") and int(c[6:]) not in TV.HCLENS)
    print(f"\n  {'class':<22}{'values':>7}{'dynamic':>9}  example (index, bytes)")
    for c in sorted(set(need) | set(have)):
        if c.endswith(":dyn"):
            continue
        ks = have.get(c, [])
        dyn = sum(1 for k in ks if corpus[k][2]["type"] == 2)
        ex = f"#{ks[0]}, {len(corpus[ks[0]][0])}" if ks else "-"
        print(f"  {c:<22}{len(ks):>7}{dyn:>9}  {ex}")
    for c in TV.WANTED:  # reported, never asserted
        n = sum(len(have[o]) for o in other) if c == "hclen=other" else len(have.get(c, []))
        print(f"  wanted: {c}: {n} values" + (f" ({', '.join(other)})" if c == "hclen=other" and other else ""))
    short = {c: (len(have.get(c, [])), n) for c, n in need.items() if len(have.get(c, [])) < n}
    assert not short, short


def test_gpu_batches_hold_what_they_are_meant_for(corpus):
    vs = TV.values()
    cap1k, cap, _ = TV.capacities()
    nz = [f["leaves"][0] for _, _, f, _ in corpus]
    for name, c in (("1k", cap1k), ("16k", cap)):
        idx = TV.batch(name)
        # above the one-kernel path's 1024 values; from 4096 values a chunk is visited in cO order
        assert len(idx) >= 4096 and idx == TV.batch(name)
        assert max(len(vs[i]) for i in idx) == (TV.ONE_K if name == "1k" else TV.MAX_LEN)
        want = set(range(len(vs))) if name == "16k" else {i for i, v in enumerate(vs) if len(v) <= TV.ONE_K}
        assert set(idx) == want
        # both sides of the capacity in one batch: the first pass and the deferred list both get work
        assert any(nz[i] == c for i in idx) and any(nz[i] == c + 1 for i in idx)
        # shuffled: most waves (64 consecutive values) hold a heap of under 20 entries beside one of over 60
        waves = [idx[w:w + 64] for w in range(0, len(idx), 64)]
        mixed = sum(1 for w in waves if min(nz[i] for i in w) < 20 and max(nz[i] for i in w) > 60)
        assert 4 * mixed >= 3 * len(waves), (name, mixed, len(waves))
    mono = TV.batch("mono")
    assert 100 <= len(mono) <= 1024 and max(len(vs[i]) for i in mono) <= 4096
    assert TV.batch("all") == list(range(len(vs))) and len(vs) <= 1024


def test_every_batch_reaches_its_route(plan_bin):  # noqa: F811
    vs = TV.values()
    n_mono, max_mono = len(TV.batch("mono")), max(len(vs[i]) for i in TV.batch("mono"))
    n_all = len(vs)
    rows = {
        "1k": row(len(TV.batch("1k")), TV.ONE_K, EXACT),
        "16k": row(len(TV.batch("16k")), TV.MAX_LEN, EXACT),
        "mono": row(n_mono, max_mono, EXACT, small=True),
        "v1": row(n_all, TV.MAX_LEN, EXACT, force_v1=1),
        "mono-env": row(n_all, TV.MAX_LEN, EXACT, mono_env=1),
        "latency": row(n_mono, max_mono, EXACT, latency=True),
        "host-all": row(n_all, TV.MAX_LEN, EXACT),
    }
    got = dict(zip(rows, routes(plan_bin, list(rows.values()))))
    # the split pipeline; its pass capacity picks the trees instance: <= 1024 kTreesCap1K, else kTreesCap
    assert (got["1k"]["kind"], got["1k"]["passes"]) == ("split", [[0, 1024, 1024, 0, 0]]), got["1k"]
    assert (got["16k"]["kind"], got["16k"]["passes"]) == ("split", [[0, 16382, 16382, 0, 0]]), got["16k"]
    assert (got["host-all"]["kind"], got["host-all"]["passes"]) == ("split", [[0, 16382, 16382, 0, 0]]), got["host-all"]
    # the one-kernel path: the device entry's small batch, the host entry's latency route, PMC_DEFLATE_MONO
    assert (got["mono"]["kind"], got["mono"]["lds_cut"]) == ("mono", max_mono), got["mono"]
    assert (got["latency"]["kind"], got["latency"]["lds_cut"]) == ("mono", max_mono), got["latency"]
    assert (got["mono-env"]["kind"], got["mono-env"]["cap"]) == ("mono", 16382), got["mono-env"]
    # PMC_DEFLATE_V1: the general kernels by length
    assert (got["v1"]["kind"], got["v1"]["gated"]) == ("v1", 0), got["v1"]


def test_oracle_reproduces_the_reference_members(corpus):
    from oracle import pyoracle as O
    G = TV.TreesGolden()
    vals = [v for v, _, _, _ in corpus]
    assert len(G.vectors) == len(vals)
    assert G.mismatches(vals, [m for _, m, _, _ in corpus]) == []
    assert G.mismatches(vals, [O.compress(v, dp=True) for v in vals]) == [], "dp"

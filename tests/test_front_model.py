"""CPU: what tests/test_gpu_front.py relies on, checked without a GPU.

The corpus of tests/front_values.py decides every level-9 match rule in every front instance that can meet it.
The table below is asserted cell by cell (at least 3 values each; `-`: a cell front_values.unreachable() excludes
by arithmetic, asserted empty where it is a rule; blank: the class is not asked of that group) from the oracle's
search log and rule variants (oracle/pmc_oracle.h).  "v:<rule>": the dp encoder with that one rule altered makes
another member.  Groups are the front instances by batch cap: 512 (runtime layout, 6-bit counts, predicted
windows), 1k (CAPC 1024, the same), 3k (u8 counts), 4k (CAPC 4096, 4-bit counts that saturate at 15, packed S),
16k (u8 counts), big (the large pass: has-candidate bits only).  15 is front_pkb's 4 bits, 32 kPreCandLanes, 96 =
32 + 64 (one step of search()), read from the source by front_values.constants().  v:lazy_lt is excluded everywhere:
zlib's longest_match returns a length above prev_length or none, so `match_length <= prev_length` never meets a tie;
v:lazy_ge (a match as long as the pending one replaces it) is the rule that can be decided, and is.

  class                              512    1k    3k    4k   16k   big
  ex=14                                7     3     9    16    11    24
  ex=15                                7     3    10    16    11    24
  ex=16                                8     4     8    16    11    24
  ex=31                                6     4     9    15    11    18
  ex=32                                4     4     9    13    10    18
  ex=33                                6     4     7    11    10    18
  ex=63                                5     3     6    11    10    16
  ex=64                                4     4     7    12    10    14
  ex=65                                3     4    10    12     8    15
  hops>3                              13    11
  last-lit-after-match                 6     3     3     3     3     6
  last-two-lits                        3     4     4     4     3     7
  lazy-run=1                          10    11    11    17    16    24
  lazy-run=2                           3     5     5    10    10    24
  lazy-run>=3                          4     4     5     8     6    11
  match-to-end                         5     7     7    10    10    13
  nice-not-first                       5     7     8    10    12    14
  p257-258                        wanted     3     3     3     3     3
  pred:first=31,farther-longer         3     3
  pred:first=32,farther-longer         4     3
  pred:first=33,farther-longer         3     3
  sat:15:hash                                           16
  sat:15:nil                                             8
  sat:15:start                                           3
  sat:16:hash                                           14
  sat:16:nil                                             9
  sat:16:start                                           3
  sat:>=32:hash                                         14
  sat:>=32:nil                                          14
  sat:>=32:start                                         8
  symbols>=16383                                                     2
  toofar-replaced                      -     -     -     -     4     9
  v:cap4096_off                        -     -     -     -     3     3
  v:chain_nocap                        -     -     3     3     6     7
  v:collide_free                       -     -     3     3     6     6
  v:first_k=1024                       -     -     3     4     7    10
  v:first_k=15                         8     7    10    16    11    24
  v:first_k=16                         8     7    10    16    11    23
  v:first_k=31                         8     7    10    14    11    18
  v:first_k=32                         8     7    10    14    11    18
  v:first_k=33                         8     7    10    14    11    18
  v:first_k=96                         3     4     9    11     8    14
  v:good_33                            -     -     3     3     3     3
  v:good_off                           -     -     3     3     3     7
  v:lazy_ge                            8     9     8    10    10    24
  v:lazy_lt                            -     -     -     -     -     -
  v:nil_ok                            10     9    11    15    13    19
  v:skip_k=0                          14    14    14    17    16    26
  v:skip_k=1                          14    10    13    17    16    26
  v:skip_k=15                          4     3     9    15    11    22
  v:skip_k=31                          3     4     8    13    10    18
  v:skip_k=32                          3     3     7    13    11    18
  v:skip_k=33                          3     3     8    13     9    18
  v:skip_k=4095                        -     -     -     -     3     4
  v:skip_k=95                          3     3     4     8     6    12
  v:skip_k=96                          3     3     6     7     5    12
  v:tie_far                           13    14    14    17    16    24
  v:too_far_4097                       -     -     -     -     3     4
  v:too_far_ge                         -     -     -     -     3     4
  win-ord>=32                          8     7    10    14    11    18
  win64=                               3     3     3     3     6
  win64>                              14    14    14    17    16
  NUL group: v:nice_258 6 of 6 values (NUL-free values cannot decide it: the bytes past the value are zeros)
(printed, with the unreachable cells' arithmetic and the wanted cells, by
`pytest -s tests/test_front_model.py::test_corpus_decides_every_match_rule`.)

"pred:*", "hops>", "win64=" and "win64>" judge device-shaped behaviour (predicted eval windows, the 64 lanes of an
eval) from zlib-level facts: coverage classes, not proofs.

Routes: every batch shape of the GPU test goes through tests/host/plan_check's `route` mode and must reach its route
with the pass cap whose front instance (front_cap_class) and chain-count field (front_pkb) the group is named for.
Reference members: the oracle, greedy walk and dynamic-programming walk alike, reproduces the reference's own member
of every value (tests/golden/front_golden.json; libz's for the NUL group).  The search log agrees with the members:
its tokens rebuild every value, and equal the dissected member's tokens for the values of at most 600 bytes."""
import time
import zlib

import numpy as np
import pytest

import front_values as FV
from test_host_plan import EXACT, plan_bin, routes, row  # noqa: F401  (plan_bin: a fixture)

_TOOK = {}


@pytest.fixture(scope="module")
def corpus():
    """[(value, the oracle's member, search records, token records, classes)], computed once."""
    t0 = time.perf_counter()
    out = []
    for v in FV.values():
        m, s, t = FV.facts_of(v)
        out.append((v, m, s, t, FV.classes_of(v, m, s, t)))
    _TOOK["corpus"] = time.perf_counter() - t0
    return out


@pytest.fixture(scope="module")
def nul_corpus():
    out = []
    for v in FV.nul_values():
        m, s, t = FV.facts_of(v)
        out.append((v, m, s, t, FV.classes_of(v, m, s, t, nul=True)))
    return out


def test_constants_come_from_the_build():
    c = FV.constants()
    # 4 bits saturate below the eval's lanes; the prediction's cap is good_length, where the chain cap drops
    assert c["cmax4"] == 15 < c["lanes"] == 32 and c["step"] == 64 and c["pred_cap"] == 32 and c["hops"] == 3
    assert FV.first_ks() == (15, 16, 31, 32, 33, 96, 1024)
    assert FV.skip_ks() == (0, 1, 15, 31, 32, 33, 95, 96, 4095)
    from boundary_values import BIG_MAX
    from test_host_plan import BIG_LIM, SMALL_LIM
    assert FV.BIG_MAX == BIG_MAX == BIG_LIM and FV.SMALL_MAX == SMALL_LIM


def test_corpus_is_small_and_quick(corpus):
    vs = FV.values()
    assert len(vs) == len(FV.PARAMS) <= 300 and sum(map(len, vs)) <= 2_000_000
    assert _TOOK["corpus"] < 15, _TOOK  # generation is milliseconds beside it
    for k, v in enumerate(vs):
        assert 3 <= len(v) <= FV.BIG_MAX and b"\0" not in v, k
    # the large-pass group is one block each, but for the two values the large pass must hand on
    hbm = FV.hbm_bound()
    assert len(hbm) == 2
    for i in FV.in_group("big"):
        assert (len(corpus[i][3]) >= FV.MAX_SYMBOLS) == (i in hbm), i
    assert all(b"\0" in v for v in FV.nul_values())


def test_corpus_decides_every_match_rule(corpus, nul_corpus):
    need, un = FV.required(), FV.unreachable()
    have = {}
    for k, (v, _, _, _, cl) in enumerate(corpus):
        g = FV.group_of(len(v))
        for c in cl:
            have.setdefault((g, c), []).append(k)
    classes = sorted({c for _, c in need} | {c for _, c in un} | {c for _, c in FV.WANTED_CELLS})
    print(f"\n  {'class':<32}" + "".join(f"{g:>6}" for g in FV.GROUP_NAMES))
    for c in classes:
        cells = []
        for g in FV.GROUP_NAMES:
            n = len(have.get((g, c), []))
            cells.append("-" if (g, c) in un else "wanted" if (g, c) in FV.WANTED_CELLS and not n
                         else str(n) if (g, c) in need or (g, c) in FV.WANTED_CELLS else "")
        print(f"  {c:<32}" + "".join(f"{x:>6}" for x in cells))
    nice = [k for k, (_, _, _, _, cl) in enumerate(nul_corpus) if "v:nice_258" in cl]
    print(f"  NUL group: v:nice_258 {len(nice)} of {len(nul_corpus)} values")
    for (g, c), why in sorted(un.items()):
        print(f"  unreachable {g:>4} {c}: {why}")
    for (g, c), why in sorted(FV.WANTED_CELLS.items()):
        print(f"  wanted {g:>4} {c}: {len(have.get((g, c), []))} values ({why})")
    short = {cell: (len(have.get(cell, [])), n) for cell, n in need.items() if len(have.get(cell, [])) < n}
    assert not short, short
    # a rule's cell that arithmetic excludes is empty indeed, and no cell is both asked and excluded
    assert not [cell for cell in un if have.get(cell)], [cell for cell in un if have.get(cell)]
    assert not set(un) & set(need)
    # every variant is decisive in every group or excluded there
    for name, _, _ in FV.variants():
        for g in FV.GROUP_NAMES:
            assert ((g, name) in need) != ((g, name) in un), (g, name)
    # the 4096 cap itself is decided where it can be met
    assert ("16k", "v:cap4096_off") in need and ("big", "v:cap4096_off") in need
    assert len(nice) >= 3
    # NUL-free values cannot decide nice_258 (the compare meets a zero past the value and a non-zero in it)
    from oracle import pyoracle as O
    for k in (0, len(corpus) // 2, len(corpus) - 1):
        assert O.compress_variant("nice_258", 0, corpus[k][0]) == corpus[k][1], k


def test_prefilter_is_sound(corpus):
    """variant_could_differ spares classes_of most variant runs; where it says no, the variant's member is the
    true one (checked on every value of at most 4096 bytes)."""
    from oracle import pyoracle as O
    for k, (v, m, s, _, _) in enumerate(corpus):
        if len(v) > 4096:
            continue
        for name, rule, arg in FV.variants():
            if not FV.variant_could_differ(rule, arg, s):
                assert O.compress_variant(rule, arg, v) == m, (k, name)


def test_oracle_reproduces_the_reference_members(corpus, nul_corpus):
    from oracle import pyoracle as O
    G = FV.FrontGolden()
    vals = [c[0] for c in corpus] + [c[0] for c in nul_corpus]
    assert len(G.vectors) == len(vals)
    assert G.mismatches(vals, [c[1] for c in corpus] + [c[1] for c in nul_corpus]) == [], "dp"
    assert G.mismatches(vals, [O.compress(v) for v in vals]) == [], "greedy"
    if zlib.ZLIB_RUNTIME_VERSION == "1.2.11":  # this interpreter's libz, where it is the reference's version
        for k, v in enumerate(vals):
            z = zlib.compressobj(9, zlib.DEFLATED, 31, 8, 0)
            assert z.compress(v) + z.flush() == (corpus + nul_corpus)[k][1], k


def test_search_log_agrees_with_the_members(corpus, nul_corpus):
    import deflate_dissect
    from oracle import pyoracle as O
    for k, (v, m, s, t, _) in enumerate(corpus + nul_corpus):
        # the tokens tile the value and rebuild it
        pos, ln, dist = t["pos"].astype(np.int64), t["len"].astype(np.int64), t["dist"].astype(np.int64)
        step = np.where(ln > 0, ln, 1)
        assert pos[0] == 0 and (pos[1:] == pos[:-1] + step[:-1]).all() and pos[-1] + step[-1] == len(v), k
        out = bytearray()
        for p, l, d in zip(pos.tolist(), ln.tolist(), dist.tolist()):
            if l == 0:
                out.append(d)
            else:
                assert 3 <= l <= 258 and 1 <= d <= p, (k, p)
                for _ in range(l):
                    out.append(out[-d])
        assert bytes(out) == v, k
        # every match is the winner of a search of the log, taken over the pending one
        sp = {int(r["pos"]): r for r in s[(s["win_len"] > s["prev_length"]) & (s["win_len"] >= 3)]}
        for p, l, d in zip(pos[ln > 0].tolist(), ln[ln > 0].tolist(), dist[ln > 0].tolist()):
            r = sp[p]
            assert (int(r["win_len"]), int(r["win_dist"])) == (l, d), (k, p)
            assert r["examined"] > r["win_ord"] and r["first_len"] <= r["win_len"], (k, p)
        # the walk's end and its count agree: a cap ends it at that many candidates
        assert (s["examined"][s["end"] == O.END_CAP4096] == 4096).all(), k
        assert (s["examined"][s["end"] == O.END_CAP1024] == 1024).all() and \
               (s["prev_length"][s["end"] == O.END_CAP1024] >= 32).all(), k
        assert (s["examined"] <= np.where(s["prev_length"] >= 32, 1024, 4096)).all(), k
        if len(v) <= 600:
            toks = [x for blk in deflate_dissect.dissect(m) for x in blk.get("tokens", [])]
            mine = [int(d) if l == 0 else (int(l), int(d)) for l, d in zip(ln.tolist(), dist.tolist())]
            if any(blk["type"] == 0 for blk in deflate_dissect.dissect(m)):
                continue  # (a stored block shows no tokens)
            assert toks == mine, k


def test_gpu_batches_hold_what_they_are_meant_for(corpus):
    vs = FV.values()
    for name, lo, hi, capc, pkb in FV.GROUPS[:5]:
        idx = FV.batch(name)
        assert idx == FV.batch(name) and set(idx) == set(FV.in_group(name)) and len(FV.in_group(name)) >= 10
        assert len(idx) == (FV.N_16K if name == "16k" else FV.N_SPLIT) and (name == "16k" or len(idx) > 1024)
        assert lo <= min(len(vs[i]) for i in idx) and max(len(vs[i]) for i in idx) == hi, name
        # shuffled: a wave of the eval's 64 consecutive values holds short and long chains side by side
        assert idx != sorted(idx)
    big, hbm = FV.batch("big"), FV.batch("big-hbm")
    assert len(big) + 2 == len(hbm) <= 2 * 256 and set(hbm) - set(big) == set(FV.hbm_bound())
    assert max(len(vs[i]) for i in big) == FV.BIG_MAX and min(len(vs[i]) for i in big) == FV.SMALL_MAX + 1
    mono = FV.batch("mono")
    assert 40 <= len(mono) <= 1024 and max(len(vs[i]) for i in mono) == 4096
    assert FV.batch("all") == list(range(len(vs))) and len(vs) <= 2 * 256


def test_every_batch_reaches_its_route(plan_bin):  # noqa: F811
    vs = FV.values()
    rows, want_front = {}, {}
    for name, lo, hi, capc, pkb in FV.GROUPS[:5]:
        idx = FV.batch(name)
        rows[name] = row(len(idx), max(len(vs[i]) for i in idx), EXACT)
        want_front[name] = (capc, pkb)
    n_big, n_hbm, n_mono, n_small, n_all = (len(FV.batch(b)) for b in ("big", "big-hbm", "mono", "small", "all"))
    rows.update({
        "big": row(n_big, FV.BIG_MAX, EXACT),
        "big-hbm": row(n_hbm, FV.BIG_MAX, EXACT),
        "mono": row(n_mono, 4096, EXACT, small=True),
        "latency": row(n_mono, 4096, EXACT, latency=True),
        "host-all": row(n_all, FV.BIG_MAX, EXACT),
        "v1": row(n_small, FV.SMALL_MAX, EXACT, force_v1=1),
        "mono-env": row(n_small, FV.SMALL_MAX, EXACT, mono_env=1),
    })
    got = dict(zip(rows, routes(plan_bin, list(rows.values()))))
    for name, lo, hi, capc, pkb in FV.GROUPS[:5]:
        g = got[name]
        cap = min((hi + 63) & ~63, FV.SMALL_MAX)
        assert (g["kind"], g["passes"], g["lv"]) == ("split", [[0, hi, cap, 0, 0]], 0), (name, g)
        # the pass cap picks the front instance and its chain-count field
        assert (FV.front_cap_class(g["passes"][0][2]), FV.front_pkb(g["passes"][0][2])) == want_front[name], name
    # the large pass: a small pass for nothing (no value of at most 16382 bytes) and the large one; values it
    # declines go to the gated HBM kernel (rlist)
    for name in ("big", "big-hbm", "host-all"):
        g = got[name]
        assert (g["kind"], g["passes"]) == ("split", [[0, 16382, 16382, 0, 0], [16382, FV.BIG_MAX, FV.BIG_MAX, 0, 0]]), g
        assert (g["lv"], g["gated"], g["rlist"], g["hbm_cut"]) == (0, 1, 1, FV.BIG_MAX), g
        assert (FV.front_cap_class(FV.BIG_MAX), FV.front_pkb(FV.BIG_MAX)) == (0, -1)
    # the one-kernel path: the device entry's small batch, the host entry's latency route, PMC_DEFLATE_MONO
    assert (got["mono"]["kind"], got["mono"]["lds_cut"]) == ("mono", 4096), got["mono"]
    assert (got["latency"]["kind"], got["latency"]["lds_cut"]) == ("mono", 4096), got["latency"]
    assert (got["mono-env"]["kind"], got["mono-env"]["cap"]) == ("mono", 16382), got["mono-env"]
    # PMC_DEFLATE_V1: the general kernels by length
    assert (got["v1"]["kind"], got["v1"]["gated"]) == ("v1", 0), got["v1"]

"""CPU: what tests/test_gpu_large_conf.py relies on, checked without a GPU.

The corpus of tests/large_conf_values.py decides the rules of the large-value pipeline (csrc/pmc_deflate_large.hip)
that no value of at most deflate_big_limit() bytes can meet, and re-decides the front's rules in that pipeline's own
copies of them.  The class table is asserted cell by cell (large_conf_values.required(): at least 3 values each) from the oracle's facts: its search and token logs, its rule variants
(oracle/pmc_oracle.h) and oracle_parse_from, read through tests/large_model.py.  The table, the arithmetic of the
unreachable cells and the wanted ones are printed by `pytest -s tests/test_large_model.py::test_class_table`.

What arithmetic excludes (large_conf_values.unreachable(), asserted empty on the corpus):
  v:max_lazy_off   longest_match returns at most 258 = prev_length, which deflate_slow ignores
  v:stored_any     a block whose start has left the window spans more than MAX_DIST bytes in at most 16383 symbols;
                   the fixed trees then undercut the stored form, so the window base never decides a stored block
  v:maxdist_*@seg0 a search below 16384 has no candidate that far back
What is decidable against expectation: v:slide_nil_off.  The window base hides only what the distance limit hides
at every loop top but one: the loop top that slides with the base exactly 32768 + MAX_DIST behind, which only the
last MIN_LOOKAHEAD - 1 positions of a value can be.  There the new base is the candidate at MAX_DIST, and NIL
(large_model.base_hides).  v:slide_early and v:slide_late are decided at the same place, through that NIL.

Tokens: the model's spliced tokens equal the oracle's token log for every value that stitches; HC: the model's
count is non-zero exactly where the oracle's search examined a candidate; base: the closed form equals the base the
dp encoder keeps step by step at every loop top.  Agreement: the oracle's member (greedy and dp walk), the
reference's recorded member (tests/golden/large_conf_golden.json) and, where its runtime is 1.2.11, Python's zlib.
Fallback: the model fails exactly large_conf_values.FALLBACK.  Routes and rounds: every batch shape of the GPU test
goes through tests/host/plan_check."""
import time
import zlib

import numpy as np
import pytest

import front_values as FV
import large_conf_values as LC
import large_model as LM
from test_host_plan import EXACT, Exact, Fast, plan_bin, routes, row, run_lv  # noqa: F401  (plan_bin: a fixture)

_TOOK = {}


@pytest.fixture(scope="module")
def corpus():
    """[(value, the oracle's member, search records, token records, classes, the model's stitch)], computed once."""
    t0 = time.perf_counter()
    out = []
    for i, v in enumerate(LC.values()):
        m, s, t = LC.facts_of(v)
        from oracle import pyoracle as O
        assert O.base_diffs() == 0, i  # the closed form is the step-by-step base at every loop top
        st = LC.stitched(i)
        out.append((v, m, s, t, LC.classes_of(v, m, s, t, stitched=st), st))
    _TOOK["corpus"] = time.perf_counter() - t0
    print(f"\n  corpus: {len(out)} values classified in {_TOOK['corpus']:.1f} s")
    return out


def test_constants_come_from_the_build():
    c = LM.constants()
    assert (c["seg"], c["overlap"], c["chunk"]) == (16384, 2048, 4096) and LC.SEG == c["seg"]
    assert LM.MAX_DIST == 32506 and LM.SLIDE_AT == 65274
    from test_host_plan import BIG_LIM
    assert LC.BIG_MAX == BIG_LIM
    assert [LM.nseg(n) for n in (16383, 32767, 32768, 49151, 49152, 65536)] == [1, 1, 2, 2, 3, 4]
    for n in (32768, 40000, 49151, 135000):  # the last segment holds 16384 .. 32767 positions
        s, e, eo, last = LM.segments(n)[-1]
        assert last and e == eo == n and 16384 <= n - s <= 32767


def test_corpus_is_small_and_quick(corpus):
    vs = LC.values()
    # (96 values: three per length around a multiple of the segment and three per look-back alone are 27 of them)
    assert len(vs) == len(LC.PARAMS) <= 100 and sum(map(len, vs)) <= 6_000_000
    for k, v in enumerate(vs):
        assert LC.BIG_MAX < len(v) <= 140_000 and b"\0" not in v, k
    assert max(map(len, vs)) > 131072
    assert all(b"\0" in v and len(v) > LC.BIG_MAX for v in LC.nul_values())
    # the values the HBM kernel redoes: few and short
    assert len(LC.FALLBACK) <= 8 and all(len(vs[i]) <= 70_000 for i in LC.FALLBACK)
    assert _TOOK["corpus"] < 60, _TOOK


def test_class_table(corpus):
    need, un = LC.required(), LC.unreachable()
    have = {}
    for k, c in enumerate(corpus):
        for name in c[4]:
            have.setdefault(name, []).append(k)
    print(f"\n  {'class':<36}{'values':>7}{'least':>7}")
    for name in sorted(set(need) | set(un) | set(LC.WANTED)):
        n = len(have.get(name, []))
        print(f"  {name:<36}{'-' if name in un else n:>7}{need.get(name, 'wanted' if name in LC.WANTED else ''):>7}")
    for name, why in sorted(un.items()):
        print(f"  unreachable {name}: {why}")
    for name, why in sorted(LC.WANTED.items()):
        print(f"  wanted {name}: {len(have.get(name, []))} values ({why})")
    short = {name: (len(have.get(name, [])), n) for name, n in need.items() if len(have.get(name, [])) < n}
    assert not short, short
    assert not [name for name in un if have.get(name)], [name for name in un if have.get(name)]
    assert not set(un) & set(need) and not set(LC.WANTED) & set(need)
    # every rule the issue names is asked for, or excluded by arithmetic, in every zone it names
    for r in LC.DIST_RULES:
        assert f"v:{r}@seg0" in un and f"v:{r}@mid" in need and f"v:{r}@slid" in need
    for r in LC.FRONT_RULES:
        assert (f"v:{r}@seg0" in need and f"v:{r}@mid" in need) != (f"v:{r}" in un), r
    assert "v:stored_any" in un and "v:slide_nil_off" in need
    # a distance rule and the base's NIL are met by the HBM kernel too: in values that fail a stitch
    for name in ("fallback+v:maxdist_first_lt", "fallback+v:maxdist_later_le", "fallback+v:slide_nil_off"):
        assert have.get(name), name
    # the window base's NIL at the first slide (two value lengths at least) and at the second
    nil = have["v:slide_nil_off"]
    assert {len(corpus[k][0]) < 65536 for k in nil} == {True, False} and len({len(corpus[k][0]) for k in nil}) >= 3
    assert any("v:slide_nil_off@slid" in corpus[k][4] for k in nil)


def test_nul_group():
    from oracle import pyoracle as O
    n = 0
    for v in LC.nul_values():
        m, s, t = LC.facts_of(v)
        n += O.compress_variant("nice_258", 0, v) != m
        assert m == O.compress(v)
    assert n >= 3


def test_spliced_tokens_are_the_serial_parse(corpus):
    for k, (v, m, s, t, cl, st) in enumerate(corpus):
        assert len(st.parses) == LM.nseg(len(v)), k
        if st.failed:
            continue
        got = st.tokens()
        assert len(got) == len(t) and (got == t).all(), k
        # a middle segment's range is cut at both ends
        for j, (a, b) in enumerate(st.ranges):
            assert 0 <= a <= b <= len(st.parses[j].tokens), (k, j)
    # values of 3 and of 5 or more segments whose middle segments are cut at both ends
    cut = [k for k, c in enumerate(corpus) if not c[5].failed and len(c[5].ranges) >= 5
           and all(a > 0 and b < len(p.tokens) for (a, b), p in list(zip(c[5].ranges, c[5].parses))[1:-1])]
    assert len(cut) >= 3, cut


def test_wrong_stitches_are_told_apart(corpus):
    """Two wrong pipelines the GPU is not asked to run (they change token ranges): a stitch that takes the first
    offset where both parses recorded any state, and a literal-run path that records code 2 whatever is pending.
    Each makes other tokens than zlib for at least 3 values of the corpus."""
    for kw in ({"relaxed": True}, {"run_code2": True}):
        wrong = []
        for k, (v, m, s, t, cl, st) in enumerate(corpus):
            if st.failed or ("relaxed" in kw and "stitch-clash" not in cl):
                continue
            w = LM.Stitched(v, **kw)
            if w.failed or w.found != st.found:
                got = None if w.failed else w.tokens()
                if got is None or len(got) != len(t) or not (got == t).all():
                    wrong.append(k)
        print(f"\n  {kw}: other tokens for values {wrong[:16]} ({len(wrong)})")
        assert len(wrong) >= 3, (kw, wrong)


def test_hc_is_where_zlib_searches(corpus):
    """The model's HC (what lv_rank_kernel must compute) is non-zero exactly at the positions where the oracle's
    search examined a candidate, for every search of every value's true parse; and it is the chain's length."""
    for k, (v, m, s, t, cl, st) in enumerate(corpus):
        hc, S = LM.hc_of(v)
        pos = s["pos"].astype(np.int64)
        assert ((hc[pos] != 0) == (s["examined"] >= 1)).all(), k
        full = (s["end"] == 0) | (s["end"] == 1) | (s["end"] == 2)  # the walk took the whole chain
        few = full & (s["examined"] < 255)
        assert (hc[pos][few] >= s["examined"][few]).all(), k
        # base_hides names a position of the corpus: the model's rule is not vacuous
    hidden = [k for k, c in enumerate(corpus) if any(LM.base_hides(int(p), len(c[0])) and x == 0 and e == 2
              for p, x, e in zip(c[2]["pos"], c[2]["examined"], c[2]["end"]))]
    assert len(hidden) >= 3, hidden


def test_window_base_closed_form():
    from oracle import pyoracle as O
    for n in (65274, 65275, 65400, 65535, 65536, 65537, 98042, 98200, 98304, 140000):
        for t in {0, 65273, 65274, 65275, 98041, 98042, 98043, n - 262, n - 261, n - 1, n}:
            if 0 <= t <= n:
                assert LM.window_base(t, n) == O.window_base(t, n), (t, n)
                hid = t - LM.MAX_DIST >= 1 and t - LM.MAX_DIST <= LM.window_base(t, n)
                assert hid == LM.base_hides(t, n), (t, n)


def test_members_agree(corpus):
    from oracle import pyoracle as O
    G = LC.LargeConfGolden()
    vals = [c[0] for c in corpus] + LC.nul_values()
    dp = [c[1] for c in corpus] + [O.compress(v, dp=True) for v in LC.nul_values()]
    assert len(G.vectors) == len(vals)
    assert G.mismatches(vals, dp) == [], "dp"
    assert G.mismatches(vals, [O.compress(v) for v in vals]) == [], "greedy"
    if zlib.ZLIB_RUNTIME_VERSION == "1.2.11":
        for k, v in enumerate(vals):
            z = zlib.compressobj(9, zlib.DEFLATED, 31, 8, 0)
            assert z.compress(v) + z.flush() == dp[k], k


def test_fallback_list(corpus):
    assert LC.fallback() == LC.FALLBACK == tuple(k for k, c in enumerate(corpus) if c[5].failed)
    assert set(LC.batch("lv")) - set(LC.batch("lv-stitched")) == set(LC.FALLBACK)


def test_batches(corpus):
    vs = LC.values()
    assert LC.batch("lv") == list(range(len(vs)))
    mixed = LC.batch("lv-mixed")
    idx = [x for x in mixed if isinstance(x, int)]
    assert sorted(idx) != idx and len(idx) == len(vs) + 3 and len(set(idx)) == len(vs)
    assert len([x for x in mixed if isinstance(x, bytes)]) >= 30
    # unaligned: every residue of the address is met by large values, and every value that ends in a match is
    # followed by bytes that would lengthen it
    tails = LC.ends_in_match()
    assert len(tails) >= 3
    for first in (1, 2, 3):
        items = LC.batch(f"lv-unaligned-{first}")
        vals = LC.batch_values(items)
        assert len(vals[0]) == first
        off = np.concatenate([[0], np.cumsum([len(v) for v in vals])[:-1]])
        assert {int(o) & 3 for o, x in zip(off, items) if isinstance(x, int)} == {0, 1, 2, 3}, first
        for k, x in enumerate(items):
            if isinstance(x, int) and x in tails:
                v, nxt = vals[k], vals[k + 1]
                t = corpus[x][3]
                src = len(v) - int(t["dist"][-1])
                assert nxt[:1] == v[src:src + 1] and len(nxt) >= 1, x


def test_every_batch_reaches_its_route(plan_bin):  # noqa: F811
    vs = LC.values()
    big = [FV.values()[i] for i in FV.batch("big")]
    rows = {
        "lv": row(len(vs), max(map(len, vs)), EXACT),
        "lv-mixed": row(len(LC.batch("lv-mixed")), max(map(len, vs)), EXACT),
        "lv-unaligned": row(len(LC.batch("lv-unaligned-1")), max(map(len, vs)), EXACT),
        "host": row(len(vs), max(map(len, vs)), EXACT),  # (the host entry's pipeline route plans as the device entry)
        "nul": row(len(LC.nul_values()), max(map(len, LC.nul_values())), EXACT),
        "nul-unaligned": row(len(LC.nul_values()) + 1, max(map(len, LC.nul_values())), EXACT),
        "big-pass-off": row(len(big) + 1, FV.BIG_MAX, EXACT, big_env=0),
        "big-default": row(len(big) + 1, FV.BIG_MAX, EXACT),
    }
    got = dict(zip(rows, routes(plan_bin, list(rows.values()))))
    for name in ("lv", "lv-mixed", "lv-unaligned", "host", "nul", "nul-unaligned", "big-pass-off"):
        g = got[name]
        # no large pass: the large-value pipeline takes every value above 16382 bytes
        assert (g["kind"], g["passes"], g["lv"], g["hbm_cut"]) == ("split", [[0, 16382, 16382, 0, 0]], 1, 16382), (name, g)
    assert got["big-default"]["lv"] == 0  # (without the switch the one-segment values take the large pass)


def test_fast_round_plan(plan_bin, golden):  # noqa: F811
    """The fast-all child's budget cuts the values of tests/test_gpu_fast_large.py into at least 3 rounds too."""
    from fast_large_values import large_values
    vals = [(i, len(v)) for i, (_, v) in enumerate(large_values(golden.corpus))]
    rounds, _ = run_lv(plan_bin, Fast, vals, LC.FAST_ROUND_MB << 20, "conf_fast")
    assert len(rounds) >= 3 and sum(r["nv"] for r in rounds) == len(vals) and max(r["nv"] for r in rounds) >= 2


def test_host_entry_takes_the_pipeline(plan_bin):  # noqa: F811
    """The host entry's own plan (plan_check `host`): the corpus is no latency batch, so compress_many takes the
    pipeline route, whose device call test_every_batch_reaches_its_route routes."""
    import json
    import subprocess
    vs = LC.values()
    # compress level lane_order_ok force_pipeline cus lat_batch lat_max_len out_limit, then count src_len dst_cap
    from oracle import pyoracle as O
    line = "1 9 1 0 256 1024 4096 0 " + " ".join(f"1 {len(v)} {O.bound(len(v))}" for v in vs)
    out = subprocess.run([plan_bin[0], "host"], input=line + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    p = json.loads(out.stdout)
    assert (p["latency"], p["path"], p["max_len"]) == (0, 2, max(map(len, vs))), p  # (path 2: pipeline compress)


def test_round_plan(plan_bin):  # noqa: F811
    """PMC_LV_ROUND_MB = ROUND_MB cuts the "lv" batch into at least 3 rounds, one of which holds a failing value
    that is not its last; the default budget takes it in one."""
    vs = LC.values()
    vals = [(i, len(v)) for i, v in enumerate(vs)]
    one, _ = run_lv(plan_bin, Exact, vals, 24 << 30, "conf_one")
    assert len(one) == 1 and one[0]["nv"] == len(vs)
    rounds, _ = run_lv(plan_bin, Exact, vals, LC.ROUND_MB << 20, "conf_rounds")
    assert len(rounds) >= 3 and sum(r["nv"] for r in rounds) == len(vs)
    assert any(r["v0"] <= f < r["v1"] - 1 for r in rounds for f in LC.FALLBACK), rounds
    assert all(r["scratch_bytes"] <= (LC.ROUND_MB << 20) + (1 << 20) or r["nv"] == 1 for r in rounds)
    print(f"\n  rounds at {LC.ROUND_MB} MB: {[(r['v0'], r['v1']) for r in rounds]}")

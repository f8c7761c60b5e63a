"""GPU: the large-value pipeline's rules (csrc/pmc_deflate_large.hip), against the oracle, on the corpus of
tests/large_conf_values.py.

Values above deflate_big_limit() are sorted by hash in HBM (lv_rank_kernel: HC counts, their cap, the look-back),
parsed speculatively segment by segment (LvParse::search, lv_parse_kernel), stitched (lv_stitch_kernel) and emitted
(deflate_lv_emit_kernel); a value that fails a stitch is redone by the gated HBM kernel.  That code holds its own
copies of the front's comparisons and the two MAX_DIST comparisons no smaller value can reach, and is checked only
through the bytes of the values a test compresses.  These values were built so that each of those rules decides a
byte of some member: tests/test_large_model.py (CPU) asserts that coverage, the model's list of failing values, the
routes and the round plan, and holds the oracle's members to the reference's (tests/golden/large_conf_golden.json).

Every member is compared byte for byte with the oracle's; a mismatch is explained by deflate_dissect.explain and
names the parameters and classes of the value.  Every batch is then decompressed back to its values.

  "lv"            every value once: the retry counter grows by exactly the values the model fails, and by nothing
                  on the batch without them
  "lv-unaligned"  pack(align=1) behind a first value of 1, 2 and 3 bytes: every residue of a value's address, a
                  neighbour's bytes in a value's last dword, and behind every value that ends in a match the bytes
                  that would lengthen it
  "lv-mixed"      the values shuffled among small ones (the split pipeline's), three of them twice
  host            pmc_gzip_compress_batch_host on its pipeline route
  NUL             the values that hold NULs
  children        one fresh process per switch: PMC_BIG_PASS=0 (front_values' "big" group and NUL values of that
                  size through the pipeline's one-segment case); PMC_LV_ROUND_MB (the "lv" batch in several
                  rounds: members, retry count and return codes as in one round); the same with the fast-all
                  level on the values of tests/test_gpu_fast_large.py

Measured on an MI355X: see DESIGN.md, "Large-value conformance"."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import front_values as FV
import large_conf_values as LC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


_WANT = {}


def want(v):
    """The oracle's member of a value, computed once."""
    if v not in _WANT:
        from oracle import pyoracle as O
        _WANT[v] = O.compress(v)
    return _WANT[v]


def check_members(tag, items, vals, got, nul=False):
    """got[k] is the member of vals[k]: all equal the oracle's, or the first one that differs is explained."""
    import deflate_dissect
    bad = [k for k, v in enumerate(vals) if got[k] != want(v)]
    if bad:
        k = bad[0]
        v, x = vals[k], items[k]
        what = f"{len(v)} B"
        if isinstance(x, int) and not nul:
            m, s, t = LC.facts_of(v)
            what = f"value #{x}, {len(v)} B, make{LC.PARAMS[x]}, classes {sorted(LC.classes_of(v, m, s, t))}"
        raise AssertionError(f"{tag}: {len(bad)} of {len(vals)} members (items {[items[j] for j in bad][:24]}) differ from "
                             f"the oracle's, first {what}: {deflate_dissect.explain(got[k], want(v))}")


def device_round_trip(ctx, tag, items, vals=None, align=4, nul=False):
    """One pmc_gzip_compress_batch of the items, checked, and one pmc_gzip_decompress_batch back.  Returns the growth
    of the retry counter over the compress call."""
    import torch
    from pmc_codec import device as D
    vals = LC.batch_values(items) if vals is None else vals
    before = ctx.guard_counts()["retry"]
    out, rc = D.compress(ctx, D.pack(vals, align=align))
    torch.cuda.synchronize()
    grew = ctx.guard_counts()["retry"] - before
    assert int((rc != 0).sum()) == 0, (tag, "rc", rc[rc != 0][:8].tolist())
    got = out.host_items()
    check_members(tag, items, vals, got, nul)
    back, brc = D.decompress(ctx, out, [max(len(v), 1) for v in vals])
    torch.cuda.synchronize()
    assert int((brc != 0).sum()) == 0, (tag, "decompress rc", brc[brc != 0][:8].tolist())
    assert back.host_items() == vals, (tag, "round trip")
    return grew


def test_every_value_that_stitches(ctx):
    grew = device_round_trip(ctx, "lv-stitched", LC.batch("lv-stitched"))
    assert grew == 0, ("lv-stitched", "retry counter", grew)


def test_every_value(ctx):
    """With the values the model fails at a boundary: the HBM kernel redoes exactly those."""
    grew = device_round_trip(ctx, "lv", LC.batch("lv"))
    assert grew == len(LC.FALLBACK), ("lv", "retry counter", grew)


@pytest.mark.parametrize("first", [1, 2, 3])
def test_unaligned(ctx, first):
    items = LC.batch(f"lv-unaligned-{first}")
    grew = device_round_trip(ctx, f"lv-unaligned-{first}", items, align=1)
    assert grew == len(LC.FALLBACK), (first, "retry counter", grew)


def test_mixed_with_small_values(ctx):
    items = LC.batch("lv-mixed")
    grew = device_round_trip(ctx, "lv-mixed", items)
    assert grew == sum(1 for x in items if isinstance(x, int) and x in LC.FALLBACK), ("lv-mixed", "retry counter", grew)


def test_host_entry(ctx):
    items = LC.batch("lv")
    vs = LC.batch_values(items)
    before = ctx.path_counts()
    res = ctx.compress_many(vs)
    after = ctx.path_counts()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {"pipeline_compress": 1}, (before, after)
    assert [c for c, _ in res] == [0] * len(vs)
    check_members("host", items, vs, [m for _, m in res])
    back = ctx.decompress_many([m for _, m in res])
    assert [(c, v) for c, v in back] == [(0, v) for v in vs], "round trip"


def test_nul_group(ctx):
    nv = LC.nul_values()
    assert device_round_trip(ctx, "nul", list(range(len(nv))), vals=nv, nul=True) == 0
    assert device_round_trip(ctx, "nul-unaligned", list(range(len(nv) + 1)), vals=[b"x"] + nv, align=1, nul=True) == 0


# ---- children: one fresh process per switch ------------------------------------------------------------------
def _digest(members):
    return [hashlib.sha256(m).hexdigest() for m in members]


def child(which):
    import torch
    import pmc_codec
    from pmc_codec import device as D
    c = pmc_codec.Context(0)
    try:
        if which == "big-pass-off":
            # the one-segment case: values of 16383 .. 31808 bytes through the large-value pipeline
            big = [FV.values()[i] for i in FV.batch("big")]
            nul = [v for v in FV.nul_values() if len(v) > FV.SMALL_MAX]
            assert len(big) >= 20 and nul
            vals = big + nul
            device_round_trip(c, "big-pass-off", list(range(len(vals))), vals=vals, nul=True)
        elif which == "rounds":
            items = LC.batch("lv")
            grew = device_round_trip(c, "rounds", items)
            print("RESULT " + json.dumps({"grew": grew}))
        elif which == "fast-rounds":
            import conftest
            from fast_large_values import large_values
            c.level = pmc_codec.LEVEL_FAST_ALL
            vals = [v for _, v in large_values(conftest.Golden().corpus)]
            out, rc = D.compress(c, D.pack(vals, align=1))
            torch.cuda.synchronize()
            assert int((rc != 0).sum()) == 0
            print("RESULT " + json.dumps({"sha": _digest(out.host_items())}))
        else:
            raise KeyError(which)
    finally:
        c.close()


CHILD = ("import sys; sys.path[:0] = [sys.argv[1]]; import conftest; import test_gpu_large_conf as T; "
         "T.child(sys.argv[2])")


def run_child(which, timeout, **env):
    import torch
    torch.cuda.synchronize()  # (raises if an earlier test left the device in error: then no child is started)
    out = subprocess.run([sys.executable, "-c", CHILD, HERE, which], env=dict(os.environ, **env), capture_output=True,
                         text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(res[-1][7:]) if res else None


def test_one_segment_case(ctx):
    """PMC_BIG_PASS=0: front_values' "big" group, as it stands, takes the large-value pipeline's one-segment case."""
    run_child("big-pass-off", 120, PMC_BIG_PASS="0")


def test_rounds(ctx):
    """PMC_LV_ROUND_MB cuts the "lv" batch into rounds (tests/test_large_model.py: at least 3, a failing value inside
    one): the child holds every member to the oracle's, as the one-round run does, and counts the same retries."""
    res = run_child("rounds", 180, PMC_LV_ROUND_MB=str(LC.ROUND_MB))
    assert res == {"grew": len(LC.FALLBACK)}, res


def test_fast_all_rounds(ctx, golden):
    """The same switch on the fast-all level's rounds, which share the driver: the members of
    tests/test_gpu_fast_large.py's values equal the one-round ones (that test holds those to the model)."""
    import torch
    import pmc_codec
    from fast_large_values import large_values
    from pmc_codec import device as D
    vals = [v for _, v in large_values(golden.corpus)]
    c = pmc_codec.Context(0)
    try:
        c.level = pmc_codec.LEVEL_FAST_ALL
        out, rc = D.compress(c, D.pack(vals, align=1))
        torch.cuda.synchronize()
        assert int((rc != 0).sum()) == 0
        one = _digest(out.host_items())
    finally:
        c.close()
    res = run_child("fast-rounds", 180, PMC_LV_ROUND_MB=str(LC.FAST_ROUND_MB))
    assert res["sha"] == one

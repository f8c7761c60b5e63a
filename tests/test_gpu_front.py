"""GPU: the front's match rules on every level-9 route, against the oracle, on the corpus of tests/front_values.py.

The front (hash sort, longest_match, deflate_slow's lazy walk) is restated by several device instances
(csrc/pmc_deflate_small.hip, pmc_deflate_split.hip) picked by the batch's cap, by search() behind them, by the
one-kernel path and by PMC_DEFLATE_V1, and is checked only through the bytes of the values a test compresses.  These
values were picked so that every rule decides some byte of some member in every instance that can meet it:
tests/test_front_model.py (CPU) asserts that coverage from the oracle's search log and rule variants, holds every
batch shape below to its route, front instance and chain-count field, and the oracle's members to the reference's
(tests/golden/front_golden.json).

Every member is compared byte for byte with the oracle's; a mismatch is explained by deflate_dissect.explain and
names the parameters and classes of the value.  Every batch is then decompressed back to its values.

  "512" "1k" "3k" "4k"   a group's values, shuffled and cycled to 4224: the split pipeline's front instance of that
                         cap (6-bit counts and predicted windows; the same at CAPC 1024; u8 counts; CAPC 4096 with
                         saturating 4-bit counts and packed S)
  "16k"                  the same, cycled to 320: the runtime layout at cap 16382
  "big"                  the large-pass group once: has-candidate bits only, every position cut; then with the two
                         values of at least 16383 symbols, which the large pass must hand to the gated HBM kernel:
                         the retry counter grows by exactly their number, and by nothing on any other split batch
  "mono"                 the values of at most 4096 bytes, once: the one-kernel device path
  host                   pmc_gzip_compress_batch_host: its latency route and, with every value, its pipeline route
  NUL                    the values that hold NULs (one ends in a zero run, where zlib's compare runs past the
                         input), on the split pipeline and the one-kernel path
  PMC_DEFLATE_V1=1, PMC_DEFLATE_MONO=1: every value of at most 16382 bytes, in a child process per switch

Measured on an MI355X: see DESIGN.md, "Front conformance"."""
import os
import subprocess
import sys

import pytest

import front_values as FV

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


def want(nul=False):
    """The oracle's member of every value, computed once."""
    if nul not in _WANT:
        from oracle import pyoracle as O
        _WANT[nul] = [O.compress(v) for v in (FV.nul_values() if nul else FV.values())]
    return _WANT[nul]


def check_members(tag, idx, got, nul=False):
    """got[k] is the member of value idx[k]: all equal the oracle's, or the first one that differs is explained."""
    import deflate_dissect
    w = want(nul)
    bad = [k for k, i in enumerate(idx) if got[k] != w[i]]
    if bad:
        i = idx[bad[0]]
        v = (FV.nul_values() if nul else FV.values())[i]
        m, s, t = FV.facts_of(v)
        params = f"make_nul{FV.NUL_PARAMS[i]}" if nul else f"make{FV.PARAMS[i]}"
        raise AssertionError(f"{tag}: {len(bad)} of {len(idx)} members ({len({idx[k] for k in bad})} values: "
                             f"{sorted({idx[k] for k in bad})[:24]}) differ from the oracle's, first value #{i} "
                             f"({len(v)} B, {params}, classes {sorted(FV.classes_of(v, m, s, t, nul=nul))}): "
                             f"{deflate_dissect.explain(got[bad[0]], w[i])}")


def device_round_trip(ctx, tag, idx, nul=False):
    """One pmc_gzip_compress_batch of the values idx, checked, and one pmc_gzip_decompress_batch back.  Returns
    the growth of the retry counter over the compress call."""
    import torch
    from pmc_codec import device as D
    src = FV.nul_values() if nul else FV.values()
    vs = [src[i] for i in idx]
    before = ctx.guard_counts()["retry"]
    out, rc = D.compress(ctx, D.pack(vs))
    torch.cuda.synchronize()
    grew = ctx.guard_counts()["retry"] - before
    assert int((rc != 0).sum()) == 0, (tag, "rc", rc[rc != 0][:8].tolist())
    check_members(tag, idx, out.host_items(), nul)
    back, brc = D.decompress(ctx, out, [max(len(v), 1) for v in vs])
    torch.cuda.synchronize()
    assert int((brc != 0).sum()) == 0, (tag, "decompress rc", brc[brc != 0][:8].tolist())
    assert back.host_items() == vs, (tag, "round trip")
    return grew


@pytest.mark.parametrize("name", FV.GROUP_NAMES[:5])
def test_split_pipeline_batch(ctx, name):
    grew = device_round_trip(ctx, name, FV.batch(name))
    assert grew == 0, (name, "retry counter", grew)


def test_large_pass(ctx):
    """At most 2 x CUs values and none above deflate_big_limit(): the split pipeline's large pass.  It keeps every
    value of one block and hands the two of at least 16383 symbols to the gated HBM kernel."""
    grew = device_round_trip(ctx, "big", FV.batch("big"))
    assert grew == 0, ("big", "retry counter", grew)
    grew = device_round_trip(ctx, "big-hbm", FV.batch("big-hbm"))
    assert grew == len(FV.hbm_bound()) == 2, ("big-hbm", "retry counter", grew)


def test_one_kernel_device_path(ctx):
    device_round_trip(ctx, "mono", FV.batch("mono"))


def test_nul_group(ctx):
    """The values that hold NULs: once each (the split pipeline with its large pass), and those of at most 4096
    bytes cycled to 4224 (the CAPC 4096 front) and once (the one-kernel path)."""
    nv = FV.nul_values()
    every = list(range(len(nv)))
    small = [i for i in every if len(nv[i]) <= 4096]
    assert device_round_trip(ctx, "nul", every, nul=True) == 0
    assert device_round_trip(ctx, "nul-4k", (small * (FV.N_SPLIT // len(small) + 1))[:FV.N_SPLIT], nul=True) == 0
    device_round_trip(ctx, "nul-mono", small, nul=True)


def test_host_entry(ctx):
    """pmc_gzip_compress_batch_host: the latency route (at most 1024 values of at most 4096 bytes) and, with every
    value, the pipeline route."""
    for name, route in (("mono", "latency_compress"), ("all", "pipeline_compress")):
        idx = FV.batch(name)
        vs = [FV.values()[i] for i in idx]
        before = ctx.path_counts()
        res = ctx.compress_many(vs)
        after = ctx.path_counts()
        assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {route: 1}, (name, before, after)
        assert [c for c, _ in res] == [0] * len(vs), name
        check_members(f"host/{name}", idx, [m for _, m in res])
        back = ctx.decompress_many([m for _, m in res])
        assert [(c, v) for c, v in back] == [(0, v) for v in vs], (name, "round trip")


def child():
    """Every value of at most 16382 bytes once through the device entry, in a process whose switch is set."""
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    try:
        device_round_trip(c, "child", FV.batch("small"))
    finally:
        c.close()


CHILD = "import sys; sys.path[:0] = [sys.argv[1]]; import conftest; import test_gpu_front as T; T.child()"


@pytest.mark.parametrize("switch", ["PMC_DEFLATE_V1", "PMC_DEFLATE_MONO"])
def test_switch(ctx, switch):
    import torch
    torch.cuda.synchronize()  # (raises if an earlier test left the device in error: then no child is started)
    env = dict(os.environ, **{switch: "1"})
    out = subprocess.run([sys.executable, "-c", CHILD, HERE], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]

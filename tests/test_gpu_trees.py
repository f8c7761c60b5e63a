"""GPU: block planning on every level-9 route, against the oracle, on the corpus of tests/trees_values.py.

deflate_trees_kernel (csrc/pmc_deflate_split.hip, LaneTrees) restates zlib's build_tree, gen_bitlen, scan_tree,
build_bl_tree and the stored/fixed/dynamic choice one lane per value, and is checked only through the bytes of the
values a test compresses.  These values were picked so that every arm of that arithmetic decides some byte of some
member: tests/test_trees_model.py (CPU) asserts the coverage from the oracle's block facts, holds every batch shape
below to its route and the oracle's members to the reference's (tests/golden/trees_golden.json).

Every member is compared byte for byte with the oracle's; a mismatch is explained by deflate_dissect.explain and
names the classes of the value.  Every batch is then decompressed back to its values.

  "1k"    the values of at most 1024 bytes, shuffled and cycled to 4224: the split pipeline's kTreesCap1K instance,
          its deferred list and the kLCodes instance that walks it, lanes in cO order
  "16k"   every value, shuffled and cycled to 4224: the kTreesCap instance
  "mono"  the values of at most 4096 bytes, once: the one-kernel device path (a batch of at most 1024 values)
  host    the same through pmc_gzip_compress_batch_host: its latency route, and every value on its pipeline route
  PMC_DEFLATE_V1=1, PMC_DEFLATE_MONO=1: every value, in a child process per switch (read once per process)

All routes must give the same bytes: the wave-per-value tree builder of the other routes (csrc/pmc_trees.hpp) and
the lane builder are two restatements of one arithmetic.  On the split rows the retry counter must not grow: a value
the back declined would be redone by the HBM kernel to the right bytes, and only the counter would tell."""
import os
import subprocess
import sys

import pytest

import trees_values as TV

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    yield c
    c.close()


_WANT = None


def want():
    """The oracle's member of every value, computed once."""
    global _WANT
    if _WANT is None:
        from oracle import pyoracle as O
        _WANT = [O.compress(v) for v in TV.values()]
    return _WANT


def check_members(tag, idx, got):
    """got[k] is the member of value idx[k]: all equal the oracle's, or the first one that differs is explained."""
    import deflate_dissect
    w = want()
    bad = [k for k, i in enumerate(idx) if got[k] != w[i]]
    if bad:
        i = idx[bad[0]]
        v = TV.values()[i]
        m, f = TV.facts_of(v)
        raise AssertionError(f"{tag}: {len(bad)} of {len(idx)} members ({len({idx[k] for k in bad})} values) differ from the "
                             f"oracle's, first value #{i} ({len(v)} B, make{TV.PARAMS[i]}, classes "
                             f"{sorted(TV.classes_of(v, m, f))}): {deflate_dissect.explain(got[bad[0]], w[i])}")


def device_round_trip(ctx, tag, idx):
    """One pmc_gzip_compress_batch of the values idx, checked, and one pmc_gzip_decompress_batch back.  Returns
    the growth of the retry counter over the compress call."""
    import torch
    from pmc_codec import device as D
    vs = [TV.values()[i] for i in idx]
    before = ctx.guard_counts()["retry"]
    out, rc = D.compress(ctx, D.pack(vs))
    torch.cuda.synchronize()
    grew = ctx.guard_counts()["retry"] - before
    assert int((rc != 0).sum()) == 0, (tag, "rc", rc[rc != 0][:8].tolist())
    check_members(tag, idx, out.host_items())
    back, brc = D.decompress(ctx, out, [max(len(v), 1) for v in vs])
    torch.cuda.synchronize()
    assert int((brc != 0).sum()) == 0, (tag, "decompress rc", brc[brc != 0][:8].tolist())
    assert back.host_items() == vs, (tag, "round trip")
    return grew


@pytest.mark.parametrize("name", ["1k", "16k"])
def test_split_pipeline_batch(ctx, name):
    grew = device_round_trip(ctx, name, TV.batch(name))
    assert grew == 0, (name, "retry counter", grew)


def test_one_kernel_device_path(ctx):
    device_round_trip(ctx, "mono", TV.batch("mono"))


def test_host_entry(ctx):
    """pmc_gzip_compress_batch_host: the latency route (at most 1024 values of at most 4096 bytes) and, with every
    value, the pipeline route."""
    for name, route in (("mono", "latency_compress"), ("all", "pipeline_compress")):
        idx = TV.batch(name)
        vs = [TV.values()[i] for i in idx]
        before = ctx.path_counts()
        res = ctx.compress_many(vs)
        after = ctx.path_counts()
        assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {route: 1}, (name, before, after)
        assert [c for c, _ in res] == [0] * len(vs), name
        check_members(f"host/{name}", idx, [m for _, m in res])
        back = ctx.decompress_many([m for _, m in res])
        assert [(c, v) for c, v in back] == [(0, v) for v in vs], (name, "round trip")


def child():
    """Every value once through the device entry, in a process whose switch is set."""
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    try:
        device_round_trip(c, "child", TV.batch("all"))
    finally:
        c.close()


CHILD = "import sys; sys.path[:0] = [sys.argv[1]]; import conftest; import test_gpu_trees as T; T.child()"


@pytest.mark.parametrize("switch", ["PMC_DEFLATE_V1", "PMC_DEFLATE_MONO"])
def test_switch(ctx, switch):
    import torch
    torch.cuda.synchronize()  # (raises if an earlier test left the device in error: then no child is started)
    env = dict(os.environ, **{switch: "1"})
    out = subprocess.run([sys.executable, "-c", CHILD, HERE], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]

"""GPU: the back on every level-9 route, against the oracle, on the corpus of tests/back_values.py.

The back (csrc/pmc_deflate_small.hip: run_back, emit_planned, emit_symbols, codes_from_lengths_all,
send_runs_fused, run_bits, or_bits_lds, wave_crc32_s8) restates zlib's gen_codes, send_tree, compress_block and
crc32 and the length and distance code tables in closed forms and wave-wide scans, and is checked only through the
bytes of the values a test compresses.  These values were picked so that every arm of that arithmetic decides some
byte of some member: tests/test_back_model.py (CPU) asserts the coverage from the oracle's members, holds every
batch shape below to its route and pass cap, and the oracle's members to the reference's
(tests/golden/back_golden.json).

Every member is compared byte for byte with the oracle's; a mismatch is explained by back_values.explain (tokens,
lengths or bit emission, and the token or header part that holds the first differing bit) and names the classes of
the value.  Every batch is then decompressed back to its values.

  "512"   the values of at most kHdrMinLen bytes, shuffled and cycled to 4224: a pass cap of at most kNostageMaxLen,
          so the unstaged back (crc32_batch_kernel, emit_symbols<true>), tree headers from send_runs_fused
  "1k"    the values of at most 1024 bytes, likewise: the same values through the staged back and wave_crc32_s8
  "16k"   every value (those above 4096 bytes once), 4224 in all: tree headers from the trees kernel, CRC lanes
          with a second lap
  each of the three with pack(align=4), and with pack(align=1) behind a 1-byte first value: sources on odd
  addresses, stage()'s byte arm and the unaligned CRC reads
  "mono"  the values of at most 4096 bytes, once: the one-kernel device path (flush() with scan_runs + send_runs
          and the byte-wise wave_crc32)
  host    the same through pmc_gzip_compress_batch_host: its latency route, and every value on its pipeline route
  big     back_values.big(): the large-value pipeline's deflate_lv_emit_kernel
  PMC_DEFLATE_V1=1, PMC_DEFLATE_MONO=1: every value, in a child process per switch (read once per process)

On the split rows the retry counter must not grow: a value the back declined would be redone by the HBM kernel to
the right bytes, and only the counter would tell."""
import os
import subprocess
import sys

import pytest

import back_values as BV

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


def check_members(tag, vals, got):
    """got[k] is the member of vals[k]: all equal the oracle's, or the first one that differs is explained."""
    bad = [k for k, v in enumerate(vals) if got[k] != want(v)]
    if bad:
        v = vals[bad[0]]
        where = BV.values().index(v) if v in BV.values() else None
        cls = sorted(BV.classes_of(v)) if where is not None else sorted(BV.large_classes_of(want(v)))
        raise AssertionError(f"{tag}: {len(bad)} of {len(vals)} members ({len({vals[k] for k in bad})} values) differ from "
                             f"the oracle's, first value #{where} ({len(v)} B, "
                             f"make{BV.PARAMS[where] if where is not None else ''}, classes {cls}): "
                             f"{BV.explain(got[bad[0]], want(v))}")


def device_round_trip(ctx, tag, vals, align=4, sources=None):
    """One pmc_gzip_compress_batch of vals, checked, and one pmc_gzip_decompress_batch back.  Returns the growth of
    the retry counter over the compress call.  sources: called with the addresses of the values' sources in the
    batch that is sent."""
    import torch
    from pmc_codec import device as D
    b = D.pack(vals, align=align)
    if sources:
        sources([b.data.data_ptr() + int(o) for o in b.off.cpu().numpy()])
    before = ctx.guard_counts()["retry"]
    out, rc = D.compress(ctx, b)
    torch.cuda.synchronize()
    grew = ctx.guard_counts()["retry"] - before
    assert int((rc != 0).sum()) == 0, (tag, "rc", rc[rc != 0][:8].tolist())
    check_members(tag, vals, out.host_items())
    back, brc = D.decompress(ctx, out, [max(len(v), 1) for v in vals])
    torch.cuda.synchronize()
    assert int((brc != 0).sum()) == 0, (tag, "decompress rc", brc[brc != 0][:8].tolist())
    assert back.host_items() == vals, (tag, "round trip")
    return grew


@pytest.mark.parametrize("align", [4, 1])
@pytest.mark.parametrize("name", ["512", "1k", "16k"])
def test_split_pipeline_batch(ctx, name, align):
    vals, _ = BV.packed(BV.batch(name), align)

    def sources(addr):
        """The addresses the kernels read from, of the batch as sent: align 1 -- sources at addresses = 0 (mod 16),
        = 4 (mod 16) and odd, so stage()'s 16-byte, 4-byte and byte arms all run; align 4 -- none off a word."""
        mods = {a % 16 for a in addr}
        if align == 1:
            assert 0 in mods and 4 in mods and any(a & 1 for a in addr), sorted(mods)
        else:
            assert mods == {0, 4, 8, 12}, sorted(mods)

    grew = device_round_trip(ctx, f"{name}/align{align}", vals, align, sources)
    assert grew == 0, (name, align, "retry counter", grew)


def test_one_kernel_device_path(ctx):
    device_round_trip(ctx, "mono", [BV.values()[i] for i in BV.batch("mono")])


def test_host_entry(ctx):
    """pmc_gzip_compress_batch_host: the latency route (at most 1024 values of at most 4096 bytes) and, with every
    value, the pipeline route."""
    for name, route in (("mono", "latency_compress"), ("all", "pipeline_compress")):
        vs = [BV.values()[i] for i in BV.batch(name)]
        before = ctx.path_counts()
        res = ctx.compress_many(vs)
        after = ctx.path_counts()
        assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {route: 1}, (name, before, after)
        assert [c for c, _ in res] == [0] * len(vs), name
        check_members(f"host/{name}", vs, [m for _, m in res])
        back = ctx.decompress_many([m for _, m in res])
        assert [(c, v) for c, v in back] == [(0, v) for v in vs], (name, "round trip")


def test_large_value_pipeline(ctx):
    """big(): a three-word token in a block that is not the first, through deflate_lv_emit_kernel's token_bits.  The
    retry counter must not grow: a value the stitch gave up would be emitted by the HBM kernel instead."""
    grew = device_round_trip(ctx, "big", BV.big())
    assert grew == 0, ("big", "retry counter", grew)


def child():
    """Every value once through the device entry, in a process whose switch is set."""
    import torch  # noqa: F401
    import pmc_codec
    c = pmc_codec.Context(0)
    try:
        device_round_trip(c, "child", BV.values())
    finally:
        c.close()


CHILD = "import sys; sys.path[:0] = [sys.argv[1]]; import conftest; import test_gpu_back as T; T.child()"


@pytest.mark.parametrize("switch", ["PMC_DEFLATE_V1", "PMC_DEFLATE_MONO"])
def test_switch(ctx, switch):
    import torch
    torch.cuda.synchronize()  # (raises if an earlier test left the device in error: then no child is started)
    env = dict(os.environ, **{switch: "1"})
    out = subprocess.run([sys.executable, "-c", CHILD, HERE], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]

#!/usr/bin/env python3
"""Ranged and growing writes against the same update done without them (include/pmc_codec.h "ranged writes",
"growing writes").

Device-resident: n JSON-slice values of vlen bytes (bench.py's generator and seed) are compressed once at
PMC_LEVEL_FAST_ALL with the index and index_crc switches on.  Then, for every patch shape, two ways of applying one
seeded patch per value alternate, each timed with device events around `calls` calls after a warm-up, `runs` times:
  rewrite        pmc_gzip_rewrite_range_batch
  full sequence  pmc_gzip_decompress_batch of the whole members, the patches laid over the values on the device,
                 pmc_gzip_compress_batch of the whole values
Both leave the new members on the device, and they are compared byte for byte once (pmc_compare_values).  Prints one
JSON line: per shape the ms per call of every run, the chunks decoded / compressed / copied per call, the ratio of
the medians, whether the slowest rewrite run beat the fastest full-sequence run, and the per-kind kernel times of
one profiled call (the rewrite's scan and tables run under `order`, its edge decode under `inflate_lane`, overlay
and parse under `deflate_large`, emit, finish and copy under `deflate_large_emit`).
The shapes append64 and append_chunk put 64 bytes, or one chunk, behind every value: there "rewrite" is
pmc_gzip_grow_range_batch, and the full sequence decompresses the whole member into a slot of the new length, copies
the tail in on the device and compresses the whole new value.

    python scripts/patch_bench.py --n 1000 --vlen 1048576 --shapes in64,across4k,chunk,whole
    python scripts/patch_bench.py --n 40000 --vlen 65536 --shapes in64
    python scripts/patch_bench.py --n 1000 --vlen 1048576 --shapes append64,append_chunk
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "poor-man-s-cache_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pmc_codec  # noqa: E402

C = 32768


def load_corpus():
    d = os.path.join(ROOT, "tests", "golden", "data")
    return b"".join(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".json"))


def kernel_times(ctx, fn):
    L = pmc_codec.lib()
    nk = len(pmc_codec.KERNEL_KINDS)
    ms, launches = (ctypes.c_double * nk)(), (ctypes.c_uint32 * nk)()
    L.pmc_ctx_profile(ctx.handle, 1)
    fn()
    torch.cuda.synchronize()
    L.pmc_ctx_kernel_times(ctx.handle, ms, launches, nk)
    L.pmc_ctx_profile(ctx.handle, 0)
    return {k: {"ms": round(ms[i], 4), "launches": int(launches[i])} for i, k in enumerate(pmc_codec.KERNEL_KINDS)
            if launches[i]}


def timed(fn, calls, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(calls):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def shape_of(name, vlen, n, rng):
    """(patch length, seeded offsets) of a shape."""
    k = vlen // C
    if name == "in64":        # 64 bytes inside one chunk
        return 64, rng.integers(0, k, n) * C + rng.integers(0, C - 64 + 1, n)
    if name == "across4k":    # 4 KiB across a chunk boundary
        return 4096, rng.integers(1, k, n) * C - rng.integers(1, 4096, n)
    if name == "chunk":       # exactly one whole chunk
        return C, rng.integers(0, k, n) * C
    if name == "whole":
        return vlen, np.zeros(n, dtype=np.int64)
    if name == "append64":    # 64 bytes behind the value
        return 64, np.full(n, vlen, dtype=np.int64)
    if name == "append_chunk":  # one chunk behind it
        return C, np.full(n, vlen, dtype=np.int64)
    raise SystemExit(f"unknown shape {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--vlen", type=int, default=1 << 20)
    ap.add_argument("--shapes", default="in64,across4k,chunk,whole")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    n, vlen = args.n, args.vlen
    assert vlen % C == 0 and vlen > C
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = pmc_codec.lib()
    ctx = pmc_codec.Context(0)
    ctx.level = pmc_codec.LEVEL_FAST_ALL
    ctx.index = True
    ctx.index_crc = True
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    corpus_b = load_corpus()
    if vlen > len(corpus_b):
        corpus_b = corpus_b * (vlen // len(corpus_b) + 2)
    corpus = torch.frombuffer(bytearray(corpus_b), dtype=torch.uint8).to(dev)
    src = torch.empty(n * vlen + 16, dtype=torch.uint8, device=dev)
    assert L.pmc_gen_values(corpus.data_ptr(), len(corpus_b), 0x5EED, 0, 0, None, n, vlen, src.data_ptr(), sh) == 0
    off = torch.arange(n, dtype=torch.int64, device=dev) * vlen
    lens = torch.full((n,), vlen, dtype=torch.int32, device=dev)
    cap = pmc_codec.gzip_bound(vlen)
    cstride = (cap + 15) // 16 * 16
    coff = torch.arange(n, dtype=torch.int64, device=dev) * cstride
    ccap = torch.full((n,), cap, dtype=torch.int32, device=dev)

    def members():
        return (torch.empty(n * cstride + 16, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                torch.full((n,), 7, dtype=torch.int32, device=dev))

    comp, clen, crc = members()       # the old members
    new_r, rlen_r, rc_r = members()   # the rewrite's output
    new_f, rlen_f, rc_f = members()   # the full sequence's output
    ctx.compress_device(src, off, lens, comp, coff, ccap, clen, crc, vlen, sh)
    torch.cuda.synchronize()
    assert int((crc != 0).sum()) == 0
    back = torch.empty(n * vlen + 16, dtype=torch.uint8, device=dev)
    blen = torch.zeros(n, dtype=torch.int32, device=dev)
    brc = torch.zeros(n, dtype=torch.int32, device=dev)
    mism = torch.zeros(1, dtype=torch.int32, device=dev)
    res = {"n": n, "vlen": vlen, "calls": args.calls, "runs": args.runs, "source_id": pmc_codec.source_id(),
           "member_bytes_mean": float(clen.double().mean()), "shapes": {}}
    rng = np.random.default_rng(0x5EED)
    for name in args.shapes.split(","):
        ln, o = shape_of(name, vlen, n, rng)
        # the patches: bytes of another place of the corpus (JSON text, as a field update would be)
        patches = torch.empty(n * ln + 16, dtype=torch.uint8, device=dev)
        assert L.pmc_gen_values(corpus.data_ptr(), len(corpus_b), 0xBEEF, 0, 0, None, n, ln, patches.data_ptr(), sh) == 0
        poff = torch.arange(n, dtype=torch.int64, device=dev) * ln
        plen = torch.full((n,), ln, dtype=torch.int32, device=dev)
        roff = torch.from_numpy(o.astype(np.uint32).view(np.int32).copy()).to(dev)
        grows = name.startswith("append")
        if grows:  # values of glen bytes: their own value slots and member slots
            glen = vlen + ln
            goff = torch.arange(n, dtype=torch.int64, device=dev) * glen
            glens = torch.full((n,), glen, dtype=torch.int32, device=dev)
            gcap = pmc_codec.gzip_bound(glen)
            gstride = (gcap + 15) // 16 * 16
            gcoff = torch.arange(n, dtype=torch.int64, device=dev) * gstride
            gccap = torch.full((n,), gcap, dtype=torch.int32, device=dev)
            gback = torch.empty(n * glen + 16, dtype=torch.uint8, device=dev)
            new_g = torch.empty(n * gstride + 16, dtype=torch.uint8, device=dev)
            new_h = torch.empty(n * gstride + 16, dtype=torch.uint8, device=dev)
            idx = ((goff + vlen)[:, None] + torch.arange(ln, device=dev)[None, :]).reshape(-1)
        elif ln == vlen:
            idx = None
        else:
            idx = (off + torch.from_numpy(o.astype(np.int64)).to(dev))[:, None] + torch.arange(ln, device=dev)[None, :]
            idx = idx.reshape(-1)

        def rewrite_in():
            ctx.rewrite_range_device(comp, coff, clen, patches, poff, plen, roff, new_r, coff, ccap, rlen_r, rc_r, sh)

        def full_in():
            ctx.decompress_device(comp, coff, clen, back, off, lens, blen, brc, vlen, sh)
            if idx is None:
                back[:n * vlen].copy_(patches[:n * ln])
            else:
                back[idx] = patches[:n * ln]
            ctx.compress_device(back, off, lens, new_f, coff, ccap, rlen_f, rc_f, vlen, sh)

        def rewrite_grow():
            ctx.grow_range_device(comp, coff, clen, patches, poff, plen, roff, new_g, gcoff, gccap, rlen_r, rc_r, sh)

        def full_grow():
            ctx.decompress_device(comp, coff, clen, gback, goff, glens, blen, brc, glen, sh)
            gback[idx] = patches[:n * ln]
            ctx.compress_device(gback, goff, glens, new_h, gcoff, gccap, rlen_f, rc_f, glen, sh)

        rewrite, full = (rewrite_grow, full_grow) if grows else (rewrite_in, full_in)
        out_r, out_f, out_off = (new_g, new_h, gcoff) if grows else (new_r, new_f, coff)

        c0 = ctx.rewrite_counts()
        rewrite()
        torch.cuda.synchronize()
        c1 = ctx.rewrite_counts()
        full()
        torch.cuda.synchronize()
        assert int((rc_r != 0).sum()) == 0 and int((rc_f != 0).sum()) == 0 and int((brc != 0).sum()) == 0
        mism.zero_()
        assert L.pmc_compare_values(out_r.data_ptr(), out_off.data_ptr(), out_f.data_ptr(), out_off.data_ptr(),
                                    rlen_r.data_ptr(), rlen_f.data_ptr(), n, mism.data_ptr(), sh) == 0
        torch.cuda.synchronize()
        assert int(mism[0]) == 0, "the rewrite's members differ from the full sequence's"
        leg = {"patch_len": ln, "rewrite_ms": [], "full_ms": [],
               "chunks_per_call": {k: int(c1[k] - c0[k]) for k in ("decoded", "compressed", "copied")}}
        for fn in (rewrite, full):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.runs):  # the two alternate
            leg["rewrite_ms"].append(round(timed(rewrite, args.calls, stream), 4))
            leg["full_ms"].append(round(timed(full, args.calls, stream), 4))
        rm, fm = float(np.median(leg["rewrite_ms"])), float(np.median(leg["full_ms"]))
        leg["full_over_rewrite"] = round(fm / rm, 3)
        leg["slowest_rewrite_beats_fastest_full"] = max(leg["rewrite_ms"]) < min(leg["full_ms"])
        leg["rewrite_kernels"] = kernel_times(ctx, rewrite)
        leg["full_kernels"] = kernel_times(ctx, full)
        res["shapes"][name] = leg
        del patches, idx
        if grows:
            del gback, new_g, new_h
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

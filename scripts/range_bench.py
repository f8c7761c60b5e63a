#!/usr/bin/env python3
"""Ranged reads against the full read a caller needs without them (include/pmc_codec.h "ranged reads").

Device-resident: n JSON-slice values of vlen bytes (bench.py's generator and seed) are compressed once at
PMC_LEVEL_FAST_ALL with the index on; then, for every range length, a ranged call at seeded offsets and the
full pmc_gzip_decompress_batch of the same members alternate, each timed with device events around `calls`
calls after a warm-up, `runs` times.  Prints one JSON line: per leg the ms per call of every run, GiB/s of
returned bytes, the chunks decoded per call and the per-kind kernel times of one profiled call (the ranged
call's scan runs under `order`, its decode and finish under `inflate_lane`).

    python scripts/range_bench.py --n 1000 --vlen 1048576 --ranges 4096,65536,0
    python scripts/range_bench.py --n 40000 --vlen 65536 --ranges 4096,0        (0: the whole value)
    python scripts/range_bench.py --index-crc       (members with chunk CRCs: every ranged call verifies them)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--vlen", type=int, default=1 << 20)
    ap.add_argument("--ranges", default="4096,65536,0", help="range lengths; 0 = the whole value")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--index-crc", action="store_true",
                    help="write members with chunk CRCs (pmc_ctx_set_index_crc); the ranged calls then check them")
    args = ap.parse_args()
    n, vlen = args.n, args.vlen
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = pmc_codec.lib()
    ctx = pmc_codec.Context(0)
    ctx.level = pmc_codec.LEVEL_FAST_ALL
    ctx.index = True
    if args.index_crc:
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
    comp = torch.empty(n * cstride + 16, dtype=torch.uint8, device=dev)
    coff = torch.arange(n, dtype=torch.int64, device=dev) * cstride
    ccap = torch.full((n,), cap, dtype=torch.int32, device=dev)
    clen = torch.zeros(n, dtype=torch.int32, device=dev)
    crc = torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.compress_device(src, off, lens, comp, coff, ccap, clen, crc, vlen, sh)
    torch.cuda.synchronize()
    assert int((crc != 0).sum()) == 0
    # the compress call that wrote the members, timed on its own (device events, one call per run)
    compress_ms = [round(timed(lambda: ctx.compress_device(src, off, lens, comp, coff, ccap, clen, crc, vlen, sh), 1,
                               stream), 4) for _ in range(args.runs)]
    back =torch.empty(n * vlen + 16, dtype=torch.uint8, device=dev)
    blen = torch.zeros(n, dtype=torch.int32, device=dev)
    brc = torch.zeros(n, dtype=torch.int32, device=dev)

    def full():
        ctx.decompress_device(comp, coff, clen, back, off, lens, blen, brc, vlen, sh)

    full()
    torch.cuda.synchronize()
    assert int((brc != 0).sum()) == 0 and torch.equal(back[:n * vlen], src[:n * vlen])
    res = {"n": n, "vlen": vlen, "calls": args.calls, "runs": args.runs, "source_id": pmc_codec.source_id(),
           "member_bytes_mean": float(clen.double().mean()), "index_crc": bool(args.index_crc), "compress_ms": compress_ms,
           "legs": {}}
    rng = np.random.default_rng(0x5EED)
    for rl in [int(x) for x in args.ranges.split(",")]:
        ln = rl if rl else vlen
        # a range that lies within one chunk where it can: seeded chunk, seeded offset in it
        if ln <= 32768:
            o = rng.integers(0, vlen // 32768, n) * 32768 + rng.integers(0, 32768 - ln + 1, n)
        else:
            o = rng.integers(0, vlen - ln + 1, n)
        roff = torch.from_numpy(o.astype(np.uint32).view(np.int32).copy()).to(dev)
        rlen = torch.full((n,), ln, dtype=torch.int32, device=dev)
        out = torch.empty(n * ln + 16, dtype=torch.uint8, device=dev)
        ooff = torch.arange(n, dtype=torch.int64, device=dev) * ln
        olen = torch.zeros(n, dtype=torch.int32, device=dev)
        orc = torch.full((n,), 7, dtype=torch.int32, device=dev)

        def ranged():
            ctx.decompress_range_device(comp, coff, clen, roff, rlen, out, ooff, rlen, olen, orc, sh)

        c0 = ctx.range_counts()
        v0 = ctx.range_verify_counts() if args.index_crc else None
        ranged()
        torch.cuda.synchronize()
        c1 = ctx.range_counts()
        assert int((orc != 0).sum()) == 0, "ranged call declined members"
        if ln == vlen:
            assert torch.equal(out[:n * ln], src[:n * vlen]), "ranged bytes differ"
        elif n * ln <= 1 << 26:
            idx = (off + torch.from_numpy(o.astype(np.int64)).to(dev))[:, None] + torch.arange(ln, device=dev)[None, :]
            assert torch.equal(out[:n * ln].view(n, ln), src[idx]), "ranged bytes differ"
            del idx
        leg = {"range_len": ln, "chunks_per_call": int(c1["chunks"] - c0["chunks"]), "ranged_ms": [], "full_ms": []}
        if args.index_crc:  # every decoded chunk was checked, and matched
            v1 = ctx.range_verify_counts()
            leg["chunks_verified_per_call"] = int(v1["matched"] - v0["matched"])
            assert leg["chunks_verified_per_call"] == leg["chunks_per_call"] and v1["mismatched"] == v0["mismatched"]
        for fn in (ranged, full):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.runs):  # the two legs alternate
            leg["ranged_ms"].append(round(timed(ranged, args.calls, stream), 4))
            leg["full_ms"].append(round(timed(full, args.calls, stream), 4))
        rm, fm = float(np.median(leg["ranged_ms"])), float(np.median(leg["full_ms"]))
        leg["ranged_gibs_returned"] = round(n * ln / rm / 1e-3 / 2**30, 3)
        leg["full_gibs_value"] = round(n * vlen / fm / 1e-3 / 2**30, 3)
        leg["full_over_ranged"] = round(fm / rm, 3)
        leg["ranged_kernels"] = kernel_times(ctx, ranged)
        leg["full_kernels"] = kernel_times(ctx, full)
        res["legs"][str(rl)] = leg
        del out
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

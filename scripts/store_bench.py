#!/usr/bin/env python3
"""Wall time per call of the device store's host path (include/pmc_codec.h pmc_store_*).

For every case (n values of vlen bytes, JSON slices of the golden corpus at seeded offsets) the four batch calls
pmc_store_put_batch, pmc_store_get_batch (RESP frame), pmc_store_get_range_batch (RESP frame, vlen / 4 bytes at
seeded offsets) and pmc_store_set_range_batch (64-byte patches at seeded offsets) are timed through the C ABI
with arrays built beforehand, so the time is the library's: staging, copies, kernels and the wait for them.
PMC_LEVEL_FAST_ALL with the index and chunk CRCs on: at 64 KiB the ranged calls take the chunk path, at 1 KiB
the whole-value rounds.  Each call is warmed up, then timed `runs` times over `calls` calls (time.perf_counter
around the calls of a run; the extents a put allocates are freed outside the timed region).  Prints one JSON
line: per case and call the ms per call of every run.

    python scripts/store_bench.py
    python scripts/store_bench.py --cases 4096x1024,1000x65536 --calls 10 --runs 3
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "poor-man-s-cache_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import pmc_codec  # noqa: E402


def load_corpus():
    d = os.path.join(ROOT, "tests", "golden", "data")
    return b"".join(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".json"))


def offsets(lens):
    off = np.zeros(len(lens), dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return off


def case(ctx, corpus, n, vlen, calls, warmup, runs):
    L = pmc_codec.lib()
    rng = np.random.default_rng(0x5EED)
    tiled = corpus * (vlen // len(corpus) + 2)
    src = b"".join(tiled[o:o + vlen] for o in rng.integers(0, len(corpus), n))
    lens = np.full(n, vlen, dtype=np.uint32)
    off = offsets(lens)
    st = pmc_codec.Store(ctx, 4 * n * pmc_codec.gzip_bound(vlen) + (64 << 20))
    ext = (pmc_codec.Extent * n)()      # the resident values the gets and the ranged set work on
    fresh = (pmc_codec.Extent * n)()    # what a timed put allocates
    rc = np.zeros(n, dtype=np.int32)
    resp = (ctypes.c_void_p * n)()
    rlen = np.zeros(n, dtype=np.uint32)
    rl = max(1, vlen // 4)
    g_off = rng.integers(0, vlen - rl + 1, n).astype(np.uint32)
    g_len = np.full(n, rl, dtype=np.uint32)
    p_len = np.full(n, 64, dtype=np.uint32)
    p_off = offsets(p_len)
    p_src = bytes(rng.integers(97, 123, 64 * n, dtype=np.uint8)) + b"\0"
    p_at = rng.integers(0, vlen - 64 + 1, n).astype(np.uint32)

    def ok(r):
        assert r == 0 and int((rc != 0).sum()) == 0, (r, pmc_codec.last_error(), rc[rc != 0][:8])

    def put():
        ok(L.pmc_store_put_batch(st.handle, src, off.ctypes.data, lens.ctypes.data, n, fresh, rc.ctypes.data))

    def get():
        ok(L.pmc_store_get_batch(st.handle, ext, n, pmc_codec.FRAME_RESP, resp, rlen.ctypes.data, rc.ctypes.data))

    def get_range():
        ok(L.pmc_store_get_range_batch(st.handle, ext, g_off.ctypes.data, g_len.ctypes.data, n, pmc_codec.FRAME_RESP, resp,
                                       rlen.ctypes.data, rc.ctypes.data))

    def set_range():
        ok(L.pmc_store_set_range_batch(st.handle, ext, p_src, p_off.ctypes.data, p_len.ctypes.data, p_at.ctypes.data, n,
                                       rc.ctypes.data))

    ok(L.pmc_store_put_batch(st.handle, src, off.ctypes.data, lens.ctypes.data, n, ext, rc.ctypes.data))
    out = {}
    for name, fn in (("put", put), ("get", get), ("get_range", get_range), ("set_range", set_range)):
        after = (lambda: L.pmc_store_free(st.handle, fresh, n)) if name == "put" else (lambda: None)
        for _ in range(warmup):
            fn()
            after()
        ms = []
        for _ in range(runs):
            t = 0.0
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                t += time.perf_counter() - t0
                after()
            ms.append(round(t / calls * 1e3, 4))
        out[name + "_ms"] = ms
    # what the calls left: every value with its patch, framed
    get()
    i = n - 1
    want = bytearray(src[i * vlen:(i + 1) * vlen])
    want[int(p_at[i]):int(p_at[i]) + 64] = p_src[64 * i:64 * i + 64]
    assert ctypes.string_at(resp[i], int(rlen[i])) == b"$%d\r\n" % vlen + bytes(want) + b"\r\n"
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="4096x1024,1000x65536", help="n x value bytes, comma separated")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = pmc_codec.Context(0)
    ctx.level = pmc_codec.LEVEL_FAST_ALL
    ctx.index = True
    ctx.index_crc = True
    corpus = load_corpus()
    res = {"calls": args.calls, "warmup": args.warmup, "runs": args.runs, "lib": os.path.basename(pmc_codec.LIB_PATH), "cases": {}}
    for c in args.cases.split(","):
        n, vlen = (int(x) for x in c.split("x"))
        res["cases"][c] = case(ctx, corpus, n, vlen, args.calls, args.warmup, args.runs)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

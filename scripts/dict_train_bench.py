"""Measurements of dictionary training (DESIGN.md §4 "Dictionary training"), on one MI355X:

  time    pmc_dict_train_batch over 65,536 x 1 KiB JSON slices at D = 2048 and 8192: the median of --reps runs after
          --warmup, by device events around the enqueue-only call; against tests/host/dict_train_check.cpp (-O2, one
          thread) on the same samples, and the results' CRC-32 compared.
  bytes   the fast level's members of the two baseline sets of tests/golden/dict_baseline.json with the trained
          dictionary (trained on the seeded set of tests/dict_train_values.py), the baseline dictionary (seed 99)
          and the twelve random-slice dictionaries of seeds 100 .. 111 (their median), at 2 KiB and 8 KiB.

    python scripts/dict_train_bench.py --out profiles/dict_train/dict_train_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "poor-man-s-cache_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from dict_train_values import case_file, packed, seeded_samples  # noqa: E402
from dict_values import BASELINE_SETS, baseline_values  # noqa: E402
from fast_values import json_slices  # noqa: E402

TIME_SET = (1024, 65536, 4242)  # size, count, seed
RANDOM_SEEDS = range(100, 112)
BASELINE_SEED = 99


def corpus():
    d = os.path.join(ROOT, "tests", "golden", "data")
    return b"".join(open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".json"))


def time_training(ctx, samples, sizes, warmup, reps, cpu_reps):
    import torch
    from pmc_codec import device as D
    b = D.pack(samples, align=1)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe, path = os.path.join(tmp, "dict_train_check"), os.path.join(tmp, "cases.bin")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe,
                               os.path.join(ROOT, "tests", "host", "dict_train_check.cpp")])
        with open(path, "wb") as f:
            f.write(case_file([packed(f"time_{s}", samples, s) for s in sizes]))
        timed = subprocess.check_output([exe, "time", path, str(cpu_reps)], text=True)
        cpu = [json.loads(ln) for ln in timed.splitlines()]
        cpu_crc = [zlib.crc32(bytes.fromhex(g.replace("-", "")))
                   for g in subprocess.check_output([exe, "train", path], text=True).split()]
    for size, c, crc in zip(sizes, cpu, cpu_crc):
        dic = torch.zeros(size, dtype=torch.uint8, device="cuda")
        dlen = torch.zeros(1, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        ms = []
        for k in range(warmup + reps):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ctx.train_dictionary_device(b.data, b.off, b.len, size, dic, dlen, st)
            z.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(a.elapsed_time(z))
        got = dic.cpu().numpy()[:int(dlen.cpu()[0])].tobytes()
        out[str(size)] = {"samples": len(samples), "sample_bytes": sum(map(len, samples)), "dict_len": len(got),
                          "gpu_ms_median": statistics.median(ms), "gpu_ms_min": min(ms), "gpu_ms_max": max(ms),
                          "launches": 2 * (size // 64) + 3, "cpu_ms": c["ms"],
                          "cpu_over_gpu": c["ms"] / statistics.median(ms),
                          "same_bytes_as_cpu": zlib.crc32(got) == crc and len(got) == c["dict_len"]}
    return out


def member_bytes(ctx, c):
    import torch
    import pmc_codec
    from pmc_codec import device as D
    sets = {name: baseline_values(c, name) for name in BASELINE_SETS}
    batches = {name: D.pack(v) for name, v in sets.items()}

    def totals(d):
        ctx.set_dictionary(d)
        res = {}
        for name, b in batches.items():
            o, rc = D.compress(ctx, b)
            torch.cuda.synchronize()
            assert int((rc != 0).sum()) == 0
            res[name] = int(o.len.sum())
        return res

    ctx.level = pmc_codec.LEVEL_FAST
    train_on = seeded_samples(c)
    out = {"none": totals(None)}
    for size in (2048, 8192):
        trained = ctx.train_dictionary(train_on, size)
        rnd = [totals(b"".join(json_slices(c, 256, size // 256, s))) for s in RANDOM_SEEDS]
        out[str(size)] = {"trained": totals(trained), "trained_len": len(trained), "trained_crc32": zlib.crc32(trained),
                          "baseline_seed_99": totals(b"".join(json_slices(c, 256, size // 256, BASELINE_SEED))),
                          "random_median": {n: statistics.median(r[n] for r in rnd) for n in sets},
                          "random_best": {n: min(r[n] for r in rnd) for n in sets},
                          "random_worst": {n: max(r[n] for r in rnd) for n in sets}}
    ctx.set_dictionary(None)
    ctx.level = pmc_codec.LEVEL_EXACT
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_train", "dict_train_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--count", type=int, default=TIME_SET[1])
    a = ap.parse_args()
    import torch
    import pmc_codec
    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured without one"
    c = corpus()
    ctx = pmc_codec.Context(0)
    doc = {"device": torch.cuda.get_device_name(0),
           "time": time_training(ctx, json_slices(c, TIME_SET[0], a.count, TIME_SET[2]), (2048, 8192), a.warmup, a.reps,
                                 a.cpu_reps),
           "member_bytes": member_bytes(ctx, c)}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()

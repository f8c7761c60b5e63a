"""Writes tests/golden/fast_large_baseline.json: the summed member lengths of zlib level 1 and level 9
(zlib.compressobj(level, DEFLATED, 31, 8)) over the seeded set of 64 KiB JSON slices the ratio condition of
the fast level for large values is stated on (tests/test_gpu_fast_large.py).  Run where Python's zlib is
1.2.11, the reference's.

    python tests/golden/make_fast_large_baseline.py
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from fast_large_values import BASELINE_COUNT, BASELINE_SIZE  # noqa: E402
from fast_values import json_slices  # noqa: E402

SEED = 11


def corpus():
    names = sorted(f for f in os.listdir(os.path.join(HERE, "data")) if f.endswith(".json"))
    return b"".join(open(os.path.join(HERE, "data", n), "rb").read() for n in names)


def member_len(v, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8)
    return len(c.compress(v) + c.flush())


def totals(c):
    vals = json_slices(c, BASELINE_SIZE, BASELINE_COUNT, SEED)
    return {"size": BASELINE_SIZE, "count": BASELINE_COUNT, "seed": SEED,
            "level1_total": sum(member_len(v, 1) for v in vals),
            "level9_total": sum(member_len(v, 9) for v in vals)}


if __name__ == "__main__":
    assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11", zlib.ZLIB_RUNTIME_VERSION
    doc = {"zlib": zlib.ZLIB_RUNTIME_VERSION, "set": totals(corpus())}
    with open(os.path.join(HERE, "fast_large_baseline.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))

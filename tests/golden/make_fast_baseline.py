"""Writes tests/golden/fast_baseline.json: the summed member lengths of zlib level 1 and level 9
(zlib.compressobj(level, DEFLATED, 31, 8)) over the two seeded JSON-slice sets the fast level's ratio
condition is stated on (tests/test_gpu_fast.py).  Run where Python's zlib is 1.2.11, the reference's.

    python tests/golden/make_fast_baseline.py
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from fast_values import BASELINE_SETS, json_slices  # noqa: E402

SEED = 7


def corpus():
    names = sorted(f for f in os.listdir(os.path.join(HERE, "data")) if f.endswith(".json"))
    return b"".join(open(os.path.join(HERE, "data", n), "rb").read() for n in names)


def member_len(v, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8)
    return len(c.compress(v) + c.flush())


def totals(c):
    sets = {}
    for name, (size, count) in BASELINE_SETS.items():
        vals = json_slices(c, size, count, SEED)
        sets[name] = {"size": size, "count": count, "seed": SEED,
                      "level1_total": sum(member_len(v, 1) for v in vals),
                      "level9_total": sum(member_len(v, 9) for v in vals)}
    return sets


if __name__ == "__main__":
    assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11", zlib.ZLIB_RUNTIME_VERSION
    doc = {"zlib": zlib.ZLIB_RUNTIME_VERSION, "sets": totals(corpus())}
    with open(os.path.join(HERE, "fast_baseline.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))

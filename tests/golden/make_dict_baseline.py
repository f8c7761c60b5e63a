"""Writes tests/golden/dict_baseline.json: what zlib gives on the two seeded JSON-slice sets the preset
dictionary's size conditions are stated on (tests/test_gpu_dict.py), with the 2 KiB dictionary of
tests/dict_values.py.  Per set: the summed lengths of raw deflate (wbits -15) at levels 1 and 9 with that
dictionary as zdict, plus 18 framing bytes per value, and of level 9 without a dictionary, framed alike.
Run where Python's zlib is 1.2.11, the reference's.

    python tests/golden/make_dict_baseline.py
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dict_values import (BASELINE_DICT, BASELINE_SEED, BASELINE_SETS, FRAMING, baseline_dictionary,  # noqa: E402
                         baseline_values)


def corpus():
    names = sorted(f for f in os.listdir(os.path.join(HERE, "data")) if f.endswith(".json"))
    return b"".join(open(os.path.join(HERE, "data", n), "rb").read() for n in names)


def framed_len(v, level, zdict=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict is not None \
        else zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return len(c.compress(v) + c.flush()) + FRAMING


def totals(c):
    d = baseline_dictionary(c)
    sets = {}
    for name, (size, count) in BASELINE_SETS.items():
        vals = baseline_values(c, name)
        sets[name] = {"size": size, "count": count, "seed": BASELINE_SEED,
                      "level1_dict_total": sum(framed_len(v, 1, d) for v in vals),
                      "level9_dict_total": sum(framed_len(v, 9, d) for v in vals),
                      "level9_total": sum(framed_len(v, 9) for v in vals)}
    return {"dict_size": BASELINE_DICT[0], "dict_seed": BASELINE_DICT[1], "dict_crc32": zlib.crc32(d), "sets": sets}


if __name__ == "__main__":
    assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11", zlib.ZLIB_RUNTIME_VERSION
    doc = dict(totals(corpus()), zlib=zlib.ZLIB_RUNTIME_VERSION)
    with open(os.path.join(HERE, "dict_baseline.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))

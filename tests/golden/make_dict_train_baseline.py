"""Writes tests/golden/dict_train_baseline.json: what zlib gives on the two seeded JSON-slice sets of
tests/golden/dict_baseline.json with the TRAINED dictionary (tests/dict_train_model.py over the seeded sample set of
tests/dict_train_values.py, D = 2048) as zdict.  Per set: the summed lengths of raw deflate (wbits -15) at levels 1
and 9, plus 18 framing bytes per value, framed as make_dict_baseline.py frames them.
Run where Python's zlib is 1.2.11, the reference's.

    python tests/golden/make_dict_train_baseline.py
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dict_train_model import train  # noqa: E402
from dict_train_values import SEEDED, seeded_samples  # noqa: E402
from dict_values import BASELINE_SEED, BASELINE_SETS, baseline_values  # noqa: E402
from make_dict_baseline import corpus, framed_len  # noqa: E402

TRAINED_SIZE = 2048


def totals(c):
    d = train(seeded_samples(c), TRAINED_SIZE)
    sets = {}
    for name, (size, count) in BASELINE_SETS.items():
        vals = baseline_values(c, name)
        sets[name] = {"size": size, "count": count, "seed": BASELINE_SEED,
                      "level1_dict_total": sum(framed_len(v, 1, d) for v in vals),
                      "level9_dict_total": sum(framed_len(v, 9, d) for v in vals)}
    return {"dict_size": TRAINED_SIZE, "dict_len": len(d), "dict_crc32": zlib.crc32(d),
            "samples": {"size": SEEDED[0], "count": SEEDED[1], "seed": SEEDED[2]}, "sets": sets}


if __name__ == "__main__":
    assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11", zlib.ZLIB_RUNTIME_VERSION
    doc = dict(totals(corpus()), zlib=zlib.ZLIB_RUNTIME_VERSION)
    with open(os.path.join(HERE, "dict_train_baseline.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))

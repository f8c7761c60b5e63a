"""Reference vectors for the corpus of tests/back_values.py (run in the build container only).

Source of truth: the reference's own GzipCompressor::Compress
(src/compressor/gzip_compressor.cpp:3-50 of the reference tree), compiled unmodified into
oracle/_ref/libref_gzip.so by `make -C oracle ref` (system zlib 1.2.11).  The values are NUL-free, so
every one passes the reference's strlen interface.

Per value of values() and of big() the fixture keeps the SHA-256 and length of the reference's member,
keyed by the SHA-256 of the value: a byte-exact check -- the tests hash the oracle's (and the device's)
member and compare.  One vector per line, sorted by key.

Output (data only): tests/golden/back_golden.json
Usage: python tests/golden/make_back_golden.py
"""
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O  # noqa: E402
import back_values as BV  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def libz(b):
    c = zlib.compressobj(9, zlib.DEFLATED, 31, 8, 0)
    return c.compress(b) + c.flush()


def main():
    O.build(ref=True)
    assert O.ref_available(), "oracle/_ref/libref_gzip.so missing (needs the reference tree)"
    vectors = {}
    for k, v in enumerate(BV.values() + BV.big()):
        assert b"\0" not in v, k
        rc, gz = O.ref_compress(v)
        assert rc == 0, (k, rc)
        assert gz == libz(v), k
        vectors[BV.sha(v)] = {"gz_sha256": BV.sha(gz), "gz_len": len(gz)}
    doc = {
        "generator": "tests/golden/make_back_golden.py",
        "reference": "the reference's src/compressor/gzip_compressor.cpp (built by oracle/Makefile ref)",
        "zlib_version": O.ref().ref_zlib_version().decode(),
        "values": "tests/back_values.py (seeded generator, parameters in PARAMS and BIG_PARAMS)",
        "record": "vectors[sha256(value)] = SHA-256 and length of the reference's gzip member of the value",
        "count": len(vectors),
    }
    dump = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(os.path.join(HERE, "back_golden.json"), "w") as f:  # one vector per line, sorted: diffable
        f.write(dump(doc)[:-1] + ',\n"vectors":{\n')
        f.write(",\n".join(f"{dump(k)}:{dump(vectors[k])}" for k in sorted(vectors)))
        f.write("\n}}\n")
    print("vectors", len(vectors))


if __name__ == "__main__":
    main()

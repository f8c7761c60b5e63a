"""Reference vectors for the corpus of tests/large_conf_values.py (run in the build container only).

Source of truth: the reference's own GzipCompressor::Compress
(/root/reference/src/compressor/gzip_compressor.cpp:3-50), compiled unmodified into
oracle/_ref/libref_gzip.so by `make -C oracle ref` (system zlib 1.2.11).  The values are NUL-free, so
every one passes the reference's strlen interface; the NUL group (large_conf_values.nul_values()) cannot, and its
vectors are libz's, which every other vector is asserted equal to as well.

Per value the fixture keeps the SHA-256 and length of the reference's member, keyed by the SHA-256 of
the value.  One vector per line, sorted by key.

Output (data only): tests/golden/large_conf_golden.json
Usage: python tests/golden/make_large_conf_golden.py
"""
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O  # noqa: E402
import large_conf_values as LC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def libz(b):
    c = zlib.compressobj(9, zlib.DEFLATED, 31, 8, 0)
    return c.compress(b) + c.flush()


def main():
    O.build(ref=True)
    assert O.ref_available(), "oracle/_ref/libref_gzip.so missing (needs /root/reference)"
    vectors = {}
    for k, v in enumerate(LC.values()):
        assert b"\0" not in v and len(v) > LC.BIG_MAX, k
        rc, gz = O.ref_compress(v)
        assert rc == 0, (k, rc)
        assert gz == libz(v), k
        vectors[LC.sha(v)] = {"gz_sha256": LC.sha(gz), "gz_len": len(gz)}
    for v in LC.nul_values():
        gz = libz(v)
        vectors[LC.sha(v)] = {"gz_sha256": LC.sha(gz), "gz_len": len(gz)}
    doc = {
        "generator": "tests/golden/make_large_conf_golden.py",
        "reference": "/root/reference/src/compressor/gzip_compressor.cpp (built by oracle/Makefile ref)",
        "zlib_version": O.ref().ref_zlib_version().decode(),
        "values": "tests/large_conf_values.py (seeded generators, parameters in PARAMS and NUL_PARAMS)",
        "record": "vectors[sha256(value)] = SHA-256 and length of the reference's gzip member of the value (libz's for "
                  "the values that hold NULs)",
        "count": len(vectors),
    }
    dump = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(os.path.join(HERE, "large_conf_golden.json"), "w") as f:  # one vector per line, sorted: diffable
        f.write(dump(doc)[:-1] + ',\n"vectors":{\n')
        f.write(",\n".join(f"{dump(k)}:{dump(vectors[k])}" for k in sorted(vectors)))
        f.write("\n}}\n")
    print("vectors", len(vectors))


if __name__ == "__main__":
    main()

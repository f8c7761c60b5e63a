"""Reference vectors for the stream windows of tests/boundary_values.py (run in the build container only).

Source of truth: the reference's own GzipCompressor::Compress
(/root/reference/src/compressor/gzip_compressor.cpp:3-50), compiled unmodified into
oracle/_ref/libref_gzip.so by `make -C oracle ref` (system zlib 1.2.11).  The streams are NUL-free, so
every value passes the reference's strlen interface; a value that held a NUL would come from Python's
zlib bound to the same libz with the reference's parameters and be tagged "libz", as in
make_large_golden.py.

Per level-9 value (the shapes mono, split-s12, split, big, lv and lv-json) the fixture keeps the SHA-256 and
length of the reference's member, keyed by the SHA-256 of the value: a byte-exact check -- the tests
hash the device's member and compare.  One vector per line, sorted by key.

Output (data only): tests/golden/boundary_golden.json
Usage: python tests/golden/make_boundary_golden.py
"""
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O  # noqa: E402
import boundary_values as BV  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def libz(b):
    c = zlib.compressobj(9, zlib.DEFLATED, 31, 8, 0)
    return c.compress(b) + c.flush()


def main():
    O.build(ref=True)
    assert O.ref_available(), "oracle/_ref/libref_gzip.so missing (needs /root/reference)"
    vectors, shapes = {}, {}
    for name in BV.LEVEL9_SHAPES:
        ws = BV.shape(name)
        for w in ws:
            v = BV.value(w)
            k = BV.sha(v)
            if k in vectors:
                continue
            if b"\0" in v:
                gz, src = libz(v), "libz"
            else:
                rc, gz = O.ref_compress(v)
                assert rc == 0, (name, w, rc)
                assert gz == libz(v)
                src = "reference"
            vectors[k] = {"gz_sha256": BV.sha(gz), "gz_len": len(gz)}
            if src != "reference":
                vectors[k]["source"] = src
        shapes[name] = len(ws)
        print(f"{name}: {len(ws)} values, {sum(w.n for w in ws)} B", flush=True)
    doc = {
        "generator": "tests/golden/make_boundary_golden.py",
        "reference": "/root/reference/src/compressor/gzip_compressor.cpp (built by oracle/Makefile ref)",
        "zlib_version": O.ref().ref_zlib_version().decode(),
        "values": "tests/boundary_values.py (windows of five deterministic streams)",
        "record": "vectors[sha256(value)] = SHA-256 and length of the reference's gzip member of the value "
                  "(\"source\" only where it is not the reference)",
        "shapes": shapes,
    }
    dump = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(os.path.join(HERE, "boundary_golden.json"), "w") as f:  # one vector per line, sorted: diffable
        f.write(dump(doc)[:-1] + ',\n"vectors":{\n')
        f.write(",\n".join(f"{dump(k)}:{dump(vectors[k])}" for k in sorted(vectors)))
        f.write("\n}}\n")
    print("vectors", len(vectors), "reference", sum("source" not in v for v in vectors.values()))


if __name__ == "__main__":
    main()

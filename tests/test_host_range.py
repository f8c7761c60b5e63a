"""CPU: the host arithmetic of ranged reads (csrc/pmc_plan.hpp range_of and plan_range, which the kernels, the
C API and the store share), printed by tests/host/range_check.cpp -- a stand-alone program built with the
address and undefined-behaviour sanitizers -- equals tests/range_model.py's statement, and the edge rows it
plans stay within the stated budget whatever n is."""
import json
import os
import subprocess
import tempfile

import pytest

from indexed_model import C
from range_model import LOG2_MAX, ROW_BYTES, SCRATCH_BUDGET, plan_range, range_of, ranges_for

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="pmc_range_")
    out = os.path.join(d, "range_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "range_check.cpp")])
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(ln) for ln in out.stdout.splitlines()]


def test_constants(exe):
    assert run(exe, "budget") == [{"log2_max": LOG2_MAX, "row_bytes": ROW_BYTES, "budget": SCRATCH_BUDGET,
                                   "fallback": 64 << 20}]


def test_range_of(exe):
    quads = []
    for isize in (C + 1, 2 * C, 2 * C + 3, 100000, 1 << 20, 0xFFFFFFFF):
        for lg in (12, 15, 16):
            ch = 1 << lg
            rs = ranges_for(isize, ch) + [(0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0xFFFFFFFF),
                                         (ch - 1, 0xFFFFFFFF), (isize - 1, 0xFFFFFFFF)]
            quads += [(isize, lg, off & 0xFFFFFFFF, ln & 0xFFFFFFFF) for off, ln in rs]
    got = run(exe, "of", *[x for q in quads for x in q])
    assert len(got) == len(quads)
    for q, g in zip(quads, got):
        o, L, k0, items = range_of(*q)
        assert g == {"o": o, "L": L, "k0": k0, "items": items}, q
        assert o + L <= q[0] and (L == 0 or (k0 + items - 1) << q[1] < q[0])
    # no 32-bit wrap: the whole of a 4 GiB - 1 value, in chunks of 64 KiB
    assert range_of(0xFFFFFFFF, 16, 0, 0xFFFFFFFF) == (0, 0xFFFFFFFF, 0, 65536)


def test_plan_and_budget(exe):
    ns = [1, 400, 16379, 16380, 100000, (1 << 32) - 1]
    for cus, per_cu in ((256, 3), (1, 1), (304, 2)):
        got = run(exe, "plan", cus, per_cu, *ns)
        for n, g in zip(ns, got):
            assert g == plan_range(n, cus, per_cu), (n, cus)
            assert g["edge_bytes"] <= SCRATCH_BUDGET and g["rows"] >= 1
            assert g["cb"] <= cus * per_cu
            # every lane that may hold an edge chunk has a row of its own
            assert g["rows"] == (2 * n if g["row_per_request"] else g["cb"] * 64)
            assert g["rows_off"] % 16 == 0 and g["pre"] % 8 == 0 and g["fail"] == 4 * n
    rows = {r["n"]: r for r in run(exe, "plan", 256, 3, *ns)}
    assert rows[400]["row_per_request"] == 1 and rows[400]["cb"] == 768
    assert rows[100000]["row_per_request"] == 0 and rows[100000]["cb"] == SCRATCH_BUDGET // ROW_BYTES // 64

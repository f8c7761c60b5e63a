"""CPU: the host arithmetic of ranged writes (csrc/pmc_plan.hpp patch_of, crc_fold_host, plan_patch and
plan_patch_round, which the kernels, the C API and the store share), printed by tests/host/patch_check.cpp -- a
stand-alone program built with the address and undefined-behaviour sanitizers -- equals tests/patch_model.py's
statement, and a round's scratch stays within the stated budget whatever n is."""
import json
import os
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from indexed_crc_model import chunk_crcs
from indexed_model import C
from patch_model import (MAX_WAVES, ROUND_CHUNKS, SCRATCH_BUDGET, SEGS, SLAB_BYTES, fold, patch_of, plan_patch,
                         plan_patch_round, slot_bytes)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="pmc_patch_")
    out = os.path.join(d, "patch_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "patch_check.cpp")])
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(ln) for ln in out.stdout.splitlines()]


def test_constants(exe):
    assert run(exe, "budget") == [{"round_chunks": ROUND_CHUNKS, "budget": SCRATCH_BUDGET, "slab": SLAB_BYTES,
                                   "max_waves": MAX_WAVES, "slot": slot_bytes(), "slot_bound": slot_bytes(), "segs": SEGS,
                                   "max_chunks": 8190}]
    assert ROUND_CHUNKS >= 8190  # a request's touched chunks fit one round


def test_patch_of(exe):
    quads = []
    for isize in (C + 1, 2 * C, 2 * C + 2, 2 * C + 3, 100000, 1 << 20, 0xFFFFFFFF):
        for lg in (12, 15):
            ch = 1 << lg
            for off, ln in ((0, 0), (0, 1), (ch - 1, 2), (ch, 1), (ch, ch), (ch - 5, ch + 10), (0, isize), (1, isize - 1),
                            (isize - 1, 1), (isize - 1, 2), (isize, 0), (isize, 1), (isize - 3, 3), (2 * ch, isize - 2 * ch),
                            (0xFFFFFFFF, 2), (0xFFFFFFFF, 0xFFFFFFFF), (5, 0xFFFFFFFF), (ch + 7, 64)):
                quads.append((isize, lg, off & 0xFFFFFFFF, ln & 0xFFFFFFFF))
    got = run(exe, "of", *[x for q in quads for x in q])
    assert len(got) == len(quads)
    for q, g in zip(quads, got):
        ok, a, b, items, ea, eb = patch_of(*q)
        assert g == {"ok": int(ok), "a": a, "b": b, "items": items, "edge_a": int(ea), "edge_b": int(eb)}, q
        assert not ok or items == 0 or (b << q[1]) < q[0]
    # no 32-bit wrap
    assert patch_of(C + 1, 15, 0xFFFFFFFF, 2)[0] is False


def test_fold(exe):
    rng = np.random.default_rng(13)
    for n in (C + 1, C + 2, C + 3, C + 1696, 2 * C, 100000, 5 * C + 1):
        v = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        crcs = chunk_crcs(v)
        got = run(exe, "fold", n, 15, *crcs)
        assert got == [{"K": len(crcs), "crc": zlib.crc32(v)}] and fold(crcs, n) == zlib.crc32(v), n
    v = rng.integers(0, 256, 3 * 4096 + 5, dtype=np.uint8).tobytes()
    assert run(exe, "fold", len(v), 12, *chunk_crcs(v, 4096)) == [{"K": 4, "crc": zlib.crc32(v)}]


def test_plan_and_budget(exe):
    ns = [1, 400, 100000, (1 << 32) - 1]
    for cus in (256, 1, 304):
        for n, g in zip(ns, run(exe, "plan", cus, *ns)):
            assert g == plan_patch(n, cus), (n, cus)
            assert g["bytes"] <= 44 * n + 8 * (n // 1024 + 1) + 16 and g["roff"] % 8 == 0
        # a round never holds more than ROUND_CHUNKS chunks, whatever n is: its scratch stays within the budget
        items = [0, 1, 4, 1000, ROUND_CHUNKS - 1, ROUND_CHUNKS]
        for it, g in zip(items, run(exe, "round", cus, *items)):
            assert g == plan_patch_round(it, cus), (it, cus)
            assert g["bytes"] <= SCRATCH_BUDGET and 4 <= g["waves"] <= MAX_WAVES and g["waves"] % 4 == 0
            assert all(g[k] % 256 == 0 for k in ("stage", "tok", "seg_val", "seg_tok0", "seg_tok", "slots", "span", "crc",
                                                 "slabs"))
        # a call of n requests: its largest round is min(n x 8190, ROUND_CHUNKS) chunks
        worst = [min(n * 8190, ROUND_CHUNKS) for n in ns]
        for n, g in zip(ns, run(exe, "round", cus, *worst)):
            assert g["bytes"] <= SCRATCH_BUDGET, (n, g["bytes"])
    # what the header states: a touched chunk takes about 197 KiB, 1000 single-chunk requests about 255 MiB
    one = plan_patch_round(1000, 256)
    assert 250 << 20 <= one["bytes"] <= 258 << 20
    assert plan_patch_round(ROUND_CHUNKS, 256)["bytes"] > SCRATCH_BUDGET * 3 // 4

"""CPU: the host arithmetic of growing writes (csrc/pmc_plan.hpp grow_of, which the scan, the decode, the C API and
the store share), printed by tests/host/grow_check.cpp -- a stand-alone program built with the address and
undefined-behaviour sanitizers -- equals tests/grow_model.py's statement over a grid that holds the 32-bit edges and
the edge between 8190 and 8191 chunks."""
import json
import os
import subprocess
import tempfile

import pytest

from grow_model import MAX_CHUNKS, SAME, SERVE, grow_of
from indexed_model import C
from patch_model import ARG, NO_INDEX, patch_of

HERE = os.path.dirname(os.path.abspath(__file__))
CODE = {SERVE: 0, SAME: 1, ARG: 2, NO_INDEX: 3}


@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="pmc_grow_")
    out = os.path.join(d, "grow_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host", "grow_check.cpp")])
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(ln) for ln in out.stdout.splitlines()]


def grid():
    quads = []
    for isize in (0, 1, C, C + 1, 2 * C, 2 * C + 3, 3 * C - 1, 100000, 1 << 20, MAX_CHUNKS * C - 1, MAX_CHUNKS * C,
                  0xFFFFFFFF):
        for lg in (12, 15):
            ch = 1 << lg
            k = (isize + ch - 1) >> lg
            for off, ln in ((0, 0), (isize + 9, 0), (0, 1), (isize, 1), (isize, 2), (isize, 3), (isize, ch),
                            (isize, ch + 1),
                            (max(isize, 5) - 5, 10), (isize + 1, 1), (isize + 2 * ch + 7, 5), (0, isize + 10),
                            (ch, isize + 100), ((k - 1) * ch if k else 0, ch + 9), (max(k, 2) * ch - 2 * ch, 3 * ch),
                            (ch - 1, 2), (5, 64), (MAX_CHUNKS * ch, 1), (MAX_CHUNKS * ch - 1, 1),
                            (MAX_CHUNKS * ch - 1, 2),
                            (0xFFFFFFFF, 1), (0xFFFFFFFF, 2), (0xFFFFFFFE, 1), (0xFFFFFFFE, 2), (5, 0xFFFFFFFF),
                            (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (1, 0xFFFFFFFF)):
                quads.append((isize, lg, off & 0xFFFFFFFF, ln & 0xFFFFFFFF))
    return quads


def test_grow_of(exe):
    quads = grid()
    got = run(exe, "of", *[x for q in quads for x in q])
    assert len(got) == len(quads)
    seen = set()
    for q, g in zip(quads, got):
        v, grows, s2, k2, a, b, items, ea, eb = grow_of(*q)
        assert g == {"verdict": CODE[v], "grows": int(grows), "S2": s2, "K2": k2, "a": a, "b": b, "items": items,
                     "edge_a": int(ea), "edge_b": int(eb)}, q
        seen.add((v, grows))
        isize, lg, off, ln = q
        if v == SERVE and not grows:       # within the value: patch_of's figures
            assert (True, a, b, items, ea, eb) == patch_of(*q), q
        if v == SERVE and grows:
            k = (isize + (1 << lg) - 1) >> lg
            assert s2 == off + ln > isize and k2 == -(-s2 >> lg) <= MAX_CHUNKS and a + items == k2 and b == k2 - 1, q
            assert a <= max(k, 1) - 1 or k == 0, q   # the old last chunk is always touched
            assert not eb, q
    assert seen == {(SERVE, False), (SERVE, True), (SAME, False), (ARG, True), (NO_INDEX, True)}


def test_the_edges_the_contract_names():
    S = 100000
    assert grow_of(S, 15, MAX_CHUNKS * C, 1)[0] == NO_INDEX
    assert grow_of(S, 15, MAX_CHUNKS * C - 1, 1)[:4] == (SERVE, True, MAX_CHUNKS * C, MAX_CHUNKS)
    assert grow_of(S, 15, 0xFFFFFFFF, 2)[0] == ARG and grow_of(S, 15, 0xFFFFFFFE, 1)[0] == NO_INDEX
    assert grow_of(S, 15, S + 9, 0)[0] == SAME
    # an append: the old last chunk is the one edge chunk; a patch from a chunk's first byte needs no decode
    assert grow_of(S, 15, S, 64)[4:] == (3, 3, 1, True, False)
    assert grow_of(2 * C, 15, 2 * C, 1)[2:] == (2 * C + 1, 3, 1, 2, 2, True, False)
    assert grow_of(S, 15, 3 * C, S - 3 * C + 9)[4:] == (3, 3, 1, False, False)
    assert grow_of(S, 15, C, 3 * C + 100)[4:] == (1, 4, 4, False, False)
    assert grow_of(S, 15, S + 2 * C + 7, 5)[2:] == (S + 2 * C + 12, 6, 3, 5, 3, True, False)

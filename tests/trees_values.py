"""Inputs of the trees conformance tests (test infrastructure): a corpus that covers every arm of block planning.

Every value is NUL-free, at most 16382 bytes and one deflate block (under 16383 symbols), so at level 9 its block is
planned by one lane of deflate_trees_kernel (csrc/pmc_deflate_split.hip, LaneTrees) when its batch takes the split
pipeline.  The values were picked by search: candidates of make() were classified by the oracle's block facts
(oracle/pmc_oracle.h: oracle_block_facts) and the dissected tree header, and a small covering set of the classes of
classes_of() was kept.  Only the parameters that regenerate the kept values are held here (PARAMS); the coverage
they give is asserted by tests/test_trees_model.py, not assumed.

Shared by tests/test_trees_model.py (CPU), tests/test_gpu_trees.py and tests/golden/make_trees_golden.py, so all
three speak of the same bytes.
"""
import functools
import hashlib
import json
import os
import re

import numpy as np

import deflate_dissect as DD

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MAX_LEN = 16382        # the longest value of the split pipeline's small pass
MAX_SYMBOLS = 16383    # a block is flushed at 16383 symbols (lit_bufsize - 1)
ONE_K = 1024           # chunks of values of at most 1 KiB run the kTreesCap1K instance


def capacities():
    """(kTreesCap1K, kTreesCap, kHdrMinLen) of this build: the defaults in csrc/pmc_kernels.hpp, which the
    Makefile does not override."""
    root = os.path.dirname(HERE)
    text = open(os.path.join(root, "poor-man-s-cache_amd", "csrc", "pmc_kernels.hpp")).read()
    mk = open(os.path.join(root, "poor-man-s-cache_amd", "Makefile")).read()
    assert "PMC_TREES_CAP" not in mk, "the Makefile sets a heap capacity: read it from there"
    cap1k = int(re.search(r"#define PMC_TREES_CAP1K (\d+)", text).group(1))
    cap = int(re.search(r"#define PMC_TREES_CAP (\d+)", text).group(1))
    hdr = int(re.search(r"kHdrMinLen = (\d+)", text).group(1))
    return cap1k, cap, hdr


# ---- the generator -----------------------------------------------------------------------------------------
def _weights(kind, k, ratio):
    if kind == "u":    # uniform
        w = np.ones(k)
    elif kind == "g":  # geometric: w[i] = ratio ** i
        w = ratio ** np.arange(k, dtype=np.float64)
    elif kind == "f":  # Fibonacci: the deepest Huffman tree a histogram can give
        w = np.ones(k)
        for i in range(2, k):
            w[i] = w[i - 1] + w[i - 2]
        w = w[::-1].copy()
    else:
        raise KeyError(kind)
    return w / w.sum()


def make(kind, k, n, seed, start=-1, ratio=0.9, rep=0, maxrep=258, exact=False):
    """n bytes over an alphabet of k symbols weighted by `kind`; start >= 1: the alphabet is start .. start + k - 1,
    else k random byte values.  rep: that many slices of 3 .. maxrep bytes are copied from one place of the value
    to another (matches at every distance the value allows).  exact: every symbol appears (round(n * w) times,
    at least once), shuffled, instead of n independent draws."""
    rng = np.random.default_rng([seed, k, n])
    if start >= 1:
        assert start + k <= 256
        alpha = np.arange(start, start + k, dtype=np.uint8)
    else:
        alpha = (rng.permutation(255)[:k] + 1).astype(np.uint8)
    w = _weights(kind, k, ratio)
    if exact:
        cnt = np.maximum(1, np.round(w * n)).astype(np.int64)
        buf = np.repeat(alpha, cnt)
        rng.shuffle(buf)
        buf = buf[:n] if len(buf) >= n else np.concatenate([buf, rng.choice(alpha, n - len(buf), p=w)])
    else:
        buf = rng.choice(alpha, n, p=w)
    for _ in range(rep):
        ln = int(rng.integers(3, min(maxrep, max(3, n // 2)) + 1))
        if n < 2 * ln + 1:
            break
        a = int(rng.integers(0, n - 2 * ln))
        b = int(rng.integers(a + ln, n - ln + 1))
        buf[b:b + ln] = buf[a:a + ln].copy()
    out = buf.tobytes()
    assert len(out) == n and 0 not in out
    return out


# ---- classification ----------------------------------------------------------------------------------------
def header_lengths(member):
    """(hlit, hdist, hclen, lit/len lengths, distance lengths) of the dynamic block a member starts with, from
    its tree header alone (the tokens are not decoded)."""
    br = DD.Bits(member, 10)
    last, typ = br.get(1), br.get(2)
    assert typ == 2
    hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[DD.ORDER[k]] = br.get(3)
    cdec = DD._decoder(cl)
    lens = []
    while len(lens) < hlit + hdist:
        s = DD._sym(br, cdec)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + br.get(2))
        elif s == 17:
            lens += [0] * (3 + br.get(3))
        else:
            lens += [0] * (11 + br.get(7))
    assert len(lens) == hlit + hdist
    return hlit, hdist, hclen, lens[:hlit], lens[hlit:]


def runs(lens):
    """The maximal runs of equal code lengths of one tree, as scan_tree walks it: [(length, count)]."""
    out = []
    for x in lens:
        if out and out[-1][0] == x:
            out[-1][1] += 1
        else:
            out.append([x, 1])
    return [(a, b) for a, b in out]


ZERO_RUNS = (2, 3, 10, 11, 138, 139)   # both sides of scan_tree's zero-run thresholds
NONZERO_RUNS = (3, 4, 7, 8)            # ... and of its repeat thresholds (one literal plus REP_3_6)
HCLENS = (14, 16, 17, 18)
HLITS = (257, 258, 286)
DYN_LENGTHS = (511, 512, 513, 514)     # both sides of kHdrMinLen


def facts_of(value):
    """(the oracle's member, the block facts) of a value; the value must be one block."""
    from oracle import pyoracle as O
    member = O.compress(value)
    facts = O.last_block_facts()
    assert len(facts) == 1, len(facts)
    return member, facts[0]


def classes_of(value, member, f, caps=None):
    """The classes of the coverage table a value falls in (a set of names).  Classes that show only in a dynamic
    block's bytes (hclen, hlit, the runs) are given to dynamic blocks alone; every other class gets a second name
    with ":dyn" appended when the block is dynamic."""
    cap1k, cap, hdr = caps or capacities()
    out = set()
    dyn = f["type"] == 2
    nz, dl = f["leaves"][0], f["leaves"][1]
    c, tag = (cap1k, "1k") if len(value) <= ONE_K else (cap, "16k")
    for d in (-1, 0, 1, 2):
        if nz == c + d:
            out.add(f"nz{tag}=CAP{d:+d}")
    if nz >= 200:
        out.add("nz>=200")
    if nz == 2:
        out.add("nz=2")
    if dl <= 2:
        out.add(f"dleaves={dl}")
    if dl >= 20:
        out.add("dleaves>=20")
    if f["max_code"][1] >= 26:
        out.add("dcode>=26")
    if f["overflow"][2]:
        out.add("bl-overflow")
    if f["overflow"][1]:
        out.add("d-overflow")
    if f["overflow"][0]:
        out.add("ll-overflow")
    if sum(f["depth_ties"]):
        out.add("depth-tie")
    if f["depth_ties"][0]:
        out.add("depth-tie-ll")
    # the block choice, as _tr_flush_block makes it
    opt_lenb, static_lenb, stored = (f["opt_len"] + 10) >> 3, (f["static_len"] + 10) >> 3, f["stored_len"]
    best = min(opt_lenb, static_lenb)
    if f["type"] == 0:
        assert stored + 4 <= best
        out.add("stored<" if stored + 4 < best else "stored-tie")
    elif f["type"] == 1:
        assert static_lenb <= opt_lenb and stored + 4 > best
        out.add("fixed<" if static_lenb < opt_lenb else "fixed-tie")
    else:
        assert static_lenb > opt_lenb and stored + 4 > opt_lenb
        if static_lenb == opt_lenb + 1:
            out.add("dyn-static+1")
        if stored + 4 == opt_lenb + 1:
            out.add("dyn-stored+1")
    out |= {f"{c}:dyn" for c in out if dyn and not c.startswith(("stored", "fixed", "dyn-"))}
    if dyn:
        hlit, hdist, hclen, ll, dlens = header_lengths(member)
        assert hlit == f["max_code"][0] + 1 and hdist == f["max_code"][1] + 1 and hclen == f["max_blindex"] + 1
        out.add(f"hclen={hclen}")
        if hlit in HLITS:
            out.add(f"hlit={hlit}")
        if len(value) in DYN_LENGTHS:
            out.add(f"dyn-len={len(value)}")
        for x, cnt in runs(ll) + runs(dlens):
            if x == 0 and cnt in ZERO_RUNS:
                out.add(f"zrun={cnt}")
            if x != 0 and cnt in NONZERO_RUNS:
                out.add(f"run={cnt}")
    return out


def required(caps=None):
    """{class: the least number of values} of the coverage table.  ":dyn" rows: the class must also show in a
    dynamic block's bytes.  nz = 2 has no such row: one literal and the end-of-block code are a value of one to
    three equal bytes, whose fixed block of at most 34 bits no dynamic header (at least 14 + 3 * 4 bits before
    the first code length) can beat."""
    need = {}
    for tag in ("1k", "16k"):
        for d in (-1, 0, 1, 2):
            need[f"nz{tag}=CAP{d:+d}"] = 3
            need[f"nz{tag}=CAP{d:+d}:dyn"] = 1
    for c in ("nz>=200", "dleaves=0", "dleaves=1", "dleaves=2", "dleaves>=20", "dcode>=26", "bl-overflow"):
        need[c] = 3
        need[c + ":dyn"] = 1
    need["nz=2"] = 3
    for c in ("stored<", "stored-tie", "fixed-tie", "fixed<", "dyn-static+1", "dyn-stored+1"):
        need[c] = 3
    for h in HCLENS:
        need[f"hclen={h}"] = 3
    for h in HLITS:
        need[f"hlit={h}"] = 3
    for n in DYN_LENGTHS:
        need[f"dyn-len={n}"] = 3
    for r in ZERO_RUNS:
        need[f"zrun={r}"] = 3
    for r in NONZERO_RUNS:
        need[f"run={r}"] = 3
    need["depth-tie"] = 10
    return need


# Wanted, not required: reported by the model test, never asserted
WANTED = ("ll-overflow", "d-overflow", "hclen=other")


# ---- the kept values ---------------------------------------------------------------------------------------
# make()'s arguments of every kept value: (kind, k, n, seed, start, ratio, rep, maxrep, exact)
PARAMS = [
    ('u', 1, 1, 0, -1, 0.9, 0, 258, False),
    ('u', 1, 1, 1, -1, 0.9, 0, 258, False),
    ('u', 1, 1, 2, -1, 0.9, 0, 258, False),
    ('u', 3, 16, 115, -1, 0.9, 0, 12, False),
    ('g', 16, 18, 142, -1, 0.7, 0, 12, False),
    ('g', 120, 19, 253, -1, 0.7, 0, 12, False),
    ('u', 5, 22, 159, -1, 0.9, 0, 12, False),
    ('u', 16, 25, 191, -1, 0.9, 0, 12, False),
    ('g', 5, 26, 187, -1, 0.7, 0, 12, False),
    ('u', 5, 30, 215, -1, 0.9, 0, 12, False),
    ('u', 8, 32, 232, -1, 0.9, 0, 12, False),
    ('u', 8, 38, 274, -1, 0.9, 0, 12, False),
    ('g', 255, 41, 542, -1, 0.7, 1, 12, False),
    ('u', 5, 44, 313, -1, 0.9, 1, 12, False),
    ('g', 8, 46, 330, -1, 0.7, 0, 12, False),
    ('u', 3, 48, 339, -1, 0.9, 0, 12, False),
    ('u', 5, 49, 348, -1, 0.9, 1, 12, False),
    ('g', 255, 50, 605, -1, 0.7, 0, 12, False),
    ('g', 8, 52, 372, -1, 0.7, 0, 12, False),
    ('g', 40, 53, 411, -1, 0.7, 0, 12, False),
    ('u', 5, 55, 390, -1, 0.9, 1, 12, False),
    ('u', 16, 55, 401, -1, 0.9, 0, 12, False),
    ('g', 8, 56, 400, -1, 0.7, 3, 12, False),
    ('g', 16, 57, 415, -1, 0.7, 3, 12, False),
    ('g', 120, 58, 526, -1, 0.7, 3, 12, False),
    ('u', 16, 58, 422, -1, 0.9, 1, 12, False),
    ('g', 120, 59, 533, -1, 0.7, 3, 12, False),
    ('g', 255, 60, 675, -1, 0.7, 3, 12, False),
    ('g', 255, 62, 689, -1, 0.7, 1, 12, False),
    ('u', 3, 62, 437, -1, 0.9, 0, 12, False),
    ('g', 120, 63, 561, -1, 0.7, 1, 12, False),
    ('g', 120, 64, 568, -1, 0.7, 0, 12, False),
    ('g', 120, 65, 575, -1, 0.7, 0, 12, False),
    ('g', 40, 66, 502, -1, 0.7, 3, 12, False),
    ('g', 16, 67, 485, -1, 0.7, 1, 12, False),
    ('g', 8, 68, 484, -1, 0.7, 3, 12, False),
    ('u', 8, 69, 491, -1, 0.9, 3, 12, False),
    ('u', 8, 70, 498, -1, 0.9, 0, 12, False),
    ('u', 5, 71, 502, -1, 0.9, 1, 12, False),
    ('u', 5, 72, 509, -1, 0.9, 0, 12, False),
    ('g', 5, 73, 516, -1, 0.7, 0, 12, False),
    ('u', 3, 74, 521, -1, 0.9, 3, 12, False),
    ('g', 120, 75, 645, -1, 0.7, 1, 12, False),
    ('u', 2, 75, 527, -1, 0.9, 3, 12, False),
    ('g', 16, 76, 548, -1, 0.7, 3, 12, False),
    ('g', 16, 77, 555, -1, 0.7, 0, 12, False),
    ('u', 8, 78, 554, -1, 0.9, 3, 12, False),
    ('g', 40, 79, 593, -1, 0.7, 0, 12, False),
    ('u', 8, 79, 561, -1, 0.9, 1, 12, False),
    ('u', 5, 100, 705, -1, 0.9, 1, 12, False),
    ('u', 255, 100, 955, -1, 0.9, 3, 12, False),
    ('u', 4, 120, 400, -1, 0.7, 10, 258, True),
    ('u', 140, 120, 447, -1, 0.85, 0, 258, False),
    ('u', 3, 150, 1053, -1, 0.9, 0, 12, False),
    ('u', 40, 150, 1090, -1, 0.9, 3, 12, False),
    ('u', 8, 200, 1408, -1, 0.9, 1, 12, False),
    ('g', 5, 300, 139, 139, 0.9, 0, 258, True),
    ('g', 20, 300, 10, 10, 0.9, 0, 258, True),
    ('g', 60, 300, 138, 138, 0.9, 0, 258, True),
    ('g', 120, 300, 2220, -1, 0.7, 0, 12, False),
    ('u', 3, 300, 2103, -1, 0.9, 1, 12, False),
    ('u', 5, 300, 139, 139, 0.9, 0, 258, True),
    ('u', 20, 300, 139, 139, 0.9, 0, 258, True),
    ('f', 140, 400, 397, -1, 0.85, 0, 258, True),
    ('g', 17, 400, 387, -1, 0.85, 10, 258, False),
    ('g', 200, 400, 303, -1, 0.85, 2, 258, True),
    ('u', 15, 400, 16, 40, 0.9, 4, 258, True),
    ('u', 39, 400, 39, 40, 0.9, 0, 258, True),
    ('u', 71, 400, 72, 40, 0.9, 4, 258, True),
    ('u', 200, 400, 81, -1, 0.95, 0, 258, True),
    ('g', 10, 511, 0, -1, 0.9, 3, 258, False),
    ('u', 10, 511, 0, -1, 0.9, 0, 258, False),
    ('u', 10, 511, 1, -1, 0.9, 0, 258, False),
    ('g', 10, 512, 0, -1, 0.9, 3, 258, False),
    ('u', 10, 512, 0, -1, 0.9, 0, 258, False),
    ('u', 10, 512, 1, -1, 0.9, 0, 258, False),
    ('u', 100, 512, 0, -1, 0.9, 0, 258, False),
    ('g', 10, 513, 0, -1, 0.9, 3, 258, False),
    ('u', 10, 513, 0, -1, 0.9, 0, 258, False),
    ('u', 10, 513, 1, -1, 0.9, 0, 258, False),
    ('g', 10, 514, 0, -1, 0.9, 3, 258, False),
    ('u', 10, 514, 0, -1, 0.9, 0, 258, False),
    ('u', 10, 514, 1, -1, 0.9, 0, 258, False),
    ('u', 100, 514, 1, -1, 0.9, 0, 258, False),
    ('g', 120, 600, 260, -1, 0.95, 2, 258, False),
    ('g', 77, 700, 0, -1, 0.97, 0, 258, True),
    ('g', 78, 700, 0, -1, 0.97, 0, 258, True),
    ('g', 79, 700, 0, -1, 0.97, 0, 258, True),
    ('u', 75, 700, 0, -1, 0.9, 0, 258, False),
    ('u', 75, 700, 0, -1, 0.9, 3, 258, False),
    ('u', 75, 700, 1, -1, 0.9, 3, 258, False),
    ('u', 76, 700, 0, -1, 0.9, 0, 258, True),
    ('u', 76, 700, 0, -1, 0.9, 3, 258, False),
    ('u', 78, 700, 1, -1, 0.9, 2, 3, True),
    ('u', 81, 700, 2, -1, 0.9, 0, 258, True),
    ('g', 79, 900, 2, -1, 0.97, 0, 258, True),
    ('g', 82, 900, 0, -1, 0.97, 0, 258, True),
    ('u', 77, 900, 1, -1, 0.9, 2, 3, True),
    ('u', 79, 900, 1, -1, 0.9, 3, 258, False),
    ('g', 4, 1000, 198, -1, 0.95, 2, 258, False),
    ('g', 50, 1000, 976, -1, 0.7, 0, 258, False),
    ('g', 140, 1000, 103, -1, 0.85, 2, 258, False),
    ('u', 75, 1000, 0, -1, 0.9, 3, 258, False),
    ('u', 76, 1000, 0, -1, 0.9, 0, 258, False),
    ('u', 81, 1000, 2, -1, 0.9, 3, 258, False),
    ('u', 200, 1000, 514, -1, 0.7, 2, 258, False),
    ('u', 200, 1000, 592, -1, 0.5, 0, 258, False),
    ('g', 79, 1024, 0, -1, 0.97, 0, 258, True),
    ('g', 80, 1024, 1, -1, 0.97, 0, 258, True),
    ('u', 74, 1024, 2, -1, 0.9, 2, 3, True),
    ('u', 76, 1024, 2, -1, 0.9, 0, 258, True),
    ('u', 77, 1024, 2, -1, 0.9, 3, 258, False),
    ('u', 78, 1024, 0, -1, 0.9, 2, 3, True),
    ('u', 80, 1024, 0, -1, 0.9, 0, 258, False),
    ('g', 82, 1025, 0, -1, 0.97, 0, 258, True),
    ('g', 82, 1025, 1, -1, 0.97, 0, 258, True),
    ('g', 82, 1025, 2, -1, 0.97, 0, 258, True),
    ('g', 83, 1025, 0, -1, 0.97, 0, 258, True),
    ('g', 83, 1025, 1, -1, 0.97, 0, 258, True),
    ('g', 83, 1025, 2, -1, 0.97, 0, 258, True),
    ('g', 84, 1025, 0, -1, 0.97, 0, 258, True),
    ('u', 79, 1025, 2, -1, 0.9, 2, 3, True),
    ('u', 80, 1025, 1, -1, 0.9, 3, 258, False),
    ('u', 80, 1025, 2, -1, 0.9, 3, 258, False),
    ('u', 81, 1025, 0, -1, 0.9, 3, 258, False),
    ('u', 81, 1025, 2, -1, 0.9, 0, 258, False),
    ('u', 82, 1025, 0, -1, 0.9, 3, 258, False),
    ('u', 83, 1025, 1, -1, 0.9, 2, 3, True),
    ('u', 86, 1025, 0, -1, 0.9, 0, 258, True),
    ('g', 35, 1500, 35, 40, 0.8, 0, 258, True),
    ('u', 4, 1500, 4, 40, 0.9, 0, 258, True),
    ('u', 68, 1500, 69, 40, 0.9, 4, 258, True),
    ('u', 82, 1500, 0, -1, 0.9, 0, 258, False),
    ('u', 83, 1500, 2, -1, 0.9, 3, 258, False),
    ('u', 85, 1500, 1, -1, 0.9, 0, 258, False),
    ('g', 5, 2000, 138, 138, 0.9, 0, 258, True),
    ('u', 5, 2000, 10, 10, 0.9, 0, 258, True),
    ('u', 5, 2000, 138, 138, 0.9, 0, 258, True),
    ('u', 60, 2000, 138, 138, 0.9, 0, 258, True),
    ('f', 2, 2500, 716, -1, 0.95, 10, 258, False),
    ('f', 9, 2500, 270, -1, 0.95, 0, 258, True),
    ('f', 30, 2500, 913, -1, 0.95, 0, 258, False),
    ('f', 90, 2500, 471, -1, 0.5, 10, 258, False),
    ('f', 200, 2500, 481, -1, 0.7, 10, 258, True),
    ('g', 200, 2500, 658, -1, 0.5, 0, 258, True),
    ('u', 9, 2500, 628, -1, 0.7, 2, 258, True),
    ('u', 30, 2500, 828, -1, 0.95, 10, 258, True),
    ('g', 60, 3000, 10, 186, 0.9, 0, 258, True),
    ('g', 82, 3000, 2, -1, 0.97, 0, 258, True),
    ('g', 86, 3000, 1, -1, 0.97, 0, 258, True),
    ('u', 81, 3000, 0, -1, 0.9, 0, 258, False),
    ('u', 82, 3000, 2, -1, 0.9, 0, 258, True),
    ('u', 86, 3000, 0, -1, 0.9, 3, 258, False),
    ('u', 8, 5000, 9, 40, 0.9, 4, 258, True),
    ('u', 80, 9000, 110, -1, 0.9, 30, 258, False),
    ('u', 2, 12000, 267, -1, 0.95, 60, 258, True),
    ('u', 140, 12000, 207, -1, 0.85, 60, 258, True),
    ('u', 200, 12000, 15, -1, 0.85, 60, 258, True),
    ('g', 230, 16382, 0, -1, 0.985, 20, 258, True),
    ('g', 230, 16382, 1, -1, 0.985, 20, 258, True),
    ('u', 140, 16382, 599, -1, 0.95, 60, 258, False),
    ('u', 200, 16382, 730, -1, 0.95, 60, 258, False),
]


@functools.lru_cache(maxsize=None)
def values():
    """The corpus, in PARAMS order."""
    out = [make(*p) for p in PARAMS]
    assert len(set(out)) == len(out)
    return out


def sha(b):
    return hashlib.sha256(b).hexdigest()


def batch(name):
    """The values of a GPU batch, as indices into values().
    "1k": the values of at most 1024 bytes, cycled to 4224 -- above the one-kernel path's 1024-value limit, so the
    split pipeline's kTreesCap1K instance and its deferred list run, and at least 4096, from which a chunk's lanes
    visit the values in cO order.
    "16k": every value, cycled to 4224 -- the kTreesCap instance.
    "mono": every value of at most 4096 bytes, once (at most 1024 values: the one-kernel device path).
    "all": every value once (the switches' child processes and the latency entry).
    The cycled batches are shuffled (seeded), so a wave's lanes hold heaps of unequal size."""
    vs = values()
    if name in ("1k", "16k"):
        idx = [i for i, v in enumerate(vs) if name == "16k" or len(v) <= ONE_K]
        idx = (idx * (4224 // len(idx) + 1))[:4224]
        return [int(i) for i in np.random.default_rng(len(idx) + len(name)).permutation(idx)]
    if name == "mono":
        return [i for i, v in enumerate(vs) if len(v) <= 4096]
    if name == "all":
        return list(range(len(vs)))
    raise KeyError(name)


class TreesGolden:
    """tests/golden/trees_golden.json (tests/golden/make_trees_golden.py): the reference's member of every value,
    as SHA-256 + length, keyed by the value's SHA-256."""

    def __init__(self):
        with open(os.path.join(GOLDEN, "trees_golden.json")) as f:
            self.vectors = json.load(f)["vectors"]

    def mismatches(self, vals, members):
        """Indices whose member is not the reference's (or whose value has no vector)."""
        bad = []
        for k, (v, m) in enumerate(zip(vals, members)):
            want = self.vectors.get(sha(v))
            if want is None or len(m) != want["gz_len"] or sha(m) != want["gz_sha256"]:
                bad.append(k)
        return bad

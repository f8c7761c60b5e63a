"""The large-value pipeline (csrc/pmc_deflate_large.hip), restated in Python on top of the oracle's facts (test
infrastructure): the normative statement tests/test_large_model.py holds the corpus of tests/large_conf_values.py
to, and tests/test_gpu_large_conf.py the kernels.

  nseg       a value of n bytes is cut into max(1, n // SEG) segments of SEG positions; the last one holds the rest,
             SEG .. 2 SEG - 1 positions (every n >= SEG).
  parse      segment j is parsed by deflate_slow from a fresh state at s = j SEG, chains over the whole value, on
             through OVERLAP positions of the next segment (oracle_parse_from states exactly that).  Each parse
             records, at every loop top with no pending match, its state code (1: no literal pending, 2: one) and
             its token count -- in its first OVERLAP positions (the start region) and, unless it is the last, in
             the OVERLAP positions from its end e (the continuation region).
  stitch     per boundary e: the first offset x < OVERLAP at which the parse of segment j (continuation region) and
             the parse of segment j + 1 (start region) both recorded the same non-zero code.  Segment j's tokens end
             at its count there, segment j + 1's begin at its count there.
  splice     the segments' token ranges, back to back, are the tokens of zlib's one serial parse.
  failure    a value with a boundary that has no such offset is redone by the gated HBM kernel.
  HC         per position p <= n - 3: 0 where zlib does not search at p (no earlier position of p's hash, the
             nearest one is position 0, or lies beyond MAX_DIST, or is the window base itself, base_hides()), else
             the earlier positions of that hash, position 0 left out, capped at 255.
  base       the window base at a loop top t, as a closed form of t and n (window_base), next to the base that the
             dp encoder keeps step by step (oracle_base_diffs counts the loop tops where they differ).

The constants are read from csrc/pmc_plan.hpp, so a changed segment, overlap or sort chunk fails here."""
import functools
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
W_SIZE, MIN_LOOKAHEAD = 32768, 262
MAX_DIST = W_SIZE - MIN_LOOKAHEAD
SLIDE_AT = W_SIZE + MAX_DIST  # 65274: fill_window slides at a loop top this far past the base


@functools.lru_cache(maxsize=None)
def constants():
    root = os.path.join(os.path.dirname(HERE), "poor-man-s-cache_amd", "csrc")
    plan = open(os.path.join(root, "pmc_plan.hpp")).read()
    large = open(os.path.join(root, "pmc_deflate_large.hip")).read()
    seg, overlap, chunk = map(int, re.search(
        r"constexpr uint32_t kLvSeg = (\d+), kLvOverlap = (\d+), kLvChunk = (\d+);", plan).groups())
    assert "return exact() ? std::max<uint64_t>(1, len / kLvSeg)" in plan
    assert "constexpr uint32_t kLvMaxDist = 32768 - 262, kLvTooFar = 4096;" in large
    # the rank kernel's look-back for the run start of a chunk's first entry, and the count's cap
    assert "for (uint32_t b = 0; b < 256 && b < k.c0; b += 64)" in large and "(cnt < 255 ? cnt : 255)" in large
    return {"seg": seg, "overlap": overlap, "chunk": chunk, "lookback": 256, "hc_cap": 255, "step": 64}


def nseg(n):
    return max(1, n // constants()["seg"])


def segments(n):
    """[(s, e, eo, last)]: a segment's start, its end, the end of its parse, and whether it is the last."""
    c = constants()
    out = []
    ns = nseg(n)
    for j in range(ns):
        last = j + 1 == ns
        s = j * c["seg"]
        e = n if last else s + c["seg"]
        out.append((s, e, n if last else min(e + c["overlap"], n), last))
    return out


def window_base(t, n):
    """The window base at a loop top t of a value of n bytes: fill_window runs when the lookahead is short (the
    window's end, or the value's, is nearer than MIN_LOOKAHEAD) and slides when t is SLIDE_AT past the base."""
    B = 0
    while True:
        wend = min(n, B + 2 * W_SIZE)
        if t - B >= SLIDE_AT and t + MIN_LOOKAHEAD > wend:
            B += W_SIZE
        else:
            return B


def base_hides(p, n):
    """True where the window base at loop top p is exactly p - MAX_DIST: the one candidate the distance limit
    admits and slide_hash turns into NIL.  For any other p the base lies below p - MAX_DIST.  (t - B == SLIDE_AT
    with the value's end nearer than MIN_LOOKAHEAD: the slide fill_window makes at p itself.)"""
    return p >= SLIDE_AT and (p - SLIDE_AT) % W_SIZE == 0 and n - p < MIN_LOOKAHEAD


def hashes(value):
    b = np.frombuffer(value, np.uint8).astype(np.uint32)
    return ((b[:-2] << 10) ^ (b[1:-1] << 5) ^ b[2:]) & 0x7fff


def hc_of(value):
    """HC of every position p <= n - 3 (uint8), and the sorted array S (stable by hash)."""
    from oracle import pyoracle as O
    c = constants()
    n = len(value)
    h = hashes(value)
    S = np.argsort(h, kind="stable")
    R = np.empty_like(S)
    R[S] = np.arange(len(S))
    prev = np.full(len(S), -1, np.int64)  # the nearest earlier position of the same hash
    same = h[S[1:]] == h[S[:-1]]
    prev[S[1:][same]] = S[:-1][same]
    p = np.arange(len(S))
    search = (prev > 0) & (p - prev <= MAX_DIST)
    for t in range(SLIDE_AT, n, W_SIZE):  # (the positions base_hides() can name)
        if t < len(S) and base_hides(t, n) and prev[t] == t - MAX_DIST:
            search[t] = False
    cnt = np.minimum(O.chain_counts(value), c["hc_cap"])
    return np.where(search, cnt, 0).astype(np.uint8), S


class Parse:
    """One segment's speculative parse: states and tokens of oracle_parse_from, and the two recorded regions as
    arrays of OVERLAP words (code << 30 | token count, 0 where nothing was recorded)."""

    def __init__(self, value, s, e, eo, last, run_code2=None):
        from oracle import pyoracle as O
        ov = constants()["overlap"]
        self.s, self.e, self.eo, self.last = s, e, eo, last
        self.states, self.tokens = O.parse_from(value, s, eo)
        pos = self.states["pos"].astype(np.int64)
        if run_code2 is not None:  # (a wrong pipeline, for the tests: every state of a no-search position is 2)
            self.states["code"][run_code2[pos]] = 2
        word = (self.states["code"].astype(np.int64) << 30) | self.states["ntok"].astype(np.int64)
        self.spec = np.zeros(ov, np.int64)
        m = pos - s < ov
        self.spec[pos[m] - s] = word[m]
        self.cont = np.zeros(ov, np.int64)
        if not last:
            m = (pos >= e) & (pos - e < ov)
            self.cont[pos[m] - e] = word[m]


class Stitched:
    """What the pipeline makes of a value: found[g] the coincidence offset of boundary g (None: the value fails),
    clash[g] whether an earlier offset held two different non-zero codes, ranges[j] the token range of segment j,
    and tokens() the spliced stream (TOKEN_DTYPE) of a value that did not fail."""

    def __init__(self, value, relaxed=False, run_code2=False):
        """relaxed / run_code2 state two wrong pipelines, for the tests that show the corpus tells them from the
        right one: the stitch takes the first offset where both parses recorded any state; the parse records code
        2 at every loop top without a search."""
        self.n = len(value)
        zero = None
        if run_code2:
            zero = np.concatenate([hc_of(value)[0] == 0, [True, True]])
        self.parses = [Parse(value, *sg, run_code2=zero) for sg in segments(self.n)]
        self.found, self.clash = [], []
        for a, b in zip(self.parses, self.parses[1:]):
            x, y = a.cont >> 30, b.spec >> 30
            hit = np.flatnonzero((x != 0) & ((y != 0) if relaxed else (x == y)))
            at = int(hit[0]) if len(hit) else None
            self.found.append(at)
            differ = np.flatnonzero((x != 0) & (y != 0) & (x != y))
            self.clash.append(bool(len(differ) and (at is None or differ[0] < at)))
        self.failed = any(f is None for f in self.found)
        self.ranges = []
        if not self.failed:
            t1 = 0
            for j, p in enumerate(self.parses):
                t2 = len(p.tokens) if p.last else int(p.cont[self.found[j]] & 0x3fffffff)
                self.ranges.append((t1, t2))
                if not p.last:
                    t1 = int(self.parses[j + 1].spec[self.found[j]] & 0x3fffffff)

    def tokens(self):
        assert not self.failed
        return np.concatenate([p.tokens[a:b] for p, (a, b) in zip(self.parses, self.ranges)])

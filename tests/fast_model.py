"""The fast level's parse (PMC_LEVEL_FAST), stated in plain Python: the normative form of the
specification DESIGN.md §4 "Front, fast level" quotes.  csrc/pmc_deflate_fast.hip computes the same
token sequence on the GPU; tests/test_gpu_fast.py compares the two token by token.

Tokens are in the form tests/deflate_dissect.py returns: an int for a literal byte, (len, dist) for
a match.
"""

K = 2        # candidates tried per position
LAZY = 1     # one-step lazy rule on
CAPT = 32    # match lengths in the table are capped here; a capped match is extended when emitted
MAX_MATCH = 258
TOO_FAR = 4096
FAST_MAX = 16382  # values above this take the exact paths


def hash3(v, p):
    """zlib's hash of the three bytes at p (15 bits)."""
    return ((v[p] << 10) ^ (v[p + 1] << 5) ^ v[p + 2]) & 0x7FFF


def match_table(v):
    """ml[p], mq[p] for every position: they depend on the value only, not on the parse."""
    n = len(v)
    ml, mq = [0] * n, [0] * n
    runs = {}  # hash -> earlier positions with that hash, in increasing order
    for p in range(0, n - 2):
        h = hash3(v, p)
        run = runs.setdefault(h, [])
        # the up-to-K nearest earlier positions of the run; a hash collision keeps its slot,
        # position 0 is never a candidate (zlib's NIL)
        cands = [q for q in run[-K:][::-1] if q != 0]
        cap = min(CAPT, n - p)
        best, bq = 0, 0
        for q in cands:  # nearest first: ties stay with the nearest
            t = 0
            while t < cap and v[q + t] == v[p + t]:
                t += 1
            if t > best:
                best, bq = t, q
        if best == 3 and p - bq > TOO_FAR:
            best = 0
        if best >= 3:
            ml[p], mq[p] = best, bq
        run.append(p)
    return ml, mq


def fast_tokens(value):
    v = bytes(value)
    n = len(v)
    assert n <= FAST_MAX
    ml, mq = match_table(v)
    toks = []
    p = 0
    while p < n:
        m = ml[p]
        if m >= 3 and not (LAZY and p + 1 < n and ml[p + 1] > m):
            q = mq[p]
            if m == CAPT:
                lim = min(MAX_MATCH, n - p)
                while m < lim and v[q + m] == v[p + m]:
                    m += 1
            toks.append((m, p - q))
            p += m
        else:
            toks.append(v[p])
            p += 1
    return toks


def replay(toks):
    """The bytes a token sequence stands for."""
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            ln, dist = t
            for _ in range(ln):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)

"""Dictionary training (include/pmc_codec.h "dictionary training"), stated in plain Python: the normative form of
the algorithm DESIGN.md §4 "Dictionary training" quotes.  csrc/pmc_dict_train.hip computes the same bytes on the
GPU (tests/test_gpu_dict_train.py) and tests/host/dict_train_check.cpp on the CPU (tests/test_host_dict_train.py).

The algorithm is this project's own, a simplified FASTCOVER: it aims at byte parity with no other tool.

  Count.      freq[h(p)] += 1 for every position p of every sample with p + 8 <= len (u32 slots, 2^F of them).
  Epochs.     E = D / 64; epoch e owns the samples [e n // E, (e + 1) n // E) and runs after epoch e - 1.
  Score.      Every start q of an owned sample with q + 64 <= len is a candidate; its score is the sum of freq[h]
              over the 57 positions of the segment, a hash value counted once, at its first position in the window.
  Selection.  The largest score wins, then the lowest sample index, then the lowest start.  No candidate, or a
              best score of 0: nothing is selected.  A selected segment's 57 slots are zeroed.
  Assembly.   The selected segments in reverse order of selection: the first one lies last, next to the value.
"""

D_KMER = 8                 # d: bytes hashed per position
K_SEG = 64                 # K: bytes per segment
F_BITS = 20                # F: the table has 2^F slots
W = K_SEG - D_KMER + 1     # 57 positions per segment
SPAN = 16382               # kDictSpan: a longer sample counts as its first SPAN bytes
MAX_SAMPLES = 262144       # PMC_DICT_TRAIN_MAX_SAMPLES; MAX_SAMPLES * SPAN < 2^32, so no u32 slot wraps
MULT = 0x9E3779B185EBCA87
M64 = (1 << 64) - 1


def valid(n: int, size: int) -> bool:
    return 1 <= n <= MAX_SAMPLES and 64 <= size <= 8192 and size % 64 == 0


def hash8(v: bytes, p: int) -> int:
    """h(p): the 8 bytes at p as a little-endian u64, times MULT mod 2^64, the top F bits."""
    return ((int.from_bytes(v[p:p + D_KMER], "little") * MULT) & M64) >> (64 - F_BITS)


def hashes(v: bytes):
    return [hash8(v, p) for p in range(len(v) - D_KMER + 1)]


def score_direct(freq, h, q: int) -> int:
    """The definition: a hash value counts once per window, at its first position in the window."""
    seen, s = set(), 0
    for j in range(W):
        x = h[q + j]
        if x not in seen:
            seen.add(x)
            s += freq.get(x, 0)
    return s


def score_by_dist(freq, h, q: int) -> int:
    """The per-position form: dist[p] = the smallest t in 1 .. 56 with h[p - t] == h[p]; position p counts in
    window q iff p - dist[p] < q."""
    s = 0
    for p in range(q, q + W):
        t = next((t for t in range(1, W) if p - t >= 0 and h[p - t] == h[p]), None)
        if t is None or p - t < q:
            s += freq.get(h[p], 0)
    return s


def scores(freq, h, nq: int):
    """score_direct for q = 0 .. nq - 1, by sliding the window (the table does not change within an epoch)."""
    out, cnt, s = [], {}, 0
    for p in range(W - 1):
        x = h[p]
        if not cnt.get(x):
            s += freq.get(x, 0)
        cnt[x] = cnt.get(x, 0) + 1
    for q in range(nq):
        x = h[q + W - 1]
        if not cnt.get(x):
            s += freq.get(x, 0)
        cnt[x] = cnt.get(x, 0) + 1
        out.append(s)
        x = h[q]
        cnt[x] -= 1
        if not cnt[x]:
            s -= freq.get(x, 0)
    return out


def train_trace(samples, size: int):
    """(dictionary, trace): trace[e] = None or (score, i, q) of epoch e's selection."""
    n = len(samples)
    assert valid(n, size)
    vs = [bytes(v)[:SPAN] for v in samples]
    hs = [hashes(v) for v in vs]
    freq = {}
    for h in hs:
        for x in h:
            freq[x] = freq.get(x, 0) + 1
    assert all(c < 1 << 32 for c in freq.values())
    E = size // K_SEG
    segs, trace = [], []
    for e in range(E):
        best = None  # (score, i, q)
        for i in range(e * n // E, (e + 1) * n // E):
            nq = len(vs[i]) - K_SEG + 1
            if nq <= 0:
                continue
            for q, s in enumerate(scores(freq, hs[i], nq)):
                if best is None or s > best[0]:  # strictly greater: ties stay with the lowest i, then the lowest q
                    best = (s, i, q)
        if best is None or best[0] == 0:
            trace.append(None)
            continue
        s, i, q = best
        for j in range(W):
            freq[hs[i][q + j]] = 0
        segs.append(vs[i][q:q + K_SEG])
        trace.append(best)
    return b"".join(reversed(segs)), trace


def train(samples, size: int) -> bytes:
    return train_trace(samples, size)[0]

"""Inputs of the large-value conformance tests (test infrastructure): a corpus in which the rules of the large-value
pipeline (csrc/pmc_deflate_large.hip: lv_rank_kernel, LvParse::search, lv_parse_kernel, lv_stitch_kernel, the
emit's window base) each decide a byte of some member.

Follows tests/front_values.py: the values are regenerated from PARAMS (a background of parts laid end to end, then
plants at stated positions), classified by the oracle's facts (oracle/pmc_oracle.h: the search and token logs, the
rule variants, oracle_parse_from) and by tests/large_model.py, and the coverage is asserted by
tests/test_large_model.py, not assumed.

"v:<rule>@<zone>": the dp encoder with that one rule altered makes another member, and a stretch of tokens of the
true parse that the altered parse does not make begins in that zone (the deciding search ran there) -- "seg0" (a first segment: below 16384), "mid" (from 16384 up to the first
slide's loop top, 65274) or "slid" (beyond it).  "v:<rule>": the same without the place.  The other classes are
structural: read from the logs, the model's stitch and the block facts.

Every value of PARAMS is NUL-free and above deflate_big_limit(), so the reference's own Compress makes its member
and the large-value pipeline takes it; NUL_PARAMS is a small group that holds NULs (libz's members).  The
one-segment case of the pipeline is tests/front_values.py's "big" group as it stands.

Shared by tests/test_large_model.py (CPU), tests/test_gpu_large_conf.py and tests/golden/make_large_conf_golden.py.
"""
import functools
import hashlib
import json
import os

import numpy as np

import front_values as FV
import large_model as LM

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BIG_MAX = FV.BIG_MAX
MAX_DIST, W_SIZE, SLIDE_AT = LM.MAX_DIST, LM.W_SIZE, LM.SLIDE_AT
SEG = 16384
ZONES = ("seg0", "mid", "slid")


def zone_of(p):
    return "seg0" if p < SEG else "mid" if p <= SLIDE_AT else "slid"


# ---- the generator -----------------------------------------------------------------------------------------
def _part(part):
    kind = part[0]
    if kind == "u":    # n draws from an alphabet of k bytes (100 .. 100 + k - 1)
        _, n, seed, k = part
        return np.random.default_rng([seed, k, n, 1]).integers(100, 100 + k, n).astype(np.uint8)
    if kind == "ut":   # the first n bytes of ("u", total, seed, k): a length that can be tuned byte by byte
        _, n, seed, k, total = part
        return _part(("u", total, seed, k))[:n].copy()
    if kind == "r":    # n random non-zero bytes: a stored block beats both trees
        _, n, seed = part
        return np.random.default_rng([seed, n, 2]).integers(1, 256, n).astype(np.uint8)
    if kind == "fv":   # a value of front_values.make
        return np.frombuffer(FV.make(*part[1:]), np.uint8).copy()
    raise KeyError(kind)


def _expand(plants):
    """("freshlit", a, L, d): a copy (from d before) that ends at a - 3, the byte 228 there (the hash of a text trigram that begins
    with 100, and no match), and ("fresh", a, L)."""
    out = []
    for pl in plants:
        if pl[0] == "freshlit":
            _, a, L, d = pl
            out += [("copy", a - 33, d, 30), ("byte", a - 3, 228), ("fresh", a, L)]
        else:
            out.append(pl)
    # every "fresh" stretch last, in ascending order: it must know every byte before it
    return [pl for pl in out if pl[0] != "fresh"] + sorted(pl for pl in out if pl[0] == "fresh")


def make(parts, plants, seed=0):
    """The parts laid end to end, then the plants in order ("fresh" ones last, in ascending order).  Bytes 1 .. 31 are `special` (no part uses them but
    front_values' own plants); strings are drawn from 128 .. 255.
      ("copy", i, d, L[, near])  a fresh string of L bytes at i - d and at i, each followed by another special byte
                                 and the one at i preceded by four, so that i is a loop top and the match is exactly
                                 L long; with near > 0 the string's first five bytes also lie at i - near, so that
                                 the far candidate is not the first of the chain
      ("copy0", i, L)            the value's first L bytes again at i (position 0 is NIL)
      ("head0", L)               the value's first L bytes are a fresh string (no trigram of it occurs elsewhere)
      ("kplant", P, ord, period) front_values' 'k' plant on a colliding background: P's only long match lies at the
                                 candidate of ordinal ord
      ("run", a, L, byte)        a period-1 run
      ("fresh", a, L)            L bytes from 128 .. 255 so that no position a - 2 .. a + L - 1 has an earlier
                                 position of its hash: zlib searches at none of these L + 2 positions
      ("freshlit", a, L, d)      the same, entered with a literal pending (_expand)
      ("rand", a, L)             random non-zero bytes
      ("end", L, d)              the value's last L bytes are a copy of those d before them (a match to the end)"""
    buf = np.concatenate([_part(p) for p in parts])
    n = len(buf)
    rng = np.random.default_rng([seed, n, len(plants), 3])
    sp = [int(x) for x in rng.permutation(np.arange(1, 32))]
    spn = 0

    def special():
        nonlocal spn
        spn += 1
        return sp[(spn - 1) % len(sp)]

    for pl in _expand(plants):
        kind = pl[0]
        if kind == "copy":
            i, d, L = pl[1:4]
            near = pl[4] if len(pl) > 4 else 0
            s = rng.integers(128, 256, L).astype(np.uint8)
            q = i - d
            assert q >= 1 and i + L + 1 <= n
            buf[q:q + L] = s
            buf[q + L] = special()
            buf[q - 1] = special()
            buf[i - 4:i] = [special() for _ in range(4)]
            buf[i:i + L] = s
            if i + L < n:
                buf[i + L] = special()
            if near:
                r = i - near
                buf[r:r + 5] = s[:5]
                buf[r + 5] = special()
                buf[r - 1] = special()
        elif kind == "copy0":
            _, i, L = pl
            buf[i - 2:i] = [special(), special()]
            buf[i:i + L] = buf[:L].copy()
            buf[i + L] = special()
        elif kind == "head0":
            buf[:pl[1]] = rng.integers(128, 256, pl[1]).astype(np.uint8)
        elif kind == "kplant":
            _, P, ordn, period = pl
            buf[P - 1] = special()
            Q = P - period * (ordn + 2)
            assert Q >= period
            buf[Q:Q + 40] = buf[P:P + 40].copy()
        elif kind == "run":
            _, a, L, byte = pl
            buf[a:a + L] = byte
        elif kind == "fresh":
            _, a, L = pl
            seen = set(LM.hashes(buf[:a].tobytes()).tolist()) if a >= 3 else set()
            hat = lambda x: ((int(buf[x]) << 10) ^ (int(buf[x + 1]) << 5) ^ int(buf[x + 2])) & 0x7fff  # noqa: E731
            for x in range(a, a + L):
                # (the last byte also decides the two trigrams that run on into the bytes behind the stretch)
                ps = (x - 2, x - 1, x) if x == a + L - 1 and x + 2 < n else (x - 2,)
                for _ in range(256):
                    buf[x] = int(rng.integers(128, 256))
                    hs = [hat(p) for p in ps]
                    if len(set(hs)) == len(hs) and not seen & set(hs):
                        break
                else:
                    raise AssertionError(("fresh", a, x))
                seen |= set(hs)
        elif kind == "byte":
            buf[pl[1]] = pl[2]
        elif kind == "rand":
            _, a, L = pl
            buf[a:a + L] = rng.integers(1, 256, L).astype(np.uint8)
        elif kind == "end":
            _, L, d = pl
            buf[n - L:] = buf[n - L - d:n - d].copy()
        else:
            raise KeyError(kind)
    out = buf.tobytes()
    assert 0 not in out
    return out


def make_nul(parts, zeros):
    """The NUL group: the parts, with an earlier zero run and the last `zeros` bytes zero (zlib's compare runs past
    the end of the input into zeros; nice is clipped to the bytes left)."""
    buf = np.concatenate([_part(p) for p in parts])
    n = len(buf)
    a = n // 3
    buf[a:a + 2 * zeros + 7] = 0
    buf[n - zeros:] = 0
    return buf.tobytes()


# ---- classification ----------------------------------------------------------------------------------------
DIST_RULES = ("maxdist_first_lt", "maxdist_first_32507", "maxdist_later_le", "maxdist_later_32505")
FRONT_RULES = ("too_far_ge", "too_far_4097", "good_off", "good_33", "cap4096_off", "chain_nocap", "tie_far", "nil_ok",
               "lazy_ge", "max_lazy_off")
BASE_RULES = ("stored_any", "slide_early", "slide_late", "slide_nil_off")
KS = (63, 64, 65, 254, 255, 256, 1023, 1024, 4095)
WIN_LENS = (15, 16, 17, 31, 32, 33, 257, 258)
NOSEARCH = ("1", "63", "64", "65", ">=129")
LOOKBACKS = ("1", "63", "64", "65", "255", "256", ">=257")


def variants():
    out = [(f"v:{r}", r, 0) for r in DIST_RULES + FRONT_RULES + BASE_RULES]
    out += [(f"v:first_k={k}", "first_k", k) for k in KS]
    out += [(f"v:skip_k={k}", "skip_k", k) for k in KS]
    return out


def facts_of(value):
    """(the oracle's member by the dp walk, its search records, its token records)."""
    return FV.facts_of(value)


def variant_could_differ(rule, arg, s, n):
    """False only where no search of the true parse meets the altered rule (front_values.variant_could_differ)."""
    from oracle import pyoracle as O
    if rule in DIST_RULES:
        return bool(((s["end"] == O.END_DIST) | (s["win_dist"] >= MAX_DIST - 1)).any())
    if rule == "max_lazy_off":
        return True
    if rule in ("slide_early", "slide_late", "slide_nil_off", "stored_any"):
        return n >= SLIDE_AT - 1
    return FV.variant_could_differ(rule, arg, s)


def _differences(t, t2):
    """Where the altered parse leaves the true one: the position of the first token of every stretch of consecutive
    tokens of log t that log t2 does not hold.  The search that decided it ran at that position or the next; what
    follows in the stretch is only the altered parse finding its way back."""
    key = lambda x: (x["pos"].astype(np.int64) << 25) | (x["len"].astype(np.int64) << 16) | x["dist"]  # noqa: E731
    missing = ~np.isin(key(t), key(t2))
    first = missing & ~np.concatenate([[False], missing[:-1]])
    return t["pos"][first].astype(np.int64)


def lookbacks(value):
    """For every sort chunk but the first: the entries of S before the chunk's first entry that share its hash (0:
    the chunk starts a hash run)."""
    ch = LM.constants()["chunk"]
    h = LM.hashes(value)
    hs = np.sort(h, kind="stable")
    out = []
    for c0 in range(ch, len(hs), ch):
        if hs[c0] != hs[c0 - 1]:
            out.append(0)
        else:
            out.append(int(c0 - np.searchsorted(hs, hs[c0], side="left")))
    return out


def classes_of(value, member, s, t, nul=False, stitched=None):
    """The classes a value falls in (a set of names)."""
    from oracle import pyoracle as O
    n = len(value)
    out = set()
    for name, rule, arg in variants() + ([("v:nice_258", "nice_258", 0)] if nul else []):
        if not variant_could_differ(rule, arg, s, n):
            continue
        if O.compress_variant(rule, arg, value) != member:
            out.add(name)
            _, t2 = O.last_search_log()
            for z in {zone_of(int(p)) for p in _differences(t, t2)}:
                out.add(f"{name}@{z}")
    blocks = O.compress(value, dp=True) and O.last_block_facts()
    types = [b["type"] for b in blocks]
    if len(types) >= 3 and set(types) == {0, 1, 2}:
        out.add("blocks:stored+fixed+dynamic")
    if len(types) >= 2:
        out.add("blocks>=2")
    # the winning lengths of the matches the parse took (16 bytes per step of the device's compare)
    tp, tl = t["pos"].astype(np.int64), t["len"].astype(np.int64)
    for L in WIN_LENS:
        if (tl == L).any():
            out.add(f"winlen={L}")
    if len(tl) and tl[-1] > 0 and tp[-1] + tl[-1] == n:
        out.add("match-to-end")
    if len(tl) >= 2 and tl[-1] == 0 and tl[-2] > 0:
        out.add("last-lit-after-match")
    if len(tl) >= 2 and tl[-1] == 0 and tl[-2] == 0:
        out.add("last-two-lits")
    # NIL met behind a long chain: the count's `cnt--` (253 .. 255 candidates before position 0) and position 0
    # beyond entry 255 (`q != 0` in member), where admitting position 0 would change the member
    nil = s[s["end"] == O.END_NIL]
    if "v:nil_ok" in out:
        for c in (253, 254, 255):
            if (nil["examined"] == c).any():
                out.add(f"nil-behind={c}")
        if (nil["examined"] >= 256).any():
            out.add("nil-behind>=256")
    # the rank kernel's look-back over a sort chunk's first entry
    for lb in lookbacks(value):
        if lb:
            out.add(f"lookback={lb}" if str(lb) in LOOKBACKS else "lookback>=257" if lb >= 257 else "lookback=other")
    out.discard("lookback=other")
    # parse: runs of positions without a search, as the parse enters them (a loop top with no pending match whose HC
    # is 0: the run lasts to the next position with a search, or to the parse's end)
    st = stitched or LM.Stitched(value)
    hc, _ = LM.hc_of(value)
    hcz = np.concatenate([hc == 0, [True, True]])  # (the last two positions have no hash)
    nxt = np.full(n + 1, n, np.int64)              # nxt[p]: the first position >= p with a search, else n
    for p in range(n - 1, -1, -1):
        nxt[p] = p if not hcz[p] else nxt[p + 1]
    ov = LM.constants()["overlap"]
    for j, P in enumerate(st.parses):
        pos, code = P.states["pos"].astype(np.int64), P.states["code"]
        zero = hcz[pos]
        entry = zero & ~np.concatenate([[False], zero[:-1] & (np.diff(pos) == 1)])
        for p, c in zip(pos[entry].tolist(), code[entry].tolist()):
            end = min(int(nxt[p]), P.eo)
            ln = end - p
            tag = str(ln) if str(ln) in NOSEARCH else ">=129" if ln >= 129 else None
            if tag:
                out.add(f"norun={tag}:{'lit' if c == 2 else 'nolit'}")
            if not P.last and p < P.e < end:
                out.add("norun-crosses-e")
            if not P.last and p < P.e + ov and int(nxt[p]) >= P.e + ov:
                out.add("norun-crosses-overlap-end")
            if int(nxt[p]) >= n:
                out.add("norun-ends-value")
        if not P.last:
            tk = P.tokens
            a, b = tk["pos"].astype(np.int64), tk["len"].astype(np.int64)
            if ((b > 0) & (a < P.e) & (a + b > P.e)).any():
                out.add("match-straddles-e")
    # stitch
    for f, clash in zip(st.found, st.clash):
        out.add("stitch=never" if f is None else "stitch=0" if f == 0 else "stitch=1..63" if f < 64 else
                "stitch=64..127" if f < 128 else "stitch>=1024" if f >= 1024 else "stitch=128..1023")
        if clash:
            out.add("stitch-clash")
    out.discard("stitch=128..1023")
    ns = LM.nseg(n)
    if ns == 3 and not st.failed:
        out.add("segs=3")
    if ns >= 5 and not st.failed:
        out.add("segs>=5")
    for k in (2, 3, 4):
        for d in (-1, 0, 1):
            if n == SEG * k + d:
                out.add(f"len=16384x{k}{d:+d}" if d else f"len=16384x{k}")
    if st.failed:
        out.add("fallback")
        for r in DIST_RULES + ("slide_nil_off", "slide_late"):
            if f"v:{r}" in out:
                out.add(f"fallback+v:{r}")
    return out


# ---- the coverage table ------------------------------------------------------------------------------------
def _stored_excess_bound():
    """The most bits by which the fixed trees can exceed the stored form of a block that is still open when its
    start leaves the window: it spans at least MAX_DIST + 1 bytes in at most 16383 symbols.  A literal costs at
    most one bit more than its byte.  A match of L bytes costs at most 8 + 5 + 5 + 13 bits (7 + 5 + 10 for L = 3,
    whose distance is at most 4096; 7 + 5 + 13 for L = 4), so it saves at least 2, 7 and 8 L - 31 bits -- never
    less than 2 L - 4.  With m matches the block holds at most 16383 - m literals, and the matches span at least
    max(MAX_DIST + 1 - literals, 3 m) bytes.  A stored block needs the excess to be positive (it must win by the
    header's bits besides).  Returns the largest excess over every m (negative)."""
    need = MAX_DIST + 1
    best = None
    for m in range(0, 16384):
        lits = 16383 - m
        span = max(need - lits, 3 * m)
        if span > 258 * m:
            continue
        ex = lits - (2 * span - 4 * m)
        best = ex if best is None else max(best, ex)
    return best


def unreachable():
    """{class: the arithmetic that excludes it}."""
    out = {}
    for r in DIST_RULES:
        out[f"v:{r}@seg0"] = f"a search below {SEG} has no candidate at a distance of {MAX_DIST - 1} or more"
    out["v:max_lazy_off"] = ("longest_match returns at most 258 = prev_length, which deflate_slow ignores "
                             "(match_length <= prev_length): a search at prev_length == 258 changes nothing")
    for z in ZONES:
        out[f"v:max_lazy_off@{z}"] = out["v:max_lazy_off"]
    ex = _stored_excess_bound()
    assert ex < 0
    out["v:stored_any"] = (f"a block whose start has left the window spans more than {MAX_DIST} bytes in at most "
                           f"16383 symbols; the fixed trees then undercut the stored form by at least {-ex} bits "
                           "(_stored_excess_bound), so the window base never decides a stored block")
    # edits of the kernels that no value can tell from the code as it stands (mutation check)
    out["edit:ord<C dropped"] = ("search() takes 64 candidates a step and goes on only while all 64 were valid, so "
                                 "`examined` is a multiple of 64 at every step; C is 1024 or 4096, multiples of 64, so "
                                 "`examined >= C` ends the walk before any ordinal reaches C")
    out["edit:pl<258 dropped"] = out["v:max_lazy_off"]
    out["edit:emit base >= made >"] = out["v:stored_any"]
    return out


def required():
    """{class: the least number of values}."""
    need = {}
    for r in DIST_RULES:
        need[f"v:{r}@mid"] = need[f"v:{r}@slid"] = 3
    for r in FRONT_RULES:
        if r != "max_lazy_off":
            need[f"v:{r}@seg0"] = need[f"v:{r}@mid"] = 3
    for k in KS:
        need[f"v:skip_k={k}"] = need[f"v:first_k={k}"] = 3
    # the window base: decided through NIL at the base itself (large_model.base_hides), the only place where it
    # decides a byte (unreachable(): never through a stored block)
    for r in ("slide_early", "slide_late", "slide_nil_off"):
        need[f"v:{r}"] = 3
    for c in ("nil-behind=253", "nil-behind=254", "nil-behind=255", "nil-behind>=256"):
        need[c] = 3
    for L in WIN_LENS:
        need[f"winlen={L}"] = 3
    for c in ("match-to-end", "last-lit-after-match", "last-two-lits", "norun-crosses-e", "norun-crosses-overlap-end",
              "norun-ends-value", "match-straddles-e", "stitch=0", "stitch=1..63", "stitch=64..127", "stitch>=1024",
              "stitch=never", "stitch-clash", "segs=3", "segs>=5", "blocks:stored+fixed+dynamic"):
        need[c] = 3
    for tag in NOSEARCH:
        need[f"norun={tag}:lit"] = need[f"norun={tag}:nolit"] = 3
    for k in (2, 3, 4):
        for d in ("-1", "", "+1"):
            need[f"len=16384x{k}{d}"] = 3
    need["fallback"] = 3
    for lb in LOOKBACKS:
        need[f"lookback={lb}" if lb[0] != ">" else f"lookback{lb}"] = 3
    return {c: n for c, n in need.items() if c not in WANTED}


# Wanted, not required: reported by the model test, never asserted, with the reason (none now)
WANTED = {}


# ---- the kept values ---------------------------------------------------------------------------------------
U = lambda n, seed, k=12: ("u", n, seed, k)  # noqa: E731


def _fv(kind, n, seed, k, rep, maxrep, extra, m):
    return ("fv", kind, n, seed, k, rep, maxrep, extra, m)


def _dist_plants(base):
    """Four plants from position `base` on: the first candidate at MAX_DIST and one beyond, a later candidate one
    below MAX_DIST and at it."""
    return (("copy", base, MAX_DIST, 40), ("copy", base + 1000, MAX_DIST + 1, 40),
            ("copy", base + 2000, MAX_DIST - 1, 40, 300), ("copy", base + 3000, MAX_DIST, 40, 300))


def _kplants(off, span, seed, period=3):
    """One 'kplant' per ordinal of KS inside the colliding part [off, off + span).  The special byte before another
    plant's P takes the position `period` before that P out of the chain, so a plant's copy lies one chain entry
    farther for every other P between it and its own; positions are drawn until no two plants' 40-byte copies (or
    the bytes before a P) overlap."""
    rng = np.random.default_rng([seed, span, 4])
    for _ in range(10000):
        Ps = {k: period * int(rng.integers(k + 24, (span - 48) // period)) for k in KS}
        iv, out = [], []
        for k, P in Ps.items():
            c = 0
            for _ in range(12):
                Q = P - period * (k + 2 + c)
                c2 = sum(1 for P2 in Ps.values() if P2 != P and Q < P2 - period < P)
                if c2 == c:
                    break
                c = c2
            else:
                break
            iv += [(Q - 1, Q + 41), (P - period - 1, P + 41)]
            out.append(("kplant", off + P, k + c, period))
        else:
            iv.sort()
            if iv[0][0] >= period and all(a[1] <= b[0] for a, b in zip(iv, iv[1:])):
                return tuple(out)
    raise AssertionError("no layout")


E = SEG
FV_SEL = (
    ('ck', 16383, 109, 6, 0, 258, 4095, 12747), ('dg', 16383, 46, 2, 0, 258, 3711, 9079),
    ('dg', 16383, 95, 7, 0, 258, 2853, 8488), ('uf', 16383, 139, 6, 2, 258, 4, 0), ('uz', 16383, 55, 12, 1, 258, 3, 0),
    ('ce', 16383, 141, 2, 2, 258, 15, 12933), ('c', 16383, 107, 6, 0, 258, 0, 12786), ('c', 16383, 51, 1, 2, 258, 0, 12758),
    ('d', 16383, 146, 1, 4, 258, 0, 8651), ('dg', 20000, 104, 2, 0, 258, 2399, 8675),
)
TOO_FAR = lambda base: (("copy", base, 4096, 3), ("copy", base + 1000, 4097, 3))  # noqa: E731
# ("fresh", a, L) gives no search to the L + 2 positions a - 2 .. a + L - 1.  Behind a copy that ends at a the parse
# enters the run at a with no literal pending (L positions); "freshlit" (L + 2 positions) puts a byte between the
# copy and the run whose trigram shares its hash with earlier text and its first byte with none, so the search there
# finds nothing and the run is entered with that literal pending
FRESH_LENS = (1, 61, 62, 63, 64, 65, 140)
FRESH = lambda s: tuple(x for k, L in enumerate(FRESH_LENS) for x in (  # noqa: E731
    ("copy", 19000 + 300 * k + s, 2500, 30), ("fresh", 19030 + 300 * k + s, L),
    ("freshlit", 23000 + 300 * k + s, L, 5000)))

# (parts, plants) of every kept value
PARAMS = (
    # distance rules past 16384 ("mid") and past the first and the second slide ("slid")
    [((U(40000, s),), TOO_FAR(20000) + _dist_plants(33000 + 100 * s)) for s in (1, 2, 3)]
    + [((U(70000, s),), TOO_FAR(9000) + _dist_plants(66000 + 100 * s)) for s in (1, 2, 3)]
    + [((U(103000, 1),), _dist_plants(98500)), ((U(82000, 2),), ()), ((U(135000, 1),), _dist_plants(130000))]
    # the window base as NIL: the candidate at MAX_DIST from loop top 65274 (98042) near the value's end, and from
    # the loop top before it
    + [((U(n, 4),), (("copy", t, MAX_DIST, 40),))
       for n, t in ((65400, SLIDE_AT), (65535, SLIDE_AT), (65320, SLIDE_AT), (98200, SLIDE_AT + W_SIZE),
                    (65400, SLIDE_AT - 1), (65500, SLIDE_AT - 1), (65320, SLIDE_AT - 1), (98200, SLIDE_AT + W_SIZE - 1))]
    # stitch failures on purpose: a period-1 run over the first boundary and the whole overlap behind it
    + [((U(40000, 1),), _dist_plants(33100) + (("run", E - 400, 2500, 0x61),)),
       ((U(70000, 1),), _dist_plants(66100) + (("run", E - 400, 2500, 0x62),)),
       ((U(65400, 4),), (("copy", SLIDE_AT, MAX_DIST, 40), ("run", E - 400, 2500, 0x63))),
       ((U(65535, 4),), (("copy", SLIDE_AT, MAX_DIST, 40), ("run", 2 * E - 399, 2500, 0x64)))]
    # lengths around multiples of the segment
    + [((U(E * k + d, 10 * k + d),), ()) for k in (2, 3, 4) for d in (-1, 0, 1)]
    + [((U(n, s),), ()) for n, s in ((2 * E - 1, 91), (2 * E, 92), (2 * E + 1, 93), (3 * E - 1, 94), (3 * E - 1, 95),
                                     (3 * E + 1, 96), (4 * E, 97), (4 * E, 98), (4 * E + 1, 99), (4 * E + 1, 100))]
    # hash runs across a sort chunk.  Exactly 63, 64 and 65 entries before the first entries of chunks 1, 2, 3:
    # four period-1 runs whose hashes lie below most of the text's, their lengths solved so that the runs of the
    # bytes 128, 129 and 130 begin at 4096 - 63, 8192 - 64 and 12288 - 65 of the sorted array
    + [((U(n, s),), (("run", 1000, a, 1), ("run", 6000, b, 128), ("run", 17400, c, 129), ("run", 23000, 200, 130)))
       for n, s, a, b, c in ((2 * E - 1, 81, 4027, 1794, 1846), (2 * E, 87, 4028, 1812, 1896),
                             (2 * E + 1, 88, 4029, 1814, 1915))]
    # ... 255 and 256 entries: a four-byte alphabet (hash runs of some 750 entries), seeds found by search
    + [((U(n, s, 4),), ()) for n, s in ((3 * E + 1, 4472), (3 * E, 4639), (3 * E, 5143))]
    # a stored, a dynamic and a fixed block in one member
    # (the text's length leaves three symbols to the third block)
    + [((("r", 17000, s), ("ut", n, s, 12, 60000)), ()) for s, n in ((1, 50680), (2, 50280), (3, 50481))]
    # the front's rules, decided in a first segment and past it
    + [((_fv(*p), U(16500, 5)), ()) for p in FV_SEL]
    + [((U(16500, 6), _fv(*p)), ()) for p in FV_SEL]
    + [((U(40000, 7 + s),), (("head0", 40), ("copy0", 20000 + 1000 * s, 40))) for s in (0, 1, 2)]
    # NIL behind a long chain: position 0 heads a run of which 253 .. 255, and more, lie before the search
    + [((_fv("c", 2400, 20 + s, 7, 0, 258, 0, 0), U(31000, 20 + s)),
        (("copy0", 3 * (c + 2), 40), ("copy0", 3 * 400, 40))) for c in (253, 254, 255) for s in (0, 1, 2)]
    # candidate ordinals around one step of search(), the HC cap and the chain caps
    + [((_fv("c", 15000, 30 + s, 7, 0, 258, 0, 0), U(18500, 30 + s)), _kplants(0, 15000, s)) for s in (0, 1, 2)]
    + [((U(16500, 33 + s), _fv("c", 15000, 33 + s, 7, 0, 258, 0, 0), U(2000, 33 + s)), _kplants(16500, 15000, 3 + s))
       for s in (0, 1, 2)]
    # winning lengths around the compare's 16-byte step, and a match to the value's end
    + [((U(36000, 40 + s),), tuple(("copy", 20000 + 600 * k + 7 * s, 1000, L) for k, L in enumerate(WIN_LENS))
        + (("end", 50, 5000),)) for s in (0, 1, 2)]
    # runs of positions without a search
    + [((U(36000, 50 + s),), (("copy", E - 100, 1000, 200), ("fresh", E + 200 - s, 70), ("fresh", E + 2048 - 32 - s, 70))
        + FRESH(s) + (("fresh", 36000 - 70, 70),))
       for s in (0, 1, 2)]
    # stitch: a match that ends on the boundary (offset 0), short and long runs over a boundary
    + [((U(70000, 60 + s),), (("copy", E - 40, 1000, 40), ("run", 2 * E - 100, 170 + s, 0x62),
                             ("run", 3 * E - 300, 1400 + s, 0x63))) for s in (0, 1, 2)]
)

# make_nul()'s arguments: (parts, zeros)
NUL_PARAMS = [((U(40000, 70),), 64), ((U(45000, 74, 3),), 64), ((U(66000, 75, 4),), 300)]


@functools.lru_cache(maxsize=None)
def values():
    """The NUL-free corpus, in PARAMS order."""
    out = [make(parts, plants, k) for k, (parts, plants) in enumerate(PARAMS)]
    assert len(set(out)) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def nul_values():
    out = [make_nul(*p) for p in NUL_PARAMS]
    assert len(set(out)) == len(out)
    return out


def sha(b):
    return hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def stitched(i):
    return LM.Stitched(values()[i])


@functools.lru_cache(maxsize=None)
def fallback():
    """Indices of the values the model fails at a boundary: the gated HBM kernel redoes exactly these."""
    return tuple(i for i in range(len(PARAMS)) if stitched(i).failed)


# ---- GPU batches -------------------------------------------------------------------------------------------
def small_values():
    """Small values for the mixed batch (the split pipeline's, beside the large ones)."""
    return [v for v in FV.values() if len(v) <= 4096][:40]


@functools.lru_cache(maxsize=None)
def ends_in_match():
    """{index: the bytes that follow the source of the value's last match}, for the values whose parse ends in a
    match: laid directly behind the value they would lengthen that match, were the compare not capped at the end."""
    out = {}
    for i, v in enumerate(values()):
        _, _, t = facts_of(v)
        if t["len"][-1] > 0 and int(t["pos"][-1]) + int(t["len"][-1]) == len(v):
            at = len(v) - int(t["dist"][-1])
            out[i] = v[at:at + 8]
    return out


def batch(name):
    """A GPU batch as a list of items: an int is an index into values(), bytes are a small value of the batch's own.
      "lv"            every value once
      "lv-stitched"   every value but those of fallback()
      "lv-unaligned"  for pack(align=1): a first value of 1, 2 or 3 bytes (name "lv-unaligned-1" ..), then every
                      value, each that ends in a match followed directly by the bytes that would lengthen that match
      "lv-mixed"      the values shuffled among small ones, three of them twice"""
    n = len(PARAMS)
    if name == "lv":
        return list(range(n))
    if name == "lv-stitched":
        return [i for i in range(n) if i not in fallback()]
    if name.startswith("lv-unaligned-"):
        first = int(name[-1])
        out = [bytes(range(100, 100 + first))]
        tail = ends_in_match()
        for i in range(n):
            out.append(i)
            if i in tail:
                out.append(tail[i])
        return out
    if name == "lv-mixed":
        items = list(range(n)) + [0, 9, n - 1] + small_values()
        order = np.random.default_rng(n).permutation(len(items))
        return [items[k] for k in order]
    raise KeyError(name)


def batch_values(items):
    vs = values()
    return [vs[x] if isinstance(x, int) else x for x in items]


class LargeConfGolden:
    """tests/golden/large_conf_golden.json (tests/golden/make_large_conf_golden.py): the reference's member of every
    value (libz's for the NUL group), as SHA-256 + length, keyed by the value's SHA-256."""

    def __init__(self):
        with open(os.path.join(GOLDEN, "large_conf_golden.json")) as f:
            self.vectors = json.load(f)["vectors"]

    def mismatches(self, vals, members):
        bad = []
        for k, (v, m) in enumerate(zip(vals, members)):
            want = self.vectors.get(sha(v))
            if want is None or len(m) != want["gz_len"] or sha(m) != want["gz_sha256"]:
                bad.append(k)
        return bad


# The values the model fails at a boundary (tests/test_large_model.py holds fallback() to this list): the list
# tests/test_gpu_large_conf.py counts the retry counter by.
FALLBACK = (17, 18, 19, 20)
# PMC_LV_ROUND_MB of the rounds child: a few values' cost, so that the "lv" batch takes several rounds
ROUND_MB = 8
# ... and of the fast-all rounds child, on the values of tests/test_gpu_fast_large.py (4 bytes of scratch per byte)
FAST_ROUND_MB = 1

"""Inputs of the back conformance tests (test infrastructure): a corpus in which every emission arm decides a byte.

The back (csrc/pmc_deflate_small.hip: run_back, emit_planned, emit_symbols, codes_from_lengths_all,
send_runs_fused, run_bits, or_bits_lds, wave_crc32_s8) turns tokens, a block plan and code lengths into a member's
bits.  It restates zlib's gen_codes, send_tree, compress_block and crc32 and the length and distance code tables in
closed forms and wave-wide scans, so it can be wrong for one code, one run shape or one bit offset alone.  The values
here were picked by search: candidates of make() were classified by dissect() -- the bit position and width of
every token, the tree header's runs -- run over the oracle's member, and a small covering set of the classes of
required() was kept.  Only the parameters that regenerate the kept values are held here (PARAMS); the coverage they
give is asserted by tests/test_back_model.py, not assumed.

Every value is NUL-free, 1 to 16382 bytes and one deflate block.  A value's side is "S" if its length is at most
kHdrMinLen (the back's own send_runs_fused writes its tree header), else "L" (the trees kernel's emit_header does).

big(): values of 33 to 70 KB for the large-value route (deflate_lv_emit_kernel), whose table-driven token_bits is
the only place distance codes 28 and 29 can occur.

Shared by tests/test_back_model.py (CPU), tests/test_gpu_back.py and tests/golden/make_back_golden.py.
"""
import functools
import hashlib
import json
import os
import re

import numpy as np

import deflate_dissect as DD
import trees_values as TV

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MAX_LEN = TV.MAX_LEN
ONE_K = 1024
SIDES = ("S", "L")


@functools.lru_cache(maxsize=None)
def constants():
    """(kHdrMinLen, kNostageMaxLen) of this build, read from csrc/pmc_kernels.hpp."""
    text = open(os.path.join(os.path.dirname(HERE), "poor-man-s-cache_amd", "csrc", "pmc_kernels.hpp")).read()
    return (int(re.search(r"kHdrMinLen = (\d+)", text).group(1)),
            int(re.search(r"kNostageMaxLen = (\d+)", text).group(1)))


def side_of(n):
    return "S" if n <= constants()[0] else "L"


# ---- the dissector -----------------------------------------------------------------------------------------
def _table(lens):
    """(table, bits): table[the next `bits` bits of the stream, first bit lowest] = symbol << 4 | code length."""
    bits = max(max(lens), 1)
    tab = np.full(1 << bits, -1, np.int64)
    bl = [0] * 17
    for x in lens:
        bl[x] += 1
    bl[0] = 0
    code, nxt = 0, [0] * 17
    for L in range(1, 16):
        code = (code + bl[L - 1]) << 1
        nxt[L] = code
    for s, L in enumerate(lens):
        if L:
            c = nxt[L]
            nxt[L] += 1
            r = int(format(c, f"0{L}b")[::-1], 2)
            tab[r::1 << L] = s << 4 | L
    return tab.tolist(), bits


def _runs(lens):
    """The maximal runs of equal code lengths of one tree, as scan_tree walks it: [(first symbol, length, count)]."""
    out = []
    for s, x in enumerate(lens):
        if out and out[-1][1] == x:
            out[-1][2] += 1
        else:
            out.append([s, x, 1])
    return [tuple(r) for r in out]


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 30
LIT = -1  # lcode of a literal token


def dissect(gz):
    """deflate_dissect.dissect's walk with bit positions.  One dict per block: type, last, start_bit (of the 3-bit
    block header, counted from the member's first byte: the back's image holds the 10-byte gzip header too), and
      stored: stored_len;
      fixed and dynamic: ll, dl, end_bit (past the end-of-block code), tokens -- a list of
        (start bit, width, length code or LIT, length extra value or the literal, distance code, distance extra value);
      dynamic: hlit, hdist, hclen, cl, hdr_bits (the tree header's bits after the 3-bit block header), runs_ll and
        runs_d ([(first symbol, code length, count)])."""
    d = bytes(gz) + bytes(16)
    frm = int.from_bytes
    p = 80
    blocks = []

    def get(n):
        nonlocal p
        v = (frm(d[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)
        p += n
        return v

    while True:
        start = p
        last, typ = get(1), get(2)
        blk = {"type": typ, "last": last, "start_bit": start}
        if typ == 0:
            p = (p + 7) & ~7
            n = get(16)
            get(16)
            p += 8 * n
            blk["stored_len"] = n
        else:
            if typ == 1:
                ll, dl = FIXED_LL, FIXED_DL
            else:
                assert typ == 2, typ
                hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[DD.ORDER[k]] = get(3)
                ct, cb = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    e = ct[(frm(d[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << cb) - 1)]
                    assert e >= 0
                    p += e & 15
                    s = e >> 4
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + get(2))
                    elif s == 17:
                        lens += [0] * (3 + get(3))
                    else:
                        lens += [0] * (11 + get(7))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, hdr_bits=p - start - 3, runs_ll=_runs(ll),
                           runs_d=_runs(dl))
            blk["ll"], blk["dl"] = ll, dl
            lt, lb = _table(ll)
            dt, db = _table(dl)
            lm, dm = (1 << lb) - 1, (1 << db) - 1
            toks = []
            LE, DE = DD.LEXT, DD.DEXT
            while True:
                t0 = p
                w = frm(d[p >> 3:(p >> 3) + 8], "little") >> (p & 7)
                e = lt[w & lm]
                assert e >= 0, "bad code"
                s, n = e >> 4, e & 15
                if s < 256:
                    toks.append((t0, n, LIT, s, 0, 0))
                    p += n
                    continue
                if s == 256:
                    p += n
                    break
                c = s - 257
                xl = LE[c]
                lx = (w >> n) & ((1 << xl) - 1)
                n += xl
                e = dt[(w >> n) & dm]
                assert e >= 0, "bad distance code"
                dc = e >> 4
                n += e & 15
                xd = DE[dc]
                dx = (w >> n) & ((1 << xd) - 1)
                n += xd
                toks.append((t0, n, c, lx, dc, dx))
                p += n
            blk["tokens"] = toks
            blk["end_bit"] = p
        blocks.append(blk)
        if last:
            break
    return blocks


def plain(blocks):
    """dissect()'s blocks as deflate_dissect.dissect gives them (tokens as literals and (length, distance))."""
    out = []
    for b in blocks:
        o = {k: v for k, v in b.items() if k in ("type", "last", "stored_len", "hlit", "hdist", "hclen", "cl", "ll", "dl")}
        if "tokens" in b:
            o["tokens"] = [t[3] if t[2] == LIT else (DD.LBASE[t[2]] + t[3], DD.DBASE[t[4]] + t[5]) for t in b["tokens"]]
        out.append(o)
    return out


# ---- the generator -----------------------------------------------------------------------------------------
# the lengths of the runs of the 'r' background: the top of the length codes 20 to 27 and 258, plus the run's first
# byte (a literal)
_RUN_LENS = (83, 99, 115, 131, 163, 195, 227, 258, 259)


def make(kind, k, n, seed, start=-1, ratio=0.9, rep=0, maxrep=258, exact=False, plants=(), far=0):
    """n bytes: a background with planted copies.
    kind 'u', 'g', 'f': the background is trees_values.make(kind, k, n, seed, start, ratio, rep, maxrep, exact).
    kind 'r': runs of one byte each, of the lengths _RUN_LENS in turn from run number `seed` on; the bytes go
    through start, start + 1 .. 255, 1 .. -- few tokens, every one rare: a long value whose block is fixed.
    kind 'c': k distinct bytes from `start` on, then slices of what stands so far, of rep .. maxrep bytes each, appended
    back to back -- few tokens at many lengths and distances, no symbol frequent: a long value whose block is fixed.
    plants: (length, dist) pairs.  Each is a string of bytes the background does not use, written once and copied
    once `dist` bytes later, between bytes that differ, so that the parse holds one match of exactly that length
    at exactly that distance; dist <= length: the string is dist bytes and is followed by length more bytes of its
    own period.  The places are drawn (seeded) so that no two plants touch.
    far >= 4: the value's first `far` bytes are such a string too and its last `far` bytes their copy (the farthest
    distance the value admits: n - far)."""
    rng = np.random.default_rng([seed, k, n, len(plants), far])
    if kind == "r":
        buf = np.empty(n, np.uint8)
        at, j, byte = 0, seed, max(start, 1)
        while at < n:
            ln = _RUN_LENS[j % len(_RUN_LENS)]
            buf[at:at + ln] = byte
            at, j, byte = at + ln, j + 1, byte % 255 + 1
        spare = np.arange(1, 256, dtype=np.uint8)
    elif kind == "c":
        assert start >= 1 and start + k <= 256 and 3 <= rep <= maxrep <= 258
        seq = list(range(start, start + k))
        while len(seq) < n:
            ln = int(rng.integers(rep, min(maxrep, len(seq)) + 1)) if len(seq) >= rep else len(seq)
            a = int(rng.integers(0, len(seq) - ln + 1))
            seq += seq[a:a + ln]
        buf = np.array(seq[:n], np.uint8)
        spare = np.setdiff1d(np.arange(1, 256, dtype=np.uint8), buf)
    else:
        buf = np.frombuffer(TV.make(kind, k, n, seed, start, ratio, rep, maxrep, exact), np.uint8).copy()
        spare = np.setdiff1d(np.arange(1, 256, dtype=np.uint8), buf)
        assert len(spare) >= 16, "no bytes left for the planted strings"
    taken = []

    def free(a, b):
        return a >= 0 and b <= n and all(b <= x or a >= y for x, y in taken)

    def fresh(m):
        s = rng.choice(spare, m + 4)
        for i in range(1, m + 4):  # (no byte twice in a row: a planted string holds no run of its own)
            while s[i] == s[i - 1]:
                s[i] = rng.choice(spare)
        return s

    if far:
        assert far >= 4 and n >= 2 * far + 4
        s = fresh(far)
        buf[:far], buf[far] = s[:far], s[far]
        buf[n - far - 1], buf[n - far:] = s[far + 1], s[:far]
        taken += [(0, far + 1), (n - far - 1, n)]
    for ln, dist in plants:
        assert 3 <= ln <= 258 and 1 <= dist and dist + ln + 2 <= n, (ln, dist, n)
        for _ in range(400):
            p = int(rng.integers(1, n - dist - ln))
            if dist <= ln:
                spans = [(p - 1, p + dist + ln + 1)]
            else:
                spans = [(p - 1, p + ln + 1), (p + dist - 1, p + dist + ln + 1)]
                if spans[0][1] > spans[1][0]:
                    spans = [(p - 1, p + dist + ln + 1)]
            if all(free(a, b) for a, b in spans):
                break
        else:
            raise AssertionError(("no room for plant", ln, dist, n))
        taken += spans
        s = fresh(ln)
        if dist <= ln:
            per = s[:dist]
            buf[p - 1] = s[-1]
            buf[p:p + dist + ln] = np.resize(per, dist + ln)
            buf[p + dist + ln] = s[-2]
        else:
            buf[p - 1], buf[p + dist + ln] = s[-1], s[-2]
            buf[p + ln], buf[p + dist - 1] = s[-3], s[-4]   # (dist == ln + 1: one byte, the later write holds)
            buf[p:p + ln] = s[:ln]
            buf[p + dist:p + dist + ln] = s[:ln]
    out = buf.tobytes()
    assert len(out) == n and 0 not in out
    return out


# ---- classification ----------------------------------------------------------------------------------------
ZERO_RUNS = (1, 2, 3, 10, 11, 138, 139)    # both sides of run_bits' zero-run arms; ">=277": two full 138s and more
ZERO_RUNS_LL = (141, 149)                  # after one full 138: a remainder of 3 (code 17) and of 11 (code 18)
NONZERO_RUNS = (1, 2, 3, 4, 6, 7, 8)       # ... and of its repeat arms; ">=13": 7 and at least one full 6
NTOK_MOD = (0, 1, 63)
HDR_MOD = (0, 1, 31)
TOP_LEXT = [(1 << x) - 1 for x in DD.LEXT]
TOP_LEXT[27] = 30                          # length 258 is code 28: code 27 ends at 227 + 30
WIDE = {"S": 24, "L": 40}                  # "widest token": at least this many bits (see required())
LEN_BANDS = (("<=512", 1, 512), ("513..1024", 513, 1024), (">1024", 1025, MAX_LEN))


def band_of(n):
    return next(name for name, lo, hi in LEN_BANDS if lo <= n <= hi)


def classes_of(value, member=None, f=None):
    """The classes of the coverage table a value falls in (a set of names), from the oracle's member and block
    facts alone.  Token, header-run and block-type classes carry the value's side; code and CRC classes do not."""
    if member is None:
        member, f = TV.facts_of(value)
    n = len(value)
    sd = side_of(n)
    (blk,) = dissect(member)
    assert blk["type"] == f["type"] and blk["last"] == 1
    out = {f"{sd}:type={('stored', 'fixed', 'dynamic')[blk['type']]}"}
    # CRC and trailer: by the length alone
    out.add(f"crc:{band_of(n)}:mod16={n % 16}")
    if n <= 15 or n in (1024, 1025, MAX_LEN):
        out.add(f"crc:len={n}")
    out.add(f"trailer:size%4={len(member) % 4}")
    if blk["type"] == 0:
        return out
    toks = blk["tokens"]
    assert len(toks) == f["symbols"]  # (ntok of run_back: the end-of-block code is not a token)
    nt = len(toks)
    if nt in (1, 2):
        out.add(f"{sd}:ntok={nt}")
    if nt % 64 in NTOK_MOD:
        out.add(f"{sd}:ntok%64={nt % 64}")
    fixed = blk["type"] == 1
    widest = 0
    for t0, w, lc, lx, dc, dx in toks:
        if t0 & 31 == 0:
            out.add(f"{sd}:tok-start@0")
        if (t0 + w) & 31 == 0:
            out.add(f"{sd}:tok-end@31")
        if lc == LIT:
            if fixed and lx >= 144:
                out.add(f"{sd}:fixed:lit>=144")
            continue
        widest = max(widest, w)
        if (t0 & 31) + w > 64:
            out.add(f"{sd}:tok-3words")
        if lx == 0:
            out.add(f"{sd}:lcode={lc}:base")
        if lx == TOP_LEXT[lc]:
            out.add(f"{sd}:lcode={lc}:top")
        if dx == 0:
            out.add(f"{sd}:dcode={dc}:base")
        if dx == (1 << DD.DEXT[dc]) - 1:
            out.add(f"{sd}:dcode={dc}:top")
        if fixed and lc >= 23:
            out.add(f"{sd}:fixed:lcode>=23")
        if fixed and DD.DEXT[dc] == 12:
            out.add(f"{sd}:fixed:dext=12")
    if widest >= WIDE[sd]:
        out.add(f"{sd}:tok-width>={WIDE[sd]}")
    if fixed:
        return out
    # codes
    ll, dl, cl = blk["ll"], blk["dl"], blk["cl"]
    for x in set(ll) - {0}:
        out.add(f"code:ll-len={x}")
    for x in set(dl) - {0}:
        out.add(f"code:d-len={x}")
    for base, lens in ((0, ll), (286, dl), (316, cl)):  # (the 286 + 30 + 19 row codes_from_lengths_all walks)
        for x in set(lens) - {0}:
            at = [base + s for s, y in enumerate(lens) if y == x]
            if len(at) >= 65:
                out.add("code:group>=65")
            if len({a // 64 for a in at}) >= 3:
                out.add("code:group-in-3-chunks")
    if 7 in cl:
        out.add("code:bl-len=7")
    if not any(t[2] != LIT for t in toks):
        assert blk["hdist"] == 2 and dl == [1, 1]  # (build_tree forces two codes: the HDIST field is 1)
        out.add("code:nomatch,HDIST=1")
    # tree header runs
    mod = blk["hdr_bits"] % 32
    if mod in HDR_MOD:
        out.add(f"{sd}:hdr-bits%32={mod}")
    for tree, runs in (("ll", blk["runs_ll"]), ("d", blk["runs_d"])):
        pre = f"{sd}:{tree}:"
        last_sym = runs[-1][0] + runs[-1][2] - 1
        for s, x, cnt in runs:
            e = s + cnt - 1
            if x == 0:
                if cnt in ZERO_RUNS or (tree == "ll" and cnt in ZERO_RUNS_LL):
                    out.add(pre + f"zrun={cnt}")
                if cnt >= 277:
                    out.add(pre + "zrun>=277")
            else:
                if cnt in NONZERO_RUNS:
                    out.add(pre + f"run={cnt}")
                if cnt >= 13:
                    out.add(pre + "run>=13")
            if e // 64 == s // 64 + 1:
                out.add(pre + "run-into-next-chunk")
            if any(e >= 64 * c + 63 for c in range(s // 64 + 1, last_sym // 64)):
                # chunk c, neither the first nor the last walked, holds no run start: sm[c] == 0
                out.add(pre + "run-over-whole-chunk")
            if s % 64 == 63:
                out.add(pre + "run-starts@lane63")
            if s % 64 == 0 and s > 0:
                out.add(pre + "run-starts@lane0")
            if e == last_sym and s // 64 < e // 64:
                # the last chunk walked holds no run start (sm[nch - 1] == 0): the run's end is max_code + 1 itself
                out.add(pre + "last-run-from-earlier-chunk")
    return out


# ---- the coverage table ------------------------------------------------------------------------------------
def unreached():
    """{class: why no value meets it}: arithmetic where it excludes the class, else what the search tried."""
    hdr = constants()[0]
    un = {}
    # a match of distance D and length >= 3 needs D + 3 <= len
    for dc in range(30):
        for edge, d in (("base", DD.DBASE[dc]), ("top", DD.DBASE[dc] + (1 << DD.DEXT[dc]) - 1)):
            for sd, most in (("S", hdr), ("L", MAX_LEN)):
                if d + 3 > most:
                    un[f"{sd}:dcode={dc}:{edge}"] = f"distance {d} + 3 > {most}, the side's longest value"
    un["S:fixed:dext=12"] = f"12 extra bits start at distance 4097 > {hdr}"
    un["S:tok-3words"] = ("needs a token of at least 34 bits; within 512 bytes a distance has at most 7 extra bits and "
                          "the search found no token above 24 bits")
    for nt in (1, 2):
        un[f"L:ntok={nt}"] = (f"the first token is a literal and every other covers at most 258 bytes: "
                              f"ntok >= 1 + ceil({hdr} / 258) = 3")
    for sd in SIDES:
        un[f"{sd}:ll:zrun>=277"] = ("the end-of-block code 256 is always in use and so is a literal below it: no zero run "
                                    "above 255 (nor above 29 past 256)")
        for x in ("zrun=138", "zrun=139", "zrun>=277", "run-into-next-chunk", "run-over-whole-chunk", "run-starts@lane63",
                  "run-starts@lane0", "last-run-from-earlier-chunk"):
            un[f"{sd}:d:{x}"] = "the distance tree has 30 codes: one chunk, no zero run above 29"
        un[f"{sd}:d:run>=13"] = ("13 distance codes in a row of one length: the search's planted copies never gave "
                                 "more than 8 equal neighbours")
    un["code:ll-len=15"] = ("a 15-bit code needs Fibonacci-like counts over 16 or more symbols; matches flatten them: "
                            "'f' alphabets of 16 to 30 symbols at 16382 bytes, exact counts, gave 14 at most")
    for x in (13, 14, 15):
        un[f"code:d-len={x}"] = "planted copies at Fibonacci-like counts per distance code gave 12 at most"
    return un


def required():
    """{class: the least number of values}.  Classes of unreached() are left out (and asserted empty)."""
    need = {}
    for sd in SIDES:
        for lc in range(29):
            need[f"{sd}:lcode={lc}:base"] = 1
            need[f"{sd}:lcode={lc}:top"] = 1
        for dc in range(28):
            need[f"{sd}:dcode={dc}:base"] = 1
            need[f"{sd}:dcode={dc}:top"] = 1
        # "widest token": S -- past the 25 bits a 32-bit shift of a 7-bit offset would still hold; L -- past 35, the
        # widest token of the trees and front corpora, and past 32 + 7
        need[f"{sd}:tok-width>={WIDE[sd]}"] = 1
        for x in ("tok-3words", "tok-start@0", "tok-end@31", "ntok=1", "ntok=2", "fixed:lit>=144", "fixed:lcode>=23",
                  "fixed:dext=12", "type=stored", "type=fixed", "type=dynamic"):
            need[f"{sd}:{x}"] = 1
        for m in NTOK_MOD:
            need[f"{sd}:ntok%64={m}"] = 1
        for m in HDR_MOD:
            need[f"{sd}:hdr-bits%32={m}"] = 1
        for tree in ("ll", "d"):
            for r in ZERO_RUNS:
                need[f"{sd}:{tree}:zrun={r}"] = 1
            for r in NONZERO_RUNS:
                need[f"{sd}:{tree}:run={r}"] = 1
            for x in ("zrun>=277", "run>=13", "run-into-next-chunk", "run-over-whole-chunk", "run-starts@lane63",
                      "run-starts@lane0", "last-run-from-earlier-chunk"):
                need[f"{sd}:{tree}:{x}"] = 1
        for r in ZERO_RUNS_LL:
            need[f"{sd}:ll:zrun={r}"] = 1
    for x in range(1, 16):
        need[f"code:ll-len={x}"] = 1
        need[f"code:d-len={x}"] = 1
    for x in ("group>=65", "group-in-3-chunks", "bl-len=7", "nomatch,HDIST=1"):
        need[f"code:{x}"] = 1
    for name, lo, hi in LEN_BANDS:
        for m in range(16):
            need[f"crc:{name}:mod16={m}"] = 1
    for n in list(range(1, 16)) + [1024, 1025, MAX_LEN]:
        need[f"crc:len={n}"] = 1
    for m in range(4):
        need[f"trailer:size%4={m}"] = 1
    un = unreached()
    return {c: k for c, k in need.items() if c not in un}


# ---- the kept values ---------------------------------------------------------------------------------------
# make()'s arguments of every kept value: (kind, k, n, seed, start, ratio, rep, maxrep, exact, plants, far)
PARAMS = [
    ('u', 1, 1, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 2, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 3, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 4, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 5, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 6, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 7, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 8, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 9, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 10, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 11, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 12, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 13, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 14, 0, -1, 0.9, 0, 258, False, (), 0),
    ('u', 1, 15, 0, -1, 0.9, 0, 258, False, (), 0),
    ('g', 60, 21, 131, 186, 0.85, 0, 12, False, (), 0),
    ('g', 20, 40, 142, 236, 0.7, 0, 258, True, (), 0),
    ('g', 4, 49, 15, 138, 0.7, 0, 12, True, (), 0),
    ('u', 4, 92, 169, 10, 0.85, 1, 12, False, (), 0),
    ('u', 40, 97, 106, 186, 0.5, 0, 258, False, (), 0),
    ('g', 3, 101, 268, 40, 0.97, 3, 12, False, (), 0),
    ('g', 60, 110, 150, 138, 0.7, 0, 12, True, (), 0),
    ('u', 56, 153, 253, 200, 0.9, 10, 258, True, (), 0),
    ('u', 2, 159, 256, -1, 0.9, 0, 258, False, (), 0),
    ('g', 60, 167, 183, 186, 0.7, 3, 258, True, (), 0),
    ('g', 30, 200, 2, 139, 0.9, 2, 258, False, (), 0),
    ('u', 10, 200, 0, 139, 0.9, 2, 258, True, (), 0),
    ('g', 10, 400, 2, 149, 0.9, 2, 258, True, (), 0),
    ('g', 3, 402, 1, -1, 0.9, 0, 258, False, ((131, 193),), 0),
    ('g', 2, 416, 235, 10, 0.85, 1, 12, False, (), 0),
    ('u', 30, 417, 24, -1, 0.9, 0, 258, False, ((258, 16), (5, 33)), 0),
    ('g', 6, 431, 441, -1, 0.9, 0, 258, False, ((12, 64), (50, 32), (30, 24), (10, 2), (15, 6)), 0),
    ('g', 3, 440, 525, -1, 0.9, 0, 258, False, ((257, 12), (9, 13), (5, 6)), 0),
    ('u', 60, 442, 41, -1, 0.9, 0, 258, False, ((4, 7), (4, 9), (5, 13), (4, 17), (6, 25), (5, 33), (6, 49), (4,
        65)), 0),
    ('u', 12, 447, 67, -1, 0.9, 0, 258, False, ((227, 65), (6, 1), (3, 4)), 0),
    ('u', 6, 454, 572, -1, 0.9, 0, 258, False, ((163, 129), (4, 7), (4, 1)), 0),
    ('u', 6, 455, 416, -1, 0.9, 0, 258, False, ((115, 129), (34, 9), (11, 8), (6, 256)), 0),
    ('u', 3, 460, 324, -1, 0.9, 0, 258, False, ((23, 2), (27, 257), (99, 193), (3, 32), (3, 385)), 0),
    ('g', 6, 461, 151, -1, 0.9, 0, 258, False, ((226, 9), (6, 2), (4, 384), (15, 256), (8, 3)), 0),
    ('g', 6, 476, 520, -1, 0.9, 0, 258, False, ((18, 129), (23, 13), (12, 193), (59, 97), (83, 17)), 0),
    ('g', 6, 492, 314, -1, 0.9, 0, 258, False, ((130, 129), (51, 24)), 0),
    ('u', 3, 496, 117, -1, 0.9, 0, 258, False, ((98, 25), (195, 12)), 0),
    ('g', 12, 500, 505, -1, 0.9, 0, 258, False, ((7, 48), (15, 3), (30, 24), (162, 16), (9, 192)), 0),
    ('g', 60, 500, 0, 141, 0.9, 0, 258, True, (), 0),
    ('u', 3, 501, 221, -1, 0.9, 0, 258, False, ((194, 24), (66, 6), (19, 384), (4, 17)), 0),
    ('u', 30, 502, 42, -1, 0.9, 0, 258, False, ((114, 25), (82, 12), (12, 7), (12, 8), (31, 25)), 0),
    ('u', 60, 513, 1, -1, 0.9, 2, 258, False, (), 0),
    ('g', 4, 515, 191, 10, 0.97, 0, 12, True, (), 0),
    ('g', 250, 516, 79, -1, 0.97, 0, 258, True, (), 0),
    ('u', 100, 516, 507, 156, 0.9, 0, 258, True, (), 0),
    ('u', 60, 533, 1, 70, 0.85, 10, 258, True, (), 0),
    ('g', 4, 534, 78, 40, 0.5, 0, 12, False, (), 0),
    ('g', 100, 554, 18, -1, 0.85, 10, 12, True, (), 0),
    ('g', 200, 556, 15, -1, 0.85, 10, 258, True, (), 0),
    ('u', 117, 561, 67, 139, 0.85, 10, 258, True, (), 0),
    ('g', 4, 571, 115, 70, 0.85, 0, 12, False, (), 0),
    ('g', 60, 600, 0, 149, 0.9, 0, 258, True, (), 0),
    ('r', 0, 600, 0, 1, 0.9, 0, 258, False, (), 0),
    ('u', 30, 600, 2, 138, 0.9, 0, 258, False, (), 0),
    ('u', 4, 600, 0, 141, 0.9, 2, 258, False, (), 0),
    ('g', 118, 601, 80, 138, 0.97, 3, 12, False, (), 0),
    ('g', 3, 605, 38, 138, 0.9, 0, 12, True, (), 0),
    ('g', 3, 621, 53, -1, 0.9, 0, 258, False, ((42, 192), (12, 4), (9, 96), (35, 13), (31, 12), (11, 9), (6,
        24), (23, 257), (6, 9), (16, 192)), 0),
    ('u', 6, 639, 19, -1, 0.9, 0, 258, False, ((83, 97), (3, 7), (59, 256), (4, 25), (17, 6), (4, 13), (6, 17),
        (4, 192)), 0),
    ('u', 3, 679, 229, -1, 0.9, 0, 258, False, ((99, 513), (163, 6), (12, 193)), 0),
    ('g', 6, 686, 147, -1, 0.9, 0, 258, False, ((50, 49), (5, 513), (59, 96), (12, 4), (17, 129), (4, 6), (6,
        192), (27, 17), (19, 5), (10, 4)), 0),
    ('g', 6, 754, 36, -1, 0.9, 0, 258, False, ((195, 129), (30, 5), (10, 512), (12, 65), (12, 17)), 0),
    ('g', 100, 781, 249, -1, 0.9, 10, 258, False, (), 0),
    ('u', 3, 841, 360, -1, 0.9, 0, 258, False, ((195, 6), (114, 9), (42, 8), (67, 24), (5, 257), (6, 6)), 0),
    ('u', 8, 896, 65, 139, 0.85, 10, 258, False, (), 0),
    ('g', 12, 1011, 366, -1, 0.9, 0, 258, False, ((82, 5), (131, 1), (98, 1), (58, 65), (9, 128), (6, 64), (14,
        257), (12, 25), (4, 32), (12, 769), (6, 97)), 0),
    ('u', 140, 1024, 39, -1, 0.9, 0, 258, True, (), 0),
    ('u', 4, 1025, 0, -1, 0.9, 2, 258, False, (), 0),
    ('r', 0, 1030, 0, 1, 0.9, 0, 258, False, (), 6),
    ('u', 3, 1032, 223, 186, 0.85, 1, 12, True, (), 0),
    ('g', 2, 1054, 112, -1, 0.5, 1, 12, False, (), 0),
    ('u', 60, 1095, 103, 40, 0.97, 10, 12, True, (), 0),
    ('g', 200, 1146, 98, -1, 0.85, 1, 258, True, (), 0),
    ('u', 140, 1155, 27, -1, 0.9, 0, 258, True, (), 0),
    ('u', 40, 1156, 117, -1, 0.5, 0, 12, True, (), 0),
    ('u', 40, 1179, 26, 200, 0.9, 3, 12, True, (), 0),
    ('u', 56, 1186, 49, 200, 0.97, 10, 258, False, (), 0),
    ('g', 6, 1212, 63, -1, 0.9, 0, 258, False, ((227, 5), (51, 256), (99, 48), (5, 129), (5, 1), (9, 49), (12,
        16), (4, 384), (9, 5), (34, 768), (4, 8), (5, 385)), 0),
    ('u', 117, 1216, 245, 139, 0.97, 0, 12, False, (), 0),
    ('u', 40, 1229, 73, 186, 0.5, 3, 12, False, (), 0),
    ('u', 117, 1247, 120, 139, 0.5, 0, 258, False, (), 0),
    ('u', 12, 1449, 127, -1, 0.9, 0, 258, False, ((115, 5), (43, 193), (66, 512), (35, 128), (99, 193), (5, 9),
        (98, 5), (4, 97), (9, 1025), (9, 25), (4, 24), (5, 65)), 0),
    ('u', 8, 1564, 5, 70, 0.85, 1, 12, True, (), 0),
    ('g', 8, 2842, 76, -1, 0.85, 0, 12, False, (), 0),
    ('c', 12, 8300, 0, 100, 0.9, 3, 258, False, (), 6),
    ('g', 12, 9349, 1, -1, 0.9, 0, 258, False, ((257, 1025), (4, 1536), (257, 1537), (10, 2048), (7, 2049), (10,
        3072), (258, 3073), (7, 4096), (4, 4097), (7, 6144), (257, 6145), (4, 8192), (5, 8193)), 0),
    ('g', 100, 16382, 4, -1, 0.9, 0, 258, False, ((226, 16124),), 0),
    ('g', 120, 16382, 20, -1, 0.95, 0, 258, False, ((257, 13713),), 0),
    ('u', 12, 16382, 1, -1, 0.95, 0, 258, False, ((163, 1025), (4, 1536), (4, 1537), (227, 2048), (4, 2049),
        (195, 3072), (6, 3073), (194, 4096), (227, 4097), (4, 6144), (5, 6145), (5, 8192), (10, 8193), (5,
        12288), (4, 12289)), 0),
]

# make()'s arguments of the values of big()
BIG_PARAMS = [
    ('g', 100, 34000, 7, -1, 0.93, 0, 258, False, ((194, 22663),), 0),
    ('g', 140, 36000, 0, -1, 0.95, 0, 258, False, ((226, 24013),), 0),
]


@functools.lru_cache(maxsize=None)
def values():
    """The corpus, in PARAMS order."""
    out = [make(*p) for p in PARAMS]
    assert len(set(out)) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def big():
    """The values added for the large-value route (33 to 70 KB)."""
    return [make(*p) for p in BIG_PARAMS]


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ---- the large-value route ---------------------------------------------------------------------------------
# deflate_lv_emit_kernel (csrc/pmc_deflate_large.hip) emits through a table-driven token_bits and a lane-0
# send_all_trees of its own; what only it can meet:
LARGE_CLASSES = ([f"lv:dcode={dc}:{edge}" for dc in (26, 27, 28, 29) for edge in ("base", "top")] +
                 ["lv:tok-3words:block>0"] + [f"lv:block>0-start%8={k}" for k in range(8)])
LARGE_UNREACHED = {"lv:dcode=29:top": "distance 32768 > 32768 - 262 = 32506, the farthest match zlib's window admits"}


def large_classes_of(member):
    """The classes of LARGE_CLASSES a member meets."""
    out = set()
    for k, b in enumerate(dissect(member)):
        if k:
            out.add(f"lv:block>0-start%8={b['start_bit'] % 8}")
        for t0, w, lc, lx, dc, dx in b.get("tokens", ()):
            if lc == LIT:
                continue
            if dc >= 26 and dx == 0:
                out.add(f"lv:dcode={dc}:base")
            if dc >= 26 and dx == (1 << DD.DEXT[dc]) - 1:
                out.add(f"lv:dcode={dc}:top")
            if k and (t0 & 31) + w > 64:
                out.add("lv:tok-3words:block>0")
    return out


# Where tests/large_values.py's sets meet them: {class: (set, index of the shortest value that does)}, found by
# running large_classes_of over every value of every set; tests/test_back_model.py holds each witness to its class.
# The one class no set meets is met by big().
LARGE_WITNESS = {
    "lv:dcode=26:base": ("segment_boundaries_json", 5),   # 8 values, this one 49153 B
    "lv:dcode=26:top": ("binary_and_stored", 6),          # 3 values, 140000 B
    "lv:dcode=27:base": ("binary_and_stored", 6),         # 2 values, 140000 B
    "lv:dcode=27:top": ("multi_megabyte", 1),             # 1 value, 2 MiB
    "lv:dcode=28:base": ("binary_and_stored", 3),         # 3 values, 70001 B
    "lv:dcode=28:top": ("multi_megabyte", 1),             # 1 value, 2 MiB
    "lv:dcode=29:base": ("binary_and_stored", 9),         # 3 values, 300007 B
    "lv:block>0-start%8=0": ("block_edges", 34),          # 22 values, 16392 B
    "lv:block>0-start%8=1": ("block_edges", 14),          # 13 values, 16867 B
    "lv:block>0-start%8=2": ("block_edges", 9),           # 11 values, 33876 B
    "lv:block>0-start%8=3": ("binary_and_stored", 2),     # 9 values, 40000 B
    "lv:block>0-start%8=4": ("block_edges", 15),          # 13 values, 33917 B
    "lv:block>0-start%8=5": ("block_edges", 20),          # 13 values, 16889 B
    "lv:block>0-start%8=6": ("binary_and_stored", 8),     # 7 values, 140000 B
    "lv:block>0-start%8=7": ("block_edges", 8),           # 20 values, 16885 B
}
LARGE_MISSING = ("lv:tok-3words:block>0",)                # no set meets it: every value of big() does


N_SPLIT = 4224   # above the one-kernel path's 1024-value limit; from 4096 a chunk's lanes visit it in cO order
LONG = 4096      # the "16k" row cycles the values up to this length and sends the longer ones once


def batch(name):
    """The values of a GPU batch, as indices into values().
    "512": the side-S values, shuffled (seeded) and cycled to N_SPLIT: a pass whose cap is at most kNostageMaxLen.
    "1k": the values of at most 1024 bytes, likewise.
    "16k": every value: those above LONG bytes once, the others cycled, N_SPLIT in all, shuffled.
    "mono": every value of at most 4096 bytes, once (at most 1024 values: the one-kernel device path).
    "all": every value once."""
    vs = values()
    hdr = constants()[0]
    if name in ("512", "1k"):
        lim = hdr if name == "512" else ONE_K
        idx = [i for i, v in enumerate(vs) if len(v) <= lim]
        idx = (idx * (N_SPLIT // len(idx) + 1))[:N_SPLIT]
        return [int(i) for i in np.random.default_rng(len(idx) + len(name)).permutation(idx)]
    if name == "16k":
        long = [i for i, v in enumerate(vs) if len(v) > LONG]
        idx = [i for i, v in enumerate(vs) if len(v) <= LONG]
        idx = long + (idx * (N_SPLIT // len(idx) + 1))[:N_SPLIT - len(long)]
        return [int(i) for i in np.random.default_rng(len(idx) + len(name)).permutation(idx)]
    if name == "mono":
        return [i for i, v in enumerate(vs) if len(v) <= 4096]
    if name == "all":
        return list(range(len(vs)))
    raise KeyError(name)


DUMMY = b"x"     # the 1-byte first value of an unaligned batch


def packed(idx, align):
    """(the values of a batch row as they are sent, their source offsets): align 4 -- the values idx at pack()'s
    default; align 1 -- DUMMY first, then the values idx back to back, so that sources fall on odd addresses (the
    buffer itself is at least 256-byte aligned)."""
    vs = values()
    vals = ([DUMMY] if align == 1 else []) + [vs[i] for i in idx]
    slots = [(len(v) + align - 1) // align * align for v in vals]
    offs = [0]
    for x in slots[:-1]:
        offs.append(offs[-1] + x)
    return vals, offs


def explain(got, want):
    """deflate_dissect.explain's verdict (tokens, lengths or bit emission), then what the first differing bit lies in
    in the oracle's member `want`: the token (with its bit position, word offset, width and codes), the tree header,
    the end-of-block code or the trailer -- a wrong OR shows as other tokens or as a failed dissection, and this names
    the place it went wrong."""
    msg = DD.explain(got, want)
    bit = next((8 * k + ((got[k] ^ want[k]) & -(got[k] ^ want[k])).bit_length() - 1
                for k in range(min(len(got), len(want))) if got[k] != want[k]), None)
    if bit is None:
        return msg
    where = "the gzip header" if bit < 80 else "the padding or the trailer"
    for blk in dissect(want) if bit >= 80 else ():
        if bit < blk["start_bit"] or blk["type"] == 0 or bit >= blk["end_bit"]:
            continue
        if bit < blk["start_bit"] + 3 + blk.get("hdr_bits", 0):
            where = f"the block or tree header ({blk.get('hdr_bits', 0)} header bits from bit {blk['start_bit'] + 3})"
            break
        where = "the end-of-block code"
        for k, (t0, w, lc, lx, dc, dx) in enumerate(blk["tokens"]):
            if t0 <= bit < t0 + w:
                what = f"literal {lx}" if lc == LIT else f"lcode {lc} extra {lx}, dcode {dc} extra {dx}"
                where = (f"token #{k} (starts at bit {t0}, word offset {t0 & 31}, {w} bits: {what}), "
                         f"{bit - t0} bits in")
                break
        break
    return msg + f"; first differing bit {bit} lies in {where}"


class BackGolden:
    """tests/golden/back_golden.json (tests/golden/make_back_golden.py): the reference's member of every value of
    values() and big(), as SHA-256 + length, keyed by the value's SHA-256."""

    def __init__(self):
        with open(os.path.join(GOLDEN, "back_golden.json")) as f:
            self.vectors = json.load(f)["vectors"]

    def mismatches(self, vals, members):
        """Indices whose member is not the reference's (or whose value has no vector)."""
        bad = []
        for k, (v, m) in enumerate(zip(vals, members)):
            want = self.vectors.get(sha(v))
            if want is None or len(m) != want["gz_len"] or sha(m) != want["gz_sha256"]:
                bad.append(k)
        return bad

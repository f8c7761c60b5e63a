"""Gzip members this project's compressor never writes: zlib's own at every level, strategy, memLevel and
flush, hand-assembled valid and invalid streams (tests/deflate_builder.py), and mutations of both.

entries(golden_corpus) is deterministic (fixed seeds) and stores no expected result: what a member must
decode to comes from zlib and the CPU oracle at test time.  An entry's `value` is what its author meant
it to hold (None where there is no such thing), `size` the output size the author meant (capacities and
the trailer are sized by it), `multi` whether it has more than one block.

Categories: zlib, crafted-valid, crafted-invalid (every one a data error), crafted-truncated (the one
construct whose verdict is "input ends": a name field without end), mutated.
"""
import zlib
from collections import namedtuple

import numpy as np

import deflate_builder as B

Entry = namedtuple("Entry", "name category member value size multi")

SIZES = [1, 5, 60, 255, 256, 257, 1024, 1025, 4096, 4097, 9000, 16383, 16384, 20000, 40000, 70000]
LEVELS = [0, 1, 6, 9]
STRATEGIES = [("default", zlib.Z_DEFAULT_STRATEGY), ("filtered", zlib.Z_FILTERED), ("huffman", zlib.Z_HUFFMAN_ONLY),
              ("rle", zlib.Z_RLE), ("fixed", zlib.Z_FIXED)]
MEMLEVELS = [1, 8, 9]
FLUSHES = [("none", None), ("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH)]
CONTENTS = ["json", "alpha4", "random", "repeat"]

_cache = {}


def _seed(name):
    return zlib.crc32(name.encode())


def content(golden_corpus, kind, size, seed):
    rng = np.random.default_rng(seed)
    if kind == "json":
        src = golden_corpus
        while len(src) < size + 1:
            src = src * 2
        o = int(rng.integers(0, len(src) - size))
        return src[o:o + size]
    if kind == "alpha4":
        return bytes(rng.integers(0, 4, size, dtype=np.uint8))
    if kind == "random":
        return bytes(rng.integers(0, 256, size, dtype=np.uint8))
    return bytes([int(rng.integers(1, 256))]) * size


def zlib_member(value, level, strategy, mem, flush):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    if flush is None:
        return c.compress(value) + c.flush()
    h = len(value) // 2
    return c.compress(value[:h]) + c.flush(flush) + c.compress(value[h:]) + c.flush()


def _zlib_entries(golden_corpus):
    out = []

    def add(size, level, sname, strat, mem, fname, flush, kind):
        name = f"zlib-{size}-l{level}-{sname}-m{mem}-{fname}-{kind}"
        v = content(golden_corpus, kind, size, _seed(name))
        multi = flush is not None or (mem == 1 and size >= 256) or size > 16383
        out.append(Entry(name, "zlib", zlib_member(v, level, strat, mem, flush), v, size, multi))

    i = 0
    for size in SIZES:
        if size <= 4097:  # every strategy x flush x memLevel, twice, levels and contents in rotation
            for sname, strat in STRATEGIES:
                for mem in MEMLEVELS:
                    for fname, flush in FLUSHES:
                        for rep in range(2):
                            add(size, LEVELS[(i + rep) % 4], sname, strat, mem, fname, flush,
                                CONTENTS[(i // 4 + 2 * rep + i) % 4])
                        i += 1
        else:  # default and fixed at a compressing level, and level 0, with and without a flush
            for fname, flush in FLUSHES:
                for mem in MEMLEVELS:
                    for sname, strat in (STRATEGIES[0], STRATEGIES[4]):
                        add(size, (1, 6, 9)[i % 3], sname, strat, mem, fname, flush, CONTENTS[i % 4])
                        i += 1
                add(size, 0, "default", zlib.Z_DEFAULT_STRATEGY, 8, fname, flush, CONTENTS[i % 4])
                i += 1
    for level in LEVELS:
        out.append(Entry(f"zlib-empty-l{level}", "zlib", zlib_member(b"", level, zlib.Z_DEFAULT_STRATEGY, 8, None),
                         b"", 0, False))
    return out


# ------------------------------------------------------------------ hand-assembled, valid
SMALL, MID = 200, 1500  # the two size classes' usual output sizes (<= 256, and 257..4096)


def _mixed_tokens(rng, size, alphabet, max_dist=None, lengths=(3, 4, 5, 9, 17, 40), start=b""):
    """Literals from `alphabet` and matches into what was produced, `size` output bytes in all."""
    toks, n = [], len(start)
    have = n
    while have - n < size:
        left = size - (have - n)
        if have >= 4 and left >= 3 and rng.random() < 0.3:
            ln = min(int(lengths[int(rng.integers(len(lengths)))]), left)
            d = int(rng.integers(1, min(have, max_dist or 32768) + 1))
            if ln >= 3:
                toks.append((ln, d))
                have += ln
                continue
        toks.append(int(alphabet[int(rng.integers(len(alphabet)))]))
        have += 1
    return toks


def _raw(tokens_blocks):
    """One writer's bytes and value from a list of callables (w, value_so_far) -> new value."""
    w = B.BitWriter()
    v = b""
    for f in tokens_blocks:
        v = f(w, v)
    return w.getvalue(), v


def _dyn(tokens, final, lit_lens=None, dist_lens=None, **kw):
    def f(w, v):
        ll, dl = (lit_lens, dist_lens) if lit_lens is not None else B.lengths_for(tokens)
        B.dynamic_block(w, tokens, ll, dl, final, **kw)
        return B.apply_tokens(tokens, v)
    return f


def _fix(tokens, final):
    def f(w, v):
        B.fixed_block(w, tokens, final)
        return B.apply_tokens(tokens, v)
    return f


def _sto(data, final, **kw):
    def f(w, v):
        B.stored_block(w, data, final, **kw)
        return v + data
    return f


def _crosses(cl_symbols, nlit, want):
    """Whether a repeat symbol in `want` spans the lit/len -> distance boundary."""
    at = 0
    for s, x in cl_symbols:
        n = 1 if s < 16 else (3 + x if s in (16, 17) else 11 + x)
        if s in want and at < nlit < at + n:
            return True
        at += n
    return False


def _valid_entries(golden_corpus):
    out = []
    A = list(b"abcdefgh\x00\n")

    def add(label, raw, value, multi=False, **hdr):
        out.append(Entry("valid-" + label, "crafted-valid", B.gzip_member(raw, value, **hdr), value, len(value), multi))

    for cls, size in (("s", SMALL), ("m", MID)):
        rng = np.random.default_rng(_seed("valid" + cls))
        # every lit/len and every distance symbol has a code
        toks = _mixed_tokens(rng, 40 if cls == "s" else 600, list(range(256)))
        ll = B.balanced_lengths(286, list(range(286)))
        dl = B.balanced_lengths(30, list(range(30)))
        add(f"allcodes-{cls}", *_raw([_dyn(toks, True, ll, dl)]))
        # code lengths 1..15 in both codes
        syms = list(range(97, 110)) + [256, 257, 258]
        ll = [0] * 259
        for k, s in enumerate(syms):
            ll[s] = min(k + 1, 15)
        dl = [min(k + 1, 15) for k in range(16)]
        assert B.kraft(ll) == 32768 and B.kraft(dl) == 32768
        toks = [97 + min(int(rng.geometric(0.5)) - 1, 12) for _ in range(size - 20)]
        toks += [(3, 1), (4, 2), (3, 130), (4, 140), (3, 3), (3, 129)]  # 257/258 and distance symbols 14: 15 bits
        add(f"len15-{cls}", *_raw([_dyn(toks, True, ll, dl)]))
        # one distance code of one bit: the permitted incomplete code
        toks, have = [120], 1
        while have + 30 <= size:
            toks.append((int(rng.integers(3, 30)), 1))
            have += toks[-1][0]
        ll, dl = B.lengths_for(toks)
        assert dl == [1]
        add(f"onedist-{cls}", *_raw([_dyn(toks, True, ll, dl)]))
        # HDIST = 0 with a zero-length code: literals only
        toks = [int(A[int(rng.integers(len(A)))]) for _ in range(size)]
        ll, dl = B.lengths_for(toks)
        assert dl == [0]
        add(f"nodist-{cls}", *_raw([_dyn(toks, True, ll, dl)]))
        # a zero run across the lit/len -> distance boundary
        toks = _mixed_tokens(rng, size, A, max_dist=8, lengths=(3,))
        toks = [t if isinstance(t, int) else (3, 5 + t[1] % 4) for t in toks[8:]]
        toks = [97, 98, 99, 100, 101, 102, 103, 104] + toks
        ll = B.balanced_lengths(270, sorted(set(A) | {256, 257}))
        dl = [0, 0, 0, 0, 1, 1]
        cl = B.cl_symbols_rle(ll + dl)
        assert _crosses(cl, 270, (17, 18))
        add(f"zerorun-cross-{cls}", *_raw([_dyn(toks, True, ll, dl, cl_symbols=cl)]))
        # a repeat-16 run across the boundary
        ll = B.balanced_lengths(286, list(range(60, 286)) + list(range(60)))
        dl = [8, 8, 7, 6, 5, 4, 3, 2, 1]
        assert B.kraft(dl) == 32768
        cl = B.cl_symbols_rle(ll + dl)
        assert _crosses(cl, 286, (16,))
        toks = _mixed_tokens(rng, size, list(range(256)), max_dist=24)
        add(f"rep16-cross-{cls}", *_raw([_dyn(toks, True, ll, dl, cl_symbols=cl)]))
        # a final empty stored block after data; an empty stored block first
        toks = _mixed_tokens(rng, size, A)
        add(f"final-empty-stored-{cls}", *_raw([_fix(toks, False), _sto(b"", True)]), multi=True)
        # every order of two block kinds, a match in the later block reaching into the earlier
        half = size // 2
        kinds = ["stored", "empty", "fixed", "dynamic"]
        for k1 in kinds:
            for k2 in kinds:
                first = bytes(rng.integers(0, 256, half, dtype=np.uint8))
                t1 = _mixed_tokens(rng, half, A)
                b1 = {"stored": _sto(first, False), "empty": _sto(b"", False), "fixed": _fix(t1, False),
                      "dynamic": _dyn(t1, False)}[k1]
                n1 = 0 if k1 == "empty" else half
                t2 = ([(min(half, 20), n1), (3, 1)] if n1 else [65, (5, 1)]) + _mixed_tokens(rng, half - 24, A)
                b2 = {"stored": _sto(bytes(rng.integers(0, 256, half, dtype=np.uint8)), True), "empty": _sto(b"", True),
                      "fixed": _fix(t2, True), "dynamic": _dyn(t2, True)}[k2]
                add(f"pair-{k1}-{k2}-{cls}", *_raw([b1, b2]), multi=True)
        # header fields
        v = content(golden_corpus, "json", size, _seed("hdr" + cls))
        raw = zlib.compress(v, 6)[2:-4]
        add(f"fextra-{cls}", raw, v, extra=b"AP\x04\x00data")
        add(f"fname-{cls}", raw, v, name=b"value.json\x00")
        add(f"fcomment-{cls}", raw, v, comment=b"a comment\x00")
        add(f"fhcrc-{cls}", raw, v, hcrc=True)
        add(f"allflags-{cls}", raw, v, extra=b"\x01\x02\x00\x00", name=b"n\x00", comment=b"\x00", hcrc=True, text=True,
            mtime=0x5F3759DF, xfl=2, os=255)
        add(f"mtime-{cls}", raw, v, mtime=1700000000, xfl=0, os=0)
        add(f"xfl2-{cls}", raw, v, xfl=2, os=11)
        add(f"xfl4-{cls}", raw, v, xfl=4, os=7)
        # a member followed by 1 KiB of arbitrary bytes
        m = B.gzip_member(raw, v)
        junk = bytes(rng.integers(0, 256, 1024, dtype=np.uint8))
        out.append(Entry(f"valid-trailing-{cls}", "crafted-valid", m + junk, v, len(v), False))

    rng = np.random.default_rng(_seed("valid-big"))
    # length 258 by symbol 285 and by symbol 284 + 31 (a match alone is past 256 bytes: no small form)
    toks = [97, (258, 1), (258, 1, 284), 98, (258, 259, 284), (258, 2)]
    add("len258-fixed", *_raw([_fix(toks, True)]))
    add("len258-dynamic", *_raw([_dyn(toks, True)]))
    # length 3 at distance 1, then every length symbol and every distance symbol, ~40 KB
    toks = [7, (3, 1)] + _mixed_tokens(rng, 33000, A, start=b"xxxx")
    for k in range(30):
        ls = 257 + k % 29
        longest = B.LEN_BASE[ls - 257] + (1 << B.LEN_EXTRA[ls - 257]) - 1  # (symbol 284's is 258 as well)
        toks.append((longest, B.DIST_BASE[k] + (1 << B.DIST_EXTRA[k]) - 1, ls))
        toks.append(int(rng.integers(0, 256)))
        toks.append((B.LEN_BASE[(k * 7) % 29], B.DIST_BASE[k]))
    toks += _mixed_tokens(rng, 2000, A, start=b"xxxx")
    add("everysym-dynamic", *_raw([_dyn(toks, True)]))
    add("everysym-fixed", *_raw([_fix(toks, True)]))
    # distance 32768, length 258, reaching the first byte of a 32768-byte stored block
    first = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    add("dist32768", *_raw([_sto(first, False), _fix([(258, 32768), 1, (258, 32768)], True)]), multi=True)
    # a stored block of 65535 bytes
    add("stored65535", *_raw([_sto(bytes(rng.integers(0, 256, 65535, dtype=np.uint8)), True)]))
    # the empty value: an empty stored block, an empty fixed block, the latter with nonzero pad bits
    add("empty-stored", *_raw([_sto(b"", True)]))
    add("empty-fixed", b"\x03\x00", b"")
    add("empty-fixed-padbits", b"\x03\xfc", b"")
    return out


# ------------------------------------------------------------------ hand-assembled, invalid
def _invalid_entries(golden_corpus):
    out = []
    A = list(b"abcdefgh\x00\n")

    def add(label, raw, size, value=None, category="crafted-invalid", **hdr):
        v = value if value is not None else bytes(size)
        hdr.setdefault("isize", size)
        out.append(Entry("invalid-" + label, category, B.gzip_member(raw, v, **hdr), None, size, False))

    def four(name, defect, tail=True):
        """defect(w, value_so_far, rng): the defective block.  First block and a later block, two sizes."""
        for cls, size in (("s", SMALL), ("m", MID)):
            for where in ("first", "later"):
                rng = np.random.default_rng(_seed(name + cls + where))
                w = B.BitWriter()
                v = b""
                if where == "later":  # (half the claimed size is produced before the defect)
                    toks = _mixed_tokens(rng, size // 2, A)
                    if _seed(name) & 1:
                        B.fixed_block(w, toks, False)
                    else:
                        B.dynamic_block(w, toks, *B.lengths_for(toks), False)
                    v = B.apply_tokens(toks)
                defect(w, v, rng)
                raw = w.getvalue()
                if tail:
                    raw += bytes(rng.integers(0, 256, 6, dtype=np.uint8))
                e = Entry(f"invalid-{name}-{cls}-{where}", "crafted-invalid",
                          B.gzip_member(raw, v, isize=size), None, size, where == "later")
                out.append(e)

    def fixed_with(extra_tokens):
        def d(w, v, rng):
            B.fixed_block(w, [104, 105, 106] + extra_tokens + [107, 108], True)
        return d

    four("litlen286", fixed_with([("sym", 286)]))
    four("litlen287", fixed_with([("sym", 287)]))
    four("dist30", fixed_with([("dsym", 3, 30, 0, 0)]))
    four("dist31", fixed_with([("dsym", 4, 31, 0, 0)]))

    def too_far(w, v, rng):  # one past the bytes produced so far (distance 1 at the very start)
        ds, dn, dx = B.dist_symbol(len(v) + 1)
        B.fixed_block(w, [("dsym", 3, ds, dn, dx), 100, 101], True)
    four("toofar", too_far)

    def too_far_after_literals(w, v, rng):
        ds, dn, dx = B.dist_symbol(len(v) + 6)
        B.fixed_block(w, [1, 2, 3, 4, 5, ("dsym", 9, ds, dn, dx), 100], True)
    four("toofar-lits", too_far_after_literals)

    def mismatch(w, v, rng):
        B.stored_block(w, b"stored bytes", True, nlen=(12 ^ 0xFFFF) ^ 0x0100)
    four("lennlen", mismatch)

    def btype3(w, v, rng):
        w.bits(1, 1)
        w.bits(3, 2)
    four("btype3", btype3)

    def hfield(hlit, hdist):
        def d(w, v, rng):
            B.dynamic_header(w, True, hlit, hdist, B.cl_symbols_rle([8] * 40))
        return d
    four("hlit30", hfield(30, 5))
    four("hlit31", hfield(31, 5))
    four("hdist30", hfield(3, 30))
    four("hdist31", hfield(3, 31))

    good_l = B.balanced_lengths(257, [97, 98, 99, 256])
    good_d = [1, 1]

    def codes(lit_lens, dist_lens, cl_lengths=None, cl_symbols=None):
        def d(w, v, rng):
            cl = cl_symbols if cl_symbols is not None else B.cl_symbols_rle(list(lit_lens) + list(dist_lens))
            B.dynamic_header(w, True, len(lit_lens) - 257, len(dist_lens) - 1, cl, cl_lengths)
            w.bits(0x2A5, 10)
        return d

    def lens257(d):
        ll = [0] * 257
        for s, n in d.items():
            ll[s] = n
        return ll

    cl19 = lambda d: [d.get(s, 0) for s in range(19)]  # noqa: E731
    # (the code-length symbols the good lengths need: 0, 1, 2, 17, 18)
    four("clcode-incomplete", codes(good_l, good_d, cl19({0: 2, 1: 3, 2: 3, 17: 3, 18: 3})))
    four("clcode-oversubscribed", codes(good_l, good_d, cl19({0: 1, 1: 2, 2: 2, 17: 2, 18: 3})))
    four("lit-incomplete", codes(lens257({97: 2, 98: 2, 256: 2}), good_d))
    four("lit-oversubscribed", codes(lens257({97: 1, 98: 1, 256: 1}), good_d))
    four("lit-single-long", codes(lens257({256: 2}), good_d))
    four("dist-incomplete", codes(good_l, [2, 2, 2]))
    four("dist-oversubscribed", codes(good_l, [1, 1, 1]))
    four("dist-single-long", codes(good_l, [0, 2]))
    four("no-eob", codes(B.balanced_lengths(257, [97, 98, 99, 100]), good_d))
    plain = B.cl_symbols_rle(good_l + good_d)
    four("rep16-first", codes(good_l, good_d, cl_symbols=[(16, 0)] + plain))
    over = B.cl_symbols_rle(good_l[:250]) + [(18, 127)]  # 250 + 138 > 257 + 2
    four("repeat-overrun", codes(good_l, good_d, cl_symbols=over))
    over16 = B.cl_symbols_plain(good_l) + [(1, 0), (16, 3)]  # 257 + 1 + 6 > 259
    four("rep16-overrun", codes(good_l, good_d, cl_symbols=over16))

    # the sizes the construct itself fixes: a distance one past 4096 and one past 32767 bytes produced
    rng = np.random.default_rng(_seed("invalid-big"))
    for produced in (4096, 32767):
        w = B.BitWriter()
        first = bytes(rng.integers(0, 256, produced, dtype=np.uint8))
        B.stored_block(w, first, False)
        ds, dn, dx = B.dist_symbol(produced + 1)
        B.fixed_block(w, [("dsym", 258, ds, dn, dx), 9], True)
        out.append(Entry(f"invalid-toofar-at-{produced + 1}", "crafted-invalid",
                         B.gzip_member(w.getvalue(), first, isize=produced + 259), None, produced + 259, True))

    # header and trailer defects on a valid stream
    for cls, size in (("s", SMALL), ("m", MID)):
        v = content(golden_corpus, "json", size, _seed("inv-hdr" + cls))
        raw = zlib.compress(v, 9)[2:-4]
        add(f"fhcrc-bad-{cls}", raw, size, v, hcrc=True, hcrc_value=0x1234)
        for bit in (0x20, 0x40, 0x80):
            add(f"flg-reserved-{bit:02x}-{cls}", raw, size, v, flg=bit)
        add(f"crc-wrong-{cls}", raw, size, v, crc=zlib.crc32(v) ^ 0x00010000)
        add(f"isize-plus-{cls}", raw, size, v, isize=size + 1)
        add(f"isize-minus-{cls}", raw, size, v, isize=size - 1)
        add(f"cm-not-8-{cls}", raw, size, v)
        m = bytearray(out[-1].member)
        m[2] = 7
        out[-1] = out[-1]._replace(member=bytes(m))
        # FNAME without its NUL: the scan for it runs on through what was meant as the stream.  Its first
        # zero byte ends the "name", and the byte after it reads as BFINAL 1, BTYPE 3.
        body = bytes(b or 1 for b in raw)
        add(f"fname-unterminated-{cls}", body + b"\x00\x07" + b"\x55" * 6, size, v, flg=B.FNAME)
        # ... and with no zero byte anywhere the input just ends: truncated, not corrupt
        add(f"fname-endless-{cls}", body, size, v, category="crafted-truncated", flg=B.FNAME, crc=0x01020304,
            isize=0x01010000 | size | 0x0100)
    return out


# ------------------------------------------------------------------ mutations
def _mutations(base):
    """20 single-bit flips and 5 truncations of ~60 members spread over the size classes, and 5 more
    flips in the second half of those that have several blocks."""
    buckets = [[], [], [], []]
    for e in base:
        if len(e.member) > 24000:
            continue  # (incompressible large values: the compressible ones of those sizes do)
        b = 0 if e.size <= 256 else 1 if e.size <= 4096 else 2 if e.size <= 16383 else 3
        buckets[b].append(e)
    picked = []
    for b, want in zip(buckets, (12, 14, 14, 20)):
        step = max(1, len(b) // want)
        picked += b[step // 2::step][:want]
    out = []
    for e in picked:
        rng = np.random.default_rng(_seed("mut" + e.name))
        m = e.member
        nbits = len(m) * 8

        def flip(k, lo):
            t = bytearray(m)
            bit = int(rng.integers(lo, nbits))
            t[bit >> 3] ^= 1 << (bit & 7)
            out.append(Entry(f"mut-{e.name}-flip{k}", "mutated", bytes(t), None, e.size, e.multi))
        for k in range(20):
            flip(k, 0)
        if e.multi:
            for k in range(20, 25):
                flip(k, nbits // 2)
        for k in range(5):
            cut = int(rng.integers(1, len(m)))
            out.append(Entry(f"mut-{e.name}-cut{k}", "mutated", m[:cut], None, e.size, e.multi))
    return out


def entries(golden_corpus):
    key = zlib.crc32(golden_corpus), len(golden_corpus)
    if key not in _cache:
        base = _zlib_entries(golden_corpus) + _valid_entries(golden_corpus)
        out = base + _invalid_entries(golden_corpus) + _mutations(base)
        assert len({e.name for e in out}) == len(out)
        _cache.clear()
        _cache[key] = out
    return _cache[key]


def corpus(golden_corpus):
    """[(name, category, member bytes)], deterministic."""
    return [(e.name, e.category, e.member) for e in entries(golden_corpus)]


# ------------------------------------------------------------------ the two references
def zlib_verdict(member):
    """(rc, bytes) of zlib's gzip inflate in the oracle's terms: -3 a data error, -5 input ended early."""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(member)
    except zlib.error:
        return -3, b""
    if not d.eof:
        return -5, b""
    return 0, out

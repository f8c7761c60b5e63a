"""A small DEFLATE / gzip assembler for tests, written from RFC 1951 and RFC 1952.

It writes what a compressor never would: every block type in any order, code lengths given symbol by
symbol (repeats 16/17/18 and their extra bits under the caller's control), raw symbols that no code may
use, header flags and trailers that lie.  Nothing here decodes; the expected value of a token list comes
from apply_tokens().

Tokens:  an int 0..255              a literal
         (length, distance)         a match, shortest length symbol
         (length, distance, lsym)   a match through length symbol lsym (258 as 284 + 31)
         ("sym", s)                 the bare lit/len symbol s (286, 287: never valid)
         ("dsym", length, d, nbits, extra)   a match whose distance is the bare symbol d + extra bits
"""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """LSB-first bit writer (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.nacc = 0

    def bits(self, value, count):
        """`count` bits of `value`, least significant first (header fields, extra bits)."""
        assert 0 <= value < (1 << count) or count == 0 and value == 0, (value, count)
        self.acc |= value << self.nacc
        self.nacc += count
        while self.nacc >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, code, length):
        """A Huffman code: most significant bit first."""
        rev = 0
        for k in range(length):
            rev |= ((code >> k) & 1) << (length - 1 - k)
        self.bits(rev, length)

    def align(self, pad=0):
        """Pad to a byte boundary with the low bits of `pad`."""
        if self.nacc:
            k = 8 - self.nacc
            self.bits(pad & ((1 << k) - 1), k)

    def raw(self, data):
        assert self.nacc == 0
        self.out += data

    def bitlen(self):
        return len(self.out) * 8 + self.nacc

    def getvalue(self, pad=0):
        self.align(pad)
        return bytes(self.out)


def canonical_codes(lengths):
    """[(code, length)] per symbol (RFC 1951 3.2.2).  Lengths that over-subscribe the code still give a
    list (codes masked to their length), so a block with such a header can be followed by some bits."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt = [0] * 16
    code = 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lengths:
        if n:
            out.append((nxt[n] & ((1 << n) - 1), n))
            nxt[n] += 1
        else:
            out.append((0, 0))
    return out


def kraft(lengths):
    """Sum of 2^-len in units of 2^-15: 32768 for a complete code."""
    return sum(1 << (15 - n) for n in lengths if n)


def balanced_lengths(total, used):
    """Lengths for `total` symbols giving the symbols of `used` (>= 2 of them, in order of preference for
    the shorter codes) a complete code of two adjacent lengths."""
    used = list(used)
    k = len(used)
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    lens = [0] * total
    for i, s in enumerate(used):
        lens[s] = m - 1 if i < short else m
    assert kraft(lens) == 32768
    return lens


def length_symbol(length, lsym=None):
    """(symbol, extra bit count, extra value) for a match length."""
    if lsym is None:
        if length == 258:
            lsym = 285
        else:
            lsym = 257 + max(k for k in range(28) if LEN_BASE[k] <= length)
    k = lsym - 257
    extra = length - LEN_BASE[k]
    assert 0 <= extra < (1 << LEN_EXTRA[k]) or extra == 0, (length, lsym)
    return lsym, LEN_EXTRA[k], extra


def dist_symbol(d):
    k = max(j for j in range(30) if DIST_BASE[j] <= d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


def apply_tokens(tokens, prefix=b""):
    """The bytes a decoder produces for `tokens` after `prefix` (the prefix included)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, d = t[0], t[1]
            assert isinstance(length, int) and 1 <= d <= len(out), t
            if d >= length:
                out += out[len(out) - d:len(out) - d + length]
            else:
                for _ in range(length):
                    out.append(out[-d])
    return bytes(out)


def emit_tokens(w, tokens, lit_codes, dist_codes, eob=True):
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit_codes[t])
        elif t[0] == "sym":
            w.code(*lit_codes[t[1]])
        elif t[0] == "dsym":
            _, length, dsym, nbits, extra = t
            s, n, x = length_symbol(length)
            w.code(*lit_codes[s])
            w.bits(x, n)
            w.code(*dist_codes[dsym])
            w.bits(extra, nbits)
        else:
            s, n, x = length_symbol(t[0], t[2] if len(t) > 2 else None)
            assert lit_codes[s][1], ("length symbol without a code", s)
            w.code(*lit_codes[s])
            w.bits(x, n)
            ds, dn, dx = dist_symbol(t[1])
            assert dist_codes[ds][1], ("distance symbol without a code", ds)
            w.code(*dist_codes[ds])
            w.bits(dx, dn)
    if eob:
        w.code(*lit_codes[256])


def stored_block(w, data, final, nlen=None, pad=0):
    """BTYPE 0.  nlen: override of the complement field."""
    assert len(data) <= 65535
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align(pad)
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen))
    w.raw(data)


def fixed_block(w, tokens, final, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    emit_tokens(w, tokens, canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST), eob)


def cl_symbols_plain(lengths):
    """Every code length as its own symbol 0..15."""
    return [(n, 0) for n in lengths]


def cl_symbols_rle(lengths):
    """Code-length symbols with repeats, greedy over the whole (lit/len + distance) sequence, so runs cross
    the boundary between the two codes -- which zlib's own writer never does."""
    out = []
    i, n = 0, len(lengths)
    while i < n:
        v = lengths[i]
        j = i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        i = j
    return out


def expand_cl(symbols):
    """The code lengths a sequence of (symbol, extra) stands for."""
    out = []
    for s, x in symbols:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_header(w, final, hlit, hdist, cl_symbols, cl_lengths=None, hclen=None):
    """BFINAL, BTYPE 2, HLIT / HDIST as given (the 5-bit fields: 0..31), then the code-length code and
    the sequence cl_symbols = [(symbol, extra value)].  cl_lengths (19, by symbol): override of the
    code-length code, which otherwise is a complete one over the symbols used."""
    if cl_lengths is None:
        freq = {}
        for s, _ in cl_symbols:
            freq[s] = freq.get(s, 0) + 1
        used = sorted(freq, key=lambda s: (-freq[s], s))
        for filler in (0, 1, 2):
            if len(used) >= 2:
                break
            if filler not in used:
                used.append(filler)  # a one-symbol code would be incomplete
        cl_lengths = balanced_lengths(19, used)
    if hclen is None:
        hclen = max([k for k in range(19) if cl_lengths[CL_ORDER[k]]] + [3]) + 1
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit, 5)
    w.bits(hdist, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lengths[CL_ORDER[k]], 3)
    codes = canonical_codes(cl_lengths)
    for s, x in cl_symbols:
        w.code(*codes[s])
        if s >= 16:
            w.bits(x, CL_EXTRA[s])


def dynamic_block(w, tokens, lit_lens, dist_lens, final, cl_symbols=None, cl_lengths=None, eob=True):
    """BTYPE 2 with the given code lengths (257..286 lit/len, 1..30 distance) and, unless cl_symbols
    says otherwise, greedy repeats over the joined sequence."""
    assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
    if cl_symbols is None:
        cl_symbols = cl_symbols_rle(list(lit_lens) + list(dist_lens))
    dynamic_header(w, final, len(lit_lens) - 257, len(dist_lens) - 1, cl_symbols, cl_lengths)
    emit_tokens(w, tokens, canonical_codes(lit_lens), canonical_codes(dist_lens), eob)


def lengths_for(tokens, nlit=None, ndist=None):
    """(lit_lens, dist_lens): complete balanced codes over the symbols `tokens` use (plus end-of-block);
    a lone distance symbol gets the permitted one-bit code, none at all a single zero length."""
    lits, dists = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lits.add(t)
        else:
            lits.add(length_symbol(t[0], t[2] if len(t) > 2 else None)[0])
            dists.add(dist_symbol(t[1])[0])
    if len(lits) < 2:
        lits.add(0)
    nlit = nlit or max(257, max(lits) + 1)
    lit_lens = balanced_lengths(nlit, sorted(lits))
    ndist = ndist or (max(dists) + 1 if dists else 1)
    if len(dists) >= 2:
        dist_lens = balanced_lengths(ndist, sorted(dists))
    else:
        dist_lens = [0] * ndist
        for d in dists:
            dist_lens[d] = 1
    return lit_lens, dist_lens


FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def gzip_member(deflate, value, extra=None, name=None, comment=None, hcrc=False, mtime=0, xfl=0, os=3, flg=None,
                hcrc_value=None, crc=None, isize=None, text=False):
    """A gzip member (RFC 1952) around raw DEFLATE bytes.  The fields present set their FLG bits; flg
    overrides the byte (reserved bits); hcrc_value, crc and isize override what is computed from the
    header and from `value`."""
    f = (FTEXT if text else 0) | (FHCRC if hcrc else 0) | (FEXTRA if extra is not None else 0) | (
        FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0)
    head = bytearray(b"\x1f\x8b\x08" + bytes([f if flg is None else flg]) + struct.pack("<I", mtime) + bytes([xfl, os]))
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name  # (the caller ends it with a NUL, or does not)
    if comment is not None:
        head += comment
    if hcrc:
        head += struct.pack("<H", (zlib.crc32(bytes(head)) & 0xFFFF) if hcrc_value is None else hcrc_value)
    return bytes(head) + deflate + struct.pack("<II", zlib.crc32(value) if crc is None else crc,
                                               (len(value) & 0xFFFFFFFF) if isize is None else isize)

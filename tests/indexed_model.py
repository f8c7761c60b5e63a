"""Indexed members (include/pmc_codec.h "member index"), stated in plain Python: with the index switch on, a
PMC_LEVEL_FAST_ALL value of more than C bytes is cut into chunks of C bytes, and every chunk is parsed as
tests/fast_large_model.py parses a value -- the history stops at the chunk's first byte, so chunks decode
independently.  parse_index reads the gzip FEXTRA field that says where the chunks begin, by the rules of
csrc/pmc_plan.hpp idx_parse (= pmc_gzip_index_info, = the decoder's scan)."""
from fast_large_model import G, fast_large_tokens

C = 32768            # chunk bytes (csrc/pmc_plan.hpp PMC_IDX_CHUNK)
LOG2C = 15
MAX_CHUNKS = 16382   # XLEN = 8 + 4 (K - 1) fits 16 bits
assert C == 1 << LOG2C and C % G == 0


def is_indexed(n: int) -> bool:
    """Does the switch act on a fast-all value of n bytes?"""
    return n > C and -(-n // C) <= MAX_CHUNKS


def header_len(n: int) -> int:
    return 20 + 4 * (-(-n // C) - 1) if is_indexed(n) else 10


def indexed_chunks(v):
    """The token list of every chunk."""
    v = bytes(v)
    return [fast_large_tokens(v[c:c + C]) for c in range(0, len(v), C)]


def replay(tokens) -> bytes:
    """The bytes a token list stands for, decoded behind nothing."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            ln, dist = t
            assert 1 <= dist <= len(out), (t, len(out))
            for _ in range(ln):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)


def header(n: int, offsets, log2c=LOG2C, version=1, sid=b"PI") -> bytes:
    """The header of an indexed member of a value of n bytes whose chunks 1.. begin at `offsets`."""
    k1 = len(offsets)
    return (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x04\x03" + (8 + 4 * k1).to_bytes(2, "little") + sid +
            (4 + 4 * k1).to_bytes(2, "little") + bytes([version, log2c, 0, 0]) +
            b"".join(int(o).to_bytes(4, "little") for o in offsets))


def assemble(v: bytes, chunk=C, log2c=None, tokens_of=fast_large_tokens) -> bytes:
    """An indexed member of v put together on the CPU with tests/deflate_builder.py: every chunk one fixed
    block of its tokens, the empty stored block between chunks, the header above.  (The library writes
    dynamic blocks of 16383 symbols; the layout is the same.)"""
    import deflate_builder as B
    v = bytes(v)
    assert len(v) > chunk
    k = -(-len(v) // chunk)
    hdr = 20 + 4 * (k - 1)
    w = B.BitWriter()
    offsets = []
    for j in range(k):
        part = v[j * chunk:(j + 1) * chunk]
        if j:
            B.stored_block(w, b"", False)
            offsets.append(hdr + len(w.out))
        B.fixed_block(w, tokens_of(part), j == k - 1)
    lg = chunk.bit_length() - 1 if log2c is None else log2c
    h = header(len(v), offsets, lg)
    return B.gzip_member(w.getvalue(), v, extra=h[12:], xfl=4)


def parse_index(m: bytes):
    """(chunk_bytes, nchunks, offsets, header_end) of the index member m carries, or None."""
    m = bytes(m)
    n = len(m)
    if n < 20 + 4 + 8 + 1 or m[:4] != b"\x1f\x8b\x08\x04":
        return None
    xlen, sl = int.from_bytes(m[10:12], "little"), int.from_bytes(m[14:16], "little")
    if m[12:14] != b"PI" or sl < 8 or sl % 4 or xlen < sl + 4:
        return None
    if m[16] != 1 or m[18] or m[19]:
        return None
    lg, k, hdr = m[17], sl // 4, 12 + xlen
    if not 12 <= lg <= 24 or hdr + 8 >= n:
        return None
    isize = int.from_bytes(m[-4:], "little")
    if k < 2 or (isize + (1 << lg) - 1) >> lg != k:
        return None
    offs = [int.from_bytes(m[20 + 4 * j:24 + 4 * j], "little") for j in range(k - 1)]
    prev = hdr
    for o in offs:
        if o <= prev or o + 8 >= n:
            return None
        prev = o
    return 1 << lg, k, offs, hdr

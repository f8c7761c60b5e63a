"""Chunk CRCs of indexed members (include/pmc_codec.h "member index", chunk CRCs), stated in plain Python: the
second FEXTRA subfield 'P' 'C' directly behind the 'P' 'I' one, which holds zlib.crc32 of every chunk of the
value; when a member carries it (csrc/pmc_plan.hpp idx_crc_parse = pmc_gzip_index_crc_info = the ranged read's
scan); and what a ranged read answers with it (csrc/pmc_inflate_range.hip)."""
import zlib

from fast_large_model import fast_large_tokens
from indexed_model import C, MAX_CHUNKS, header, parse_index
from range_model import chunk_bytes, covered, range_of

CRC_MAX_CHUNKS = 8190   # XLEN = 8 K + 12 fits 16 bits (csrc/pmc_plan.hpp kIdxCrcMaxChunks)
CRC_FIXED = 8           # 'P' 'C', LEN, version, three reserved bytes (kIdxCrcFixed)


def plan(n: int, chunk=C, crc=True):
    """csrc/pmc_plan.hpp idx_plan: (indexed, K, header bytes, carries CRCs, byte of chunk 0's entry)."""
    if chunk == 0 or n <= chunk:
        return False, 1, 10, False, 0
    k = -(-n // chunk)
    if k > MAX_CHUNKS:
        return False, 1, 10, False, 0
    hdr = 20 + 4 * (k - 1)
    if crc and k <= CRC_MAX_CHUNKS:
        return True, k, hdr + CRC_FIXED + 4 * k, True, hdr + CRC_FIXED
    return True, k, hdr, False, 0


def chunk_crcs(v: bytes, chunk=C):
    return [zlib.crc32(v[c:c + chunk]) for c in range(0, len(v), chunk)]


def crc_subfield(crcs, sid=b"PC", version=1, reserved=(0, 0, 0), length=None) -> bytes:
    ln = 4 + 4 * len(crcs) if length is None else length
    return (sid + ln.to_bytes(2, "little") + bytes([version, *reserved]) +
            b"".join(int(c).to_bytes(4, "little") for c in crcs))


def header_crc(n: int, offsets, crcs, log2c=15, sub=None) -> bytes:
    """The header of a member with chunk CRCs: indexed_model.header with XLEN grown by the second subfield, then
    the subfield (or the bytes `sub` in its place).  `offsets` count from the member's first byte, as ever."""
    h = header(n, offsets, log2c)
    sub = crc_subfield(crcs) if sub is None else sub
    xlen = int.from_bytes(h[10:12], "little") + len(sub)
    return h[:10] + xlen.to_bytes(2, "little") + h[12:] + sub


def assemble_crc(v: bytes, chunk=C, log2c=None, tokens_of=fast_large_tokens, sub=None) -> bytes:
    """indexed_model.assemble plus the 'P' 'C' subfield: the same fixed blocks and separators, every offset
    8 + 4 K larger.  sub: other bytes in the subfield's place (crc_defects), the offsets shifted by their
    number."""
    import deflate_builder as B
    v = bytes(v)
    assert len(v) > chunk
    k = -(-len(v) // chunk)
    hdr = 20 + 4 * (k - 1) + (CRC_FIXED + 4 * k if sub is None else len(sub))
    w = B.BitWriter()
    offsets = []
    for j in range(k):
        part = v[j * chunk:(j + 1) * chunk]
        if j:
            B.stored_block(w, b"", False)
            offsets.append(hdr + len(w.out))
        B.fixed_block(w, tokens_of(part), j == k - 1)
    lg = chunk.bit_length() - 1 if log2c is None else log2c
    h = header_crc(len(v), offsets, chunk_crcs(v, chunk), lg, sub)
    assert len(h) == hdr
    return B.gzip_member(w.getvalue(), v, extra=h[12:], xfl=4)


def crc_defects(v: bytes, chunk=C):
    """{name: bytes in the subfield's place}: every single defect of the subfield.  Each gives, through
    assemble_crc(v, chunk, sub=...), a valid indexed member that carries no chunk CRCs."""
    crcs = chunk_crcs(v, chunk)
    k = len(crcs)
    good = crc_subfield(crcs)
    return {
        "id": crc_subfield(crcs, sid=b"PD"), "id2": crc_subfield(crcs, sid=b"QC"), "id_pi": crc_subfield(crcs, sid=b"PI"),
        "len-4": crc_subfield(crcs, length=4 * k), "len+4": crc_subfield(crcs, length=8 + 4 * k),
        "version0": crc_subfield(crcs, version=0), "version2": crc_subfield(crcs, version=2),
        "reserved1": crc_subfield(crcs, reserved=(1, 0, 0)), "reserved2": crc_subfield(crcs, reserved=(0, 1, 0)),
        "reserved3": crc_subfield(crcs, reserved=(0, 0, 1)),
        "xlen_short": good[:-4],   # XLEN ends one entry before the subfield does
        "xlen_short1": good[:-1],
        "not_directly_behind": b"XY\x00\x00" + good,   # an empty foreign subfield between the two
        "absent": b"",
    }


def parse_chunk_crcs(m: bytes):
    """The list of chunk CRCs the member m carries, or None (csrc/pmc_plan.hpp idx_crc_parse)."""
    m = bytes(m)
    idx = parse_index(m)
    if idx is None:
        return None
    _, k, _, hdr = idx
    p = 16 + 4 * k
    if p + CRC_FIXED + 4 * k > hdr:
        return None
    if m[p:p + 2] != b"PC" or int.from_bytes(m[p + 2:p + 4], "little") != 4 + 4 * k:
        return None
    if m[p + 4] != 1 or m[p + 5] or m[p + 6] or m[p + 7]:
        return None
    at = p + CRC_FIXED
    return [int.from_bytes(m[at + 4 * j:at + 4 * j + 4], "little") for j in range(k)]


def read_range_verified(m: bytes, off: int, length: int, cap=None, require=False):
    """range_model.read_range plus the CRC rule: bytes, None (PMC_E_NO_INDEX) or ("capacity", L).  With `require`
    a member without chunk CRCs is declined before the empty-range and capacity verdicts."""
    m = bytes(m)
    ks = covered(m, off, length)
    if ks is None:
        return None
    crcs = parse_chunk_crcs(m)
    if require and crcs is None:
        return None
    cb = parse_index(m)[0]
    o, L, _, _ = range_of(int.from_bytes(m[-4:], "little"), cb.bit_length() - 1, off, length)
    if L == 0:
        return b""
    if cap is not None and L > cap:
        return ("capacity", L)
    parts = []
    for k in ks:
        b = chunk_bytes(m, k)
        if b is None or (crcs is not None and zlib.crc32(b) != crcs[k]):
            return None
        parts.append(b)
    whole = b"".join(parts)
    s = o - ks[0] * cb
    return whole[s:s + L]

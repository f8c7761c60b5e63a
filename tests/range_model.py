"""Ranged reads of indexed members (include/pmc_codec.h "ranged reads"), stated in plain Python: which bytes a
request gets, which chunks hold them, and when a member can be served by its chunks at all.  csrc/pmc_plan.hpp
range_of is the same arithmetic (tests/test_host_range.py), csrc/pmc_inflate_range.hip the same verdicts
(tests/test_gpu_range.py)."""
import zlib

from indexed_model import parse_index

LOG2_MAX = 16                      # the largest chunk a ranged read serves (csrc/pmc_plan.hpp kRangeLog2Max)
ROW_BYTES = (1 << LOG2_MAX) + 16   # an edge row (kRangeRowBytes)
SCRATCH_BUDGET = 2048 << 20        # all the edge rows of a call (kRangeScratchBudget)


def range_of(isize: int, lg: int, off: int, length: int):
    """(o, L, k0, items): the clamped range (Redis GETRANGE) and the chunks of 2^lg bytes that hold it."""
    o = min(off, isize)
    L = min(length, isize - o)
    if L == 0:
        return o, 0, 0, 0
    k0 = o >> lg
    return o, L, k0, ((o + L - 1) >> lg) - k0 + 1


def chunk_span(m: bytes, k: int):
    """(start, next, clen, last) of chunk k of the indexed member m."""
    cb, K, offs, hdr = parse_index(m)
    isize = int.from_bytes(m[-4:], "little")
    start = hdr if k == 0 else offs[k - 1]
    last = k == K - 1
    nxt = len(m) - 8 if last else offs[k]
    return start, nxt, min(cb, isize - k * cb), last


def chunk_bytes(m: bytes, k: int):
    """The bytes of chunk k by a strict inflate of its span alone, or None: exactly clen bytes, the span used
    up to its last byte, the stream's end only in the last chunk, and before every other chunk's end the empty
    stored block's 00 00 ff ff."""
    start, nxt, clen, last = chunk_span(m, k)
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(m[start:nxt])
    except zlib.error:
        return None
    if len(out) != clen or d.unused_data or d.eof != last:
        return None
    if not last and m[nxt - 4:nxt] != b"\x00\x00\xff\xff":
        return None
    return out


def covered(m: bytes, off: int, length: int):
    """The chunk numbers a request decodes ([] for an empty range), or None when m has no usable index."""
    idx = parse_index(m)
    if idx is None or idx[0] > 1 << LOG2_MAX:
        return None
    lg = idx[0].bit_length() - 1
    o, L, k0, items = range_of(int.from_bytes(m[-4:], "little"), lg, off, length)
    return list(range(k0, k0 + items))


def read_range(m: bytes, off: int, length: int, cap=None):
    """bytes, None (PMC_E_NO_INDEX) or ("capacity", L)."""
    m = bytes(m)
    ks = covered(m, off, length)
    if ks is None:
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
        if b is None:
            return None
        parts.append(b)
    whole = b"".join(parts)
    s = o - ks[0] * cb
    return whole[s:s + L]


def ranges_for(n: int, C: int):
    """The smallest shapes where an edge can go wrong, for a value of n > C bytes."""
    return [(0, 1), (C - 1, 2), (C, 1), (C, C), (C - 1, C + 2), (0, n), (1, n - 2), (n - 1, 1), (n - 3, 10), (n, 5),
            (n + 7, 5), (5, 0), (0, 0xFFFFFFFF)]


def plan_range(n: int, cus: int, per_cu: int, scan_block: int = 1024):
    """csrc/pmc_plan.hpp plan_range."""
    max_rows = SCRATCH_BUDGET // ROW_BYTES
    resident = max(1, cus * per_cu)
    need = (min(n, 1 << 32) * 16382 + 63) // 64
    per_request = 2 * n <= max_rows
    cb = max(1, min(need, resident))
    if not per_request:
        cb = max(1, min(cb, max_rows // 64))
    rows = 2 * n if per_request else cb * 64
    nb = (n + scan_block - 1) // scan_block
    pre = (8 * n + 7) & ~7
    total = pre + 8 * n + 8 * nb
    rows_off = (total + 8 + 15) & ~15
    return {"n": n, "mb": max(1, min((n + 255) // 256, cus * 8)), "cb": cb, "row_per_request": int(per_request),
            "rows": rows, "cnt": 0, "fail": 4 * n, "pre": pre, "bsum": pre + 8 * n, "total": total,
            "rows_off": rows_off, "edge_bytes": rows * ROW_BYTES, "bytes": rows_off + rows * ROW_BYTES}

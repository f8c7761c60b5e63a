"""Ranged writes of indexed members (include/pmc_codec.h "ranged writes"), stated in plain Python: when a member
can be rewritten by its chunks, which chunks a patch touches, which of them are decoded first, and the member that
comes out -- the old spans of the untouched chunks, fresh spans for the touched ones, the member index header with
every offset recomputed, and a trailer whose CRC-32 is folded from the chunk CRCs alone (crc32_combine).
csrc/pmc_plan.hpp patch_of / crc_fold_host / plan_patch are the same arithmetic (tests/test_host_patch.py),
csrc/pmc_deflate_patch.hip the same verdicts and bytes (tests/test_gpu_patch.py)."""
import zlib

from indexed_crc_model import header_crc, parse_chunk_crcs
from indexed_model import C, LOG2C, parse_index
from range_model import chunk_bytes, chunk_span

NO_INDEX, ARG = "no_index", "arg"   # PMC_E_NO_INDEX, PMC_E_ARG
POLY = 0xEDB88320

ROUND_CHUNKS = 8192                 # csrc/pmc_plan.hpp kPatchRoundChunks
SCRATCH_BUDGET = 2048 << 20         # kPatchScratchBudget
SLAB_BYTES = 65536
MAX_WAVES = 2048
SEGS = C // 2048


def multmodp(a: int, b: int) -> int:
    """a * b mod P in GF(2)[x], reflected (zlib's multmodp)."""
    p = 0
    for k in range(31, -1, -1):
        if (a >> k) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x8n(n: int) -> int:
    """x^(8 n) mod P."""
    r, sq = 0x80000000, 0x00800000
    while n:
        if n & 1:
            r = multmodp(sq, r)
        sq = multmodp(sq, sq)
        n >>= 1
    return r


def fold(crcs, isize: int, chunk=C) -> int:
    """The CRC-32 of a value of isize bytes from the CRC-32s of its chunks: crc = crc x^(8 clen) + crc_k."""
    crc = 0
    for k, e in enumerate(crcs):
        clen = min(chunk, isize - k * chunk)
        crc = multmodp(x8n(clen), crc) ^ e
    return crc


def patch_of(isize: int, lg: int, off: int, length: int):
    """(ok, a, b, items, edge_a, edge_b): csrc/pmc_plan.hpp patch_of."""
    if off + length > isize:
        return False, 0, 0, 0, False, False
    if length == 0:
        return True, 0, 0, 0, False, False
    ch = 1 << lg
    end = off + length
    a, b = off >> lg, (end - 1) >> lg
    be = min((b + 1) * ch, isize)
    head, tail = off % ch != 0, end != be
    return True, a, b, b - a + 1, head or (a == b and tail), a != b and tail


def member_check(m: bytes):
    """(K, crcs, isize) of a member the rewrite takes, or None: a valid index with this library's chunk size, chunk
    CRCs, and entries whose fold is the trailer's CRC-32."""
    m = bytes(m)
    idx = parse_index(m)
    if idx is None or idx[0] != C:
        return None
    crcs = parse_chunk_crcs(m)
    if crcs is None:
        return None
    isize = int.from_bytes(m[-4:], "little")
    if fold(crcs, isize) != int.from_bytes(m[-8:-4], "little"):
        return None
    return idx[1], crcs, isize


def old_span(m: bytes, k: int) -> bytes:
    start, nxt, _, _ = chunk_span(m, k)
    return m[start:nxt]


def rewrite(old_member: bytes, off: int, patch: bytes, fresh_span_of):
    """The member of V' = V with [off, off + len(patch)) replaced, NO_INDEX or ARG.  fresh_span_of(bytes, last): the
    compressed span of a chunk of those bytes (its blocks, and behind every chunk but the last the empty stored
    block).  Returns (member, counts) with counts = (decoded, compressed, copied) on success."""
    m = bytes(old_member)
    chk = member_check(m)
    if chk is None:
        return NO_INDEX, (0, 0, 0)
    K, crcs, isize = chk
    ok, a, b, items, edge_a, edge_b = patch_of(isize, LOG2C, off, len(patch))
    if not ok:
        return ARG, (0, 0, 0)
    if items == 0:
        return m, (0, 0, K)
    decoded = int(edge_a) + int(edge_b)
    new = {}
    for k in range(a, b + 1):
        c0 = k * C
        clen = min(C, isize - c0)
        lo, hi = max(c0, off), min(c0 + clen, off + len(patch))
        if (k == a and edge_a) or (k == b and k != a and edge_b):
            base = chunk_bytes(m, k)
            if base is None or zlib.crc32(base) != crcs[k]:
                return NO_INDEX, (decoded, 0, 0)
        else:
            assert (lo, hi) == (c0, c0 + clen)
            base = bytes(clen)
        new[k] = base[:lo - c0] + patch[lo - off:hi - off] + base[hi - c0:]
    spans = [fresh_span_of(new[k], k == K - 1) if k in new else old_span(m, k) for k in range(K)]
    entries = [zlib.crc32(new[k]) if k in new else crcs[k] for k in range(K)]
    hdr = 20 + 4 * (K - 1) + 8 + 4 * K
    offsets, at = [], hdr
    for s in spans[:-1]:
        at += len(s)
        offsets.append(at)
    out = (header_crc(isize, offsets, entries) + b"".join(spans) + fold(entries, isize).to_bytes(4, "little") +
           isize.to_bytes(4, "little"))
    return out, (decoded, items, K - items)


def fixed_span(tokens_of):
    """fresh_span_of for the fixed-block members of indexed_crc_model.assemble_crc."""
    import deflate_builder as B

    def span(part: bytes, last: bool) -> bytes:
        w = B.BitWriter()
        B.fixed_block(w, tokens_of(part), last)
        if not last:
            B.stored_block(w, b"", False)
        return w.getvalue()
    return span


def plan_patch(n: int, cus: int, scan_block: int = 1024):
    """csrc/pmc_plan.hpp plan_patch."""
    nb = (n + scan_block - 1) // scan_block
    roff = (28 * n + 7) & ~7
    return {"n": n, "mb": max(1, min((n + 255) // 256, cus * 8)), "cnt": 0, "ka": 4 * n, "fail": 8 * n, "pfail": 12 * n,
            "lv_val": 16 * n, "seg0": 20 * n, "rlen": 24 * n, "roff": roff, "pre": roff + 8 * n, "bsum": roff + 16 * n,
            "total": roff + 16 * n + 8 * nb, "bytes": roff + 16 * n + 8 * nb + 8}


def slot_bytes() -> int:
    bound = C + (C >> 3) + 6 * (C // 16383 + 1) + 32
    return (bound + 16 + 15) & ~15


def plan_patch_round(items: int, cus: int):
    """csrc/pmc_plan.hpp plan_patch_round."""
    items = max(1, items)
    waves = max(4, min((items + 3) // 4 * 4, cus * 8, MAX_WAVES))
    o = 0
    out = {"items": items, "waves": waves}
    for name, size in (("stage", items * C + 4096), ("tok", items * C * 4), ("seg_val", items * SEGS * 4),
                       ("seg_tok0", items * SEGS * 8), ("seg_tok", items * SEGS * 16), ("slots", items * slot_bytes()),
                       ("span", items * 4), ("crc", items * 4), ("slabs", waves * SLAB_BYTES)):
        out[name] = o
        o = (o + size + 255) & ~255
    out["bytes"] = o
    return out

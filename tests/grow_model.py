"""Growing writes of indexed members (include/pmc_codec.h "growing writes"), stated in plain Python from
tests/patch_model.py's pieces: a ranged write whose patch may reach past the value's end (APPEND, SETRANGE with zero
padding).  The old member's (S, K) governs what is read -- the member check, the spans and entries of the chunks
before the first touched one, the one edge chunk -- and the new value's (S', K') what is written.
csrc/pmc_plan.hpp grow_of is the same arithmetic (tests/test_host_grow.py), csrc/pmc_deflate_patch.hip the same
verdicts and bytes (tests/test_gpu_grow.py)."""
import zlib

from indexed_crc_model import header_crc
from indexed_model import C, LOG2C
from patch_model import ARG, NO_INDEX, fold, member_check, old_span, patch_of
from range_model import chunk_bytes

SERVE, SAME = "serve", "same"   # csrc/pmc_plan.hpp kGrowServe, kGrowSame (kGrowArg: ARG, kGrowNoIndex: NO_INDEX)
MAX_CHUNKS = 8190               # kIdxCrcMaxChunks


def grow_of(isize: int, lg: int, off: int, length: int):
    """(verdict, grows, S2, K2, a, b, items, edge_a, edge_b): csrc/pmc_plan.hpp grow_of."""
    ch = 1 << lg
    end = off + length
    K = (isize + ch - 1) >> lg
    if length == 0:
        return SAME, False, isize, K, 0, 0, 0, False, False
    if end <= isize:
        _, a, b, items, ea, eb = patch_of(isize, lg, off, length)
        return SERVE, False, isize, K, a, b, items, ea, eb
    if end > 0xFFFFFFFF:
        return ARG, True, isize, K, 0, 0, 0, False, False
    K2 = (end + ch - 1) >> lg
    if K2 > MAX_CHUNKS:
        return NO_INDEX, True, end, K2, 0, 0, 0, False, False
    a = min(off >> lg, K - 1) if K else off >> lg
    return SERVE, True, end, K2, a, K2 - 1, K2 - a, min(off, isize) > a * ch, False


def grown(value: bytes, off: int, patch: bytes) -> bytes:
    """V': V with [off, off + len(patch)) replaced, zeros between V's end and off; an empty patch changes nothing."""
    if not patch:
        return value
    return value[:off] + bytes(max(0, off - len(value))) + patch + value[off + len(patch):]


def grow(old_member: bytes, off: int, patch: bytes, fresh_span_of):
    """The member of V' = grown(V, off, patch), NO_INDEX or ARG.  fresh_span_of(bytes, last): as in
    patch_model.rewrite.  Returns (member, counts) with counts = (decoded, compressed, copied) on success."""
    m = bytes(old_member)
    chk = member_check(m)
    if chk is None:
        return NO_INDEX, (0, 0, 0)
    K, crcs, isize = chk
    verdict, _, S2, K2, a, b, items, edge_a, edge_b = grow_of(isize, LOG2C, off, len(patch))
    if verdict == SAME:
        return m, (0, 0, K)
    if verdict != SERVE:
        return verdict, (0, 0, 0)
    decoded = int(edge_a) + int(edge_b)
    end = off + len(patch)
    new = {}
    for k in range(a, b + 1):
        c0 = k * C
        clen = min(C, S2 - c0)
        if (k == a and edge_a) or (k == b and k != a and edge_b):
            base = chunk_bytes(m, k)                      # old geometry: chunk k of K, of the old length
            if base is None or zlib.crc32(base) != crcs[k]:
                return NO_INDEX, (decoded, 0, 0)
        else:
            base = b""
        base = (base + bytes(clen))[:clen]                # zeros behind the old end
        lo, hi = max(c0, off), min(c0 + clen, end)
        if hi > lo:
            base = base[:lo - c0] + patch[lo - off:hi - off] + base[hi - c0:]
        new[k] = base
    spans = [fresh_span_of(new[k], k == K2 - 1) if k in new else old_span(m, k) for k in range(K2)]
    entries = [zlib.crc32(new[k]) if k in new else crcs[k] for k in range(K2)]
    hdr = 20 + 4 * (K2 - 1) + 8 + 4 * K2
    offsets, at = [], hdr
    for s in spans[:-1]:
        at += len(s)
        offsets.append(at)
    out = (header_crc(S2, offsets, entries) + b"".join(spans) + fold(entries, S2).to_bytes(4, "little") +
           S2.to_bytes(4, "little"))
    return out, (decoded, items, K2 - items)

// pmc_inflate_chunk.hip -- chunk-parallel decoding of indexed members (include/pmc_codec.h "member index").
//
// An indexed member names, in its gzip FEXTRA field, the byte where each chunk of C value bytes begins;
// every chunk starts on a block header, is byte-aligned, and holds no distance that reaches before it.  So
// a large member has work to hand out: one LANE per (member, chunk), with the lane decoder's parts
// (pmc_inflate_lane.hip: LaneIn, LaneWin, LaneOut, LaneCode, lane_block, the multi-block layout).
//   inflate_chunk_scan_kernel   one thread per member: is it indexed, and how many chunks has it
//   (exclusive prefix sum of the counts: scan_u32, pmc_capi.hip)
//   inflate_chunk_kernel        one lane per chunk; a wave takes 64 consecutive items of the prefix array
//   inflate_chunk_finish_kernel one thread per member: rc, dst_len and the CRC-32 to verify
//   (inflate_verify_kernel, unchanged)
//   inflate_chunk_count_kernel  the context's two counters (pmc_ctx_index_counts)
// The index is advisory: whatever the scan does not take, a chunk that does not decode exactly as its index
// says, and a CRC mismatch all leave the member kInflateRetry, and the wave kernels decode it from its first
// byte with FLG.FEXTRA skipped.  A lane writes only its chunk's bytes of dst: within [0, ISIZE), which the
// scan checked against the capacity.
#include <hip/hip_runtime.h>

#include "pmc_device.hpp"
#include "pmc_kernels.hpp"

namespace pmc {

typedef LaneLayout<kLaneWideLit, true> ChunkLayout;
constexpr uint32_t kChunkLdsBytes = ChunkLayout::kLds;

__device__ __forceinline__ uint32_t idx_u32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// X.all (the wave-only route): every member is looked at, and one that is not taken is marked kInflateRetry
// for the wave kernels' retry_only mode.  Else only the members the lane passes left kInflateRetry.
__global__ void __launch_bounds__(256) inflate_chunk_scan_kernel(InflateArgs a, ChunkArgs X) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < a.n; v += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t K = 0;
        if (X.all || a.rc[v] == kInflateRetry) {
            uint32_t lg, k, isz, hdr;
            if (idx_parse(a.src + a.src_off[v], a.src_len[v], &lg, &k, &isz, &hdr) && isz <= a.dst_cap[v]) K = k;
            if (X.all) a.rc[v] = kInflateRetry;
        }
        X.cnt[v] = K;
        X.fail[v] = 0;
    }
}

// One lane decodes one chunk: the member m of in_len bytes from its byte `start`, exactly clen bytes to `out`,
// then what must follow -- the empty stored block that ends on byte `next` (the next chunk's index entry), or
// for the member's last chunk (lastc) the final block's end with the trailer at `next` = in_len - 8.  Called by
// all 64 lanes of a wave (the loop is wave-synchronous); st: 0 an item to decode, 3 none (m: any mapped byte,
// in_len 0).  Returns 8 (the chunk is complete, every byte of it in `out`), 2 (declined) or 3.  The lane
// kernel's decode loop with positions relative to the chunk: `d > o.pos` keeps a distance inside the chunk,
// the capacity tests keep the output inside [out, out + clen).
template <class LL>
__device__ __forceinline__ uint32_t chunk_decode(PMC_LDS uint16_t *col, PMC_LDS uint32_t *ring, PMC_LDS uint8_t *bcol,
                                                 PMC_LDS uint32_t *winw, uint32_t st, const uint8_t *m, uint32_t in_len,
                                                 uint32_t start, uint32_t next, uint32_t clen, bool lastc, uint8_t *out) {
    typedef typename LL::Cols Cols;
    LaneIn in;
    in.p = m;
    in.len = in_len;
    in.blk = (PMC_GLB const uint4 *)((uintptr_t)in.p & ~(uintptr_t)15);
    LaneCode<15> lit, dist;
    lit.base = (PMC_LDS int16_t *)(col + Cols::kColBaseL * 64);
    lit.sym = col + Cols::kColLit * 64;
    dist.base = (PMC_LDS int16_t *)(col + Cols::kColBaseD * 64);
    dist.sym = col + Cols::kColDist * 64;
    bool fixed = false;
    uint32_t blast = 0;
    if (st == 0) {
        in.seek((uint64_t)start * 8);
        blast = in.bits(1);
        bool ov = false;
        if (!lane_block<Cols>(in, col, bcol, lit, dist, fixed, &ov, kLaneWideLit, kLaneDistCap)) st = 2;
    }
    LaneWin win;
    win.w = winw;
    win.start(in, st == 0 ? in.bitpos() : 0);
    const uint32_t cap = st == 0 ? clen : 0u;
    LaneOut o;
    o.dst = (PMC_GLB uint8_t *)out;
    o.a0 = (uint32_t)((uintptr_t)o.dst & 3);
    o.dw = (PMC_GLB uint32_t *)((uintptr_t)o.dst & ~(uintptr_t)3);
    o.rw = ring;
    o.rb = (PMC_LDS uint8_t *)ring;
    o.pos = 0;
    o.flushed = 0;
    uint32_t rem = 0, md = 0; // pending match: bytes left, distance
    // st: 0 decoding, 1 the final block's end, 2 failed, 3 no item, 6 a block's end, 8 chunk complete
    while (ballot(st == 0)) {
        if (ballot(st == 0 && win.needs()))
            if (st == 0) win.advance();
        if (st == 0) {
            if (rem == 0) {
                win.refill();
                const uint32_t sy = fixed ? fixed_lit(win) : lit.decode(win);
                if (sy < 256) {
                    if (o.pos >= cap) {
                        st = 2;
                    } else {
                        o.put(o.pos++, sy);
                        uint32_t l2;
                        const uint32_t s2 = fixed ? fixed_peek(win, l2) : lit.peek_sym(win, l2);
                        if (s2 < 256 && o.pos < cap) {
                            win.drop(l2);
                            o.put(o.pos++, s2);
                            win.refill();
                            uint32_t l3;
                            const uint32_t s3 = fixed ? fixed_peek(win, l3) : lit.peek_sym(win, l3);
                            if (s3 < 256 && o.pos < cap) {
                                win.drop(l3);
                                o.put(o.pos++, s3);
                            }
                        }
                    }
                } else if (sy == 256) {
                    st = blast ? 1u : 6u;
                } else if (sy > 285) {
                    st = 2;
                } else {
                    const uint32_t li = sy - 257;
                    const uint32_t lx = li < 8 || li == 28 ? 0u : (li - 4) >> 2;
                    const uint32_t lb = li < 8 ? li + 3 : li == 28 ? 258u : ((4 + (li & 3)) << lx) + 3;
                    const uint32_t len = lb + win.bits(lx);
                    win.refill();
                    const uint32_t ds = fixed ? __builtin_bitreverse32(win.peek(5)) >> 27 : dist.decode(win);
                    if (fixed) win.drop(5);
                    const uint32_t dx = ds < 4 ? 0u : (ds >> 1) - 1;
                    const uint32_t db = ds < 4 ? ds + 1 : ((2 + (ds & 1)) << dx) + 1;
                    const uint32_t d = db + win.bits(dx < 14 ? dx : 0u);
                    if (ds > 29 || d > o.pos || o.pos + len > cap) {
                        st = 2;
                    } else if (d < 8) {
                        uint64_t pat = o.get8(o.pos - d, true) & ((1ull << (8 * d)) - 1);
                        for (uint32_t w = d; w < 8; w <<= 1) pat |= pat << (8 * w);
                        const uint32_t mm = len < 8 ? len : 8;
#pragma unroll
                        for (uint32_t j = 0; j < 8; j++)
                            if (j < mm) o.put(o.pos + j, (uint32_t)(pat >> (8 * j)));
                        o.pos += mm;
                        rem = len - mm;
                        md = d * ((8 + d - 1) / d);
                    } else {
                        rem = len;
                        md = d;
                    }
                }
            }
            if (st == 0 && rem) {
                const uint32_t mm = rem < 8 ? rem : 8;
                const uint64_t x = o.get8(o.pos - md, md <= kRing - 16);
#pragma unroll
                for (uint32_t j = 0; j < 8; j++)
                    if (j < mm) o.put(o.pos + j, (uint32_t)(x >> (8 * j)));
                o.pos += mm;
                rem -= mm;
            }
            if (st == 6) { // end of a block that is not final
                const uint64_t bp = win.bitpos();
                if (bp + 3 > (uint64_t)in_len * 8) {
                    st = 2;
                } else if (o.pos == clen && !lastc) {
                    // the chunk is complete: exactly the empty stored block must follow (bits 000, padding,
                    // 00 00 ff ff) and end on the byte the index names for the next chunk
                    in.seek(bp);
                    const uint32_t b3 = in.bits(3);
                    const uint32_t q = (uint32_t)((bp + 3 + 7) >> 3);
                    st = b3 == 0 && q + 4 == next && in.byte_at(q) == 0 && in.byte_at(q + 1) == 0 &&
                                 in.byte_at(q + 2) == 0xff && in.byte_at(q + 3) == 0xff
                             ? 8u
                             : 2u;
                } else { // the next block's header and tables
                    in.seek(bp);
                    blast = in.bits(1);
                    bool ov = false;
                    if (lane_block<Cols>(in, col, bcol, lit, dist, fixed, &ov, kLaneWideLit, kLaneDistCap)) {
                        win.start(in, in.bitpos());
                        st = 0;
                    } else {
                        st = 2; // stored blocks, longer lists, malformed codes: the wave kernels
                    }
                }
            }
        }
        if (ballot(st == 0 && o.pos - o.flushed >= kFlush))
            if (st == 0) o.flush(o.pos, false);
    }
    // the final block's end: only the last chunk's, with every byte of it produced and the trailer ending
    // the member
    if (st == 1) {
        const uint64_t bp = win.bitpos();
        st = lastc && o.pos == clen && bp <= (uint64_t)in_len * 8 && ((bp + 7) >> 3) == next ? 8u : 2u;
    }
    if (st == 8) o.flush(o.pos, true);
    return st;
}

__global__ void __launch_bounds__(64) inflate_chunk_kernel(InflateArgs a, ChunkArgs X) {
    typedef ChunkLayout LL;
    extern __shared__ __attribute__((aligned(16))) uint16_t lcol[];
    PMC_LDS uint16_t *col = to_lds<uint16_t>(lcol + threadIdx.x);
    PMC_LDS uint32_t *ring = to_lds<uint32_t>((uint8_t *)lcol + LL::kRingOff) + threadIdx.x;
    PMC_LDS uint8_t *bcol = to_lds<uint8_t>((uint8_t *)lcol + LL::kBColOff + threadIdx.x);
    PMC_LDS uint32_t *winw = to_lds<uint32_t>((uint8_t *)lcol + LL::kWinOff) + threadIdx.x;
    const uint64_t total = *X.total;
    for (uint64_t ib = (uint64_t)blockIdx.x * 64; ib < total; ib += (uint64_t)gridDim.x * 64) {
        const uint64_t it = ib + threadIdx.x;
        uint32_t st = it < total ? 0u : 3u; // (chunk_decode: 0 an item, 3 none)
        // the item's member: the last one whose prefix is <= it (members of no chunks share their successor's)
        uint64_t v = 0;
        if (st == 0) {
            uint64_t lo = 0, hi = a.n - 1;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if (X.pre[mid] <= it) lo = mid;
                else hi = mid - 1;
            }
            v = lo;
        }
        const uint32_t k = st == 0 ? (uint32_t)(it - X.pre[v]) : 0u;
        const uint32_t K = st == 0 ? X.cnt[v] : 0u;
        const uint8_t *m = st == 0 ? a.src + a.src_off[v] : a.src;
        const uint32_t in_len = st == 0 ? a.src_len[v] : 0u;
        uint32_t lg = 12, start = 0, next = 0, clen = 0;
        bool lastc = true;
        if (st == 0) {
            lg = m[17];
            const uint32_t isz = idx_u32(m + in_len - 4);
            const uint32_t xlen = (uint32_t)m[10] | (uint32_t)m[11] << 8;
            start = k == 0 ? 12 + xlen : idx_u32(m + kIdxHdrFixed + 4 * (k - 1));
            lastc = k + 1 == K;
            next = lastc ? in_len - 8 : idx_u32(m + kIdxHdrFixed + 4 * k);
            const uint64_t c0 = (uint64_t)k << lg;
            clen = (uint32_t)(isz - c0 < (1ull << lg) ? isz - c0 : (1ull << lg));
        }
        st = chunk_decode<LL>(col, ring, bcol, winw, st, m, in_len, start, next, clen, lastc,
                              st == 0 ? a.dst + a.dst_off[v] + ((uint64_t)k << lg) : a.dst);
        if (st == 2) X.fail[v] = 1;
    }
}

__global__ void __launch_bounds__(256) inflate_chunk_finish_kernel(InflateArgs a, ChunkArgs X) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < a.n; v += (uint64_t)gridDim.x * blockDim.x) {
        if (X.cnt[v] == 0 || X.fail[v]) continue; // (a failed member stays kInflateRetry)
        const uint8_t *t = a.src + a.src_off[v] + a.src_len[v] - 8;
        a.crc_expect[v] = idx_u32(t);
        a.dst_len[v] = idx_u32(t + 4);
        a.rc[v] = 0;
    }
}

// after inflate_verify_kernel: X.counts[0] += members the chunk pass completed, [1] += members it took and
// then left to the wave kernels (a failed chunk, a CRC mismatch)
__global__ void __launch_bounds__(256) inflate_chunk_count_kernel(InflateArgs a, ChunkArgs X) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < a.n; v += (uint64_t)gridDim.x * blockDim.x) {
        if (X.cnt[v] == 0) continue;
        atomicAdd((unsigned long long *)&X.counts[a.rc[v] == 0 ? 0 : 1], 1ull);
    }
}

} // namespace pmc

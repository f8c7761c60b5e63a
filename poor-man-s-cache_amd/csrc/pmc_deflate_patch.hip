// pmc_deflate_patch.hip -- ranged and growing writes of indexed members (include/pmc_codec.h "ranged writes",
// "growing writes").
//
// An indexed member with chunk CRCs can be rewritten chunk by chunk: the chunks a patch does not touch keep their
// compressed spans (they start on the bytes the index names), the touched ones are compressed again alone (a
// chunk's tokens depend on its bytes only), and the member's CRC-32 is folded from the chunk CRCs, so no untouched
// byte of the value is read.
//   patch_scan_kernel     one thread per request: the member check (index, chunk size, chunk CRCs, the fold of the
//                         entries against the trailer), the bounds, and the number of touched chunks
//   (exclusive prefix sum of the counts: scan_u32, pmc_capi.hip; the host reads the total and cuts the requests
//   into rounds, pmc_plan.hpp plan_patch_round)
//   patch_tables_kernel   the round's regions (a request's touched chunks, contiguous in the stage) as the "values"
//                         of lv_fast_parse_kernel, and its segment tables
//   patch_decode_kernel   one lane per edge chunk (a chunk the patch covers in part; at most two per request):
//                         chunk_decode into the chunk's place in the stage, then its CRC-32 against its entry
//                         (range_crc32, the whole wave on one chunk) -- inflate_range_kernel<true>'s method
//   patch_overlay_kernel  one block per touched chunk: the patch's bytes over the stage
//   (lv_fast_parse_kernel, unchanged: the history rule stops at a chunk's first byte in a region as in a value)
//   patch_emit_kernel     one wave per touched chunk: the blocks of its tokens with DeflateWave::flush_block, as
//                         run_lv writes them at the chunk's place in a value of S bytes, into the chunk's slot
//   patch_finish_kernel   one wave per request: verdict, the new offsets (a prefix sum over the K span lengths), the
//                         header with every offset and CRC entry, the fold, the trailer, the counters
//   patch_copy_kernel     one block per (request, chunk): the span from the old member or from the slot to its
//                         place -- dword stores through alignbyte, plain vector stores only
// A write may make the value longer (PatchArgs::grow; without it the scan refuses growth).  Two geometries are then
// kept apart: the old member's (S, K) for everything that is read -- the member check, the untouched spans and
// entries, the edge decode -- and the new value's (S2, K2) (pmc_plan.hpp grow_of) for everything that is written:
// the regions, the overlay with its zero gap [S, range_off), the emit's chunk lengths, last chunk and window
// arithmetic, the header, the fold, the trailer and the copy.  Where the value does not grow the two are the same.
#include <hip/hip_runtime.h>

#include "pmc_device.hpp"
#include "pmc_kernels.hpp"

namespace pmc {

constexpr uint32_t kPatchLg = 31 - __builtin_clz(kIdxChunk);
static_assert(kPatchSlabBytes == (uint64_t)kSlabSyms * 4, "the emit's symbol slab");
static_assert(kPatchSlotBytes % 16 == 0, "slots keep the stage's alignment");

// the facts of a member that passed the scan (no test repeated): S = ISIZE, K chunks, the header's end and the
// first CRC entry
struct PatchMember {
    uint32_t S, K, hdr, crc_at;
};
__device__ __forceinline__ PatchMember patch_member(const uint8_t *m, uint32_t len) {
    PatchMember M;
    M.S = idx_u32(m + len - 4);
    M.K = (uint32_t)(((uint64_t)M.S + kIdxChunk - 1) >> kPatchLg);
    M.hdr = 12 + ((uint32_t)m[10] | (uint32_t)m[11] << 8);
    M.crc_at = 16 + 4 * M.K + kIdxCrcFixed;
    return M;
}
// chunk k's span in the old member: [start, end) -- its blocks and, for every chunk but the last, the separator
__device__ __forceinline__ uint32_t patch_old_start(const uint8_t *m, const PatchMember &M, uint32_t k) {
    return k == 0 ? M.hdr : idx_u32(m + kIdxHdrFixed + 4 * (k - 1));
}
__device__ __forceinline__ uint32_t patch_old_end(const uint8_t *m, uint32_t len, const PatchMember &M, uint32_t k) {
    return k + 1 == M.K ? len - 8 : idx_u32(m + kIdxHdrFixed + 4 * k);
}
__device__ __forceinline__ uint32_t patch_clen(uint32_t S, uint32_t k) {
    const uint32_t c0 = k << kPatchLg;
    return S - c0 < kIdxChunk ? S - c0 : kIdxChunk;
}
// the new value's length for a request the scan took with touched chunks (cnt != 0: the scan has checked the sum)
__device__ __forceinline__ uint32_t patch_new_size(uint32_t S, uint32_t off, uint32_t len) {
    return off + len > S ? off + len : S;
}
__device__ __forceinline__ uint32_t patch_chunks(uint32_t S) {
    return (uint32_t)(((uint64_t)S + kIdxChunk - 1) >> kPatchLg);
}
// x^(8 clen) mod P: what a chunk of clen bytes shifts the CRC register by (run_lv's recurrence)
__device__ __forceinline__ uint32_t patch_shift(uint32_t clen) {
    constexpr CrcX8 kX8 = make_crc_x8();
    return multmodp(crc_shift_chunks(clen >> 4), kX8.v[clen & 15]);
}
// the request of the round's chunk item `it` (absolute): the last one of v0 .. v1 - 1 whose prefix is <= it
__device__ __forceinline__ uint32_t patch_request(const PatchArgs &P, uint64_t it) {
    uint32_t lo = P.v0, hi = P.v1 - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (P.pre[mid] <= it) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// n bytes from src to dst by the nt threads of a block (t: this thread), any alignment of either: the head bytes up
// to dst's next dword, whole dwords assembled from the two aligned source words that hold them (the second is read
// only where it holds a byte of src), the tail bytes
__device__ __forceinline__ void patch_block_copy(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t t, uint32_t nt) {
    PMC_GLB uint8_t *d = (PMC_GLB uint8_t *)dst;
    PMC_GLB const uint8_t *s = (PMC_GLB const uint8_t *)src;
    uint64_t head = (4 - ((uintptr_t)d & 3)) & 3;
    head = head < n ? head : n;
    for (uint64_t j = t; j < head; j += nt) d[j] = s[j];
    d += head;
    s += head;
    n -= head;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
    PMC_GLB const uint32_t *sw = (PMC_GLB const uint32_t *)((uintptr_t)s - sh);
    PMC_GLB uint32_t *dw = (PMC_GLB uint32_t *)d;
    const uint64_t nw = n >> 2;
    for (uint64_t j = t; j < nw; j += nt) {
        const uint32_t w0 = sw[j], w1 = sh ? sw[j + 1] : 0u;
        dw[j] = __builtin_amdgcn_alignbyte(w1, w0, sh);
    }
    for (uint64_t j = nw * 4 + t; j < n; j += nt) d[j] = s[j];
}

// n zero bytes at dst, the same way
__device__ __forceinline__ void patch_block_zero(uint8_t *dst, uint64_t n, uint32_t t, uint32_t nt) {
    PMC_GLB uint8_t *d = (PMC_GLB uint8_t *)dst;
    uint64_t head = (4 - ((uintptr_t)d & 3)) & 3;
    head = head < n ? head : n;
    for (uint64_t j = t; j < head; j += nt) d[j] = 0;
    d += head;
    n -= head;
    PMC_GLB uint32_t *dw = (PMC_GLB uint32_t *)d;
    const uint64_t nw = n >> 2;
    for (uint64_t j = t; j < nw; j += nt) dw[j] = 0u;
    for (uint64_t j = nw * 4 + t; j < n; j += nt) d[j] = 0;
}

__global__ void __launch_bounds__(256) patch_scan_kernel(PatchArgs P) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < P.n; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t *m = P.src + P.src_off[v];
        const uint32_t len = P.src_len[v];
        uint32_t lg, K, S, hdr, at, cnt = 0, ka = 0;
        int32_t rc = PMC_E_NO_INDEX;
        if (!P.off && idx_parse(m, len, &lg, &K, &S, &hdr) && lg == kPatchLg && idx_crc_sub(m, K, hdr, &at)) {
            // the fold of the K entries (run_lv's recurrence) against the trailer's CRC-32
            const uint32_t xc = patch_shift(kIdxChunk);
            uint32_t crc = 0;
            for (uint32_t k = 0; k < K; k++) {
                const uint32_t clen = patch_clen(S, k);
                crc = multmodp(clen == kIdxChunk ? xc : patch_shift(clen), crc) ^ idx_u32(m + at + 4 * k);
            }
            if (crc == idx_u32(m + len - 8)) {
                const GrowOf g = grow_of(S, kPatchLg, P.range_off[v], P.patch_len[v]);
                // (a rewrite refuses what reaches past the end, an empty patch behind it too)
                if ((!P.grow && (uint64_t)P.range_off[v] + P.patch_len[v] > S) || g.verdict == kGrowArg) {
                    rc = PMC_E_ARG_DEV;
                } else if (g.verdict != kGrowNoIndex) { // (until the finish kernel: pending)
                    rc = kDeflateRetry;
                    cnt = g.items;
                    ka = g.a;
                }
            }
        }
        P.cnt[v] = cnt;
        P.ka[v] = ka;
        P.fail[v] = 0;
        P.pfail[v] = 0;
        P.rc[v] = rc;
        P.dst_len[v] = 0;
    }
}

__global__ void __launch_bounds__(256) patch_tables_kernel(PatchArgs P) {
    const uint64_t nr = P.v1 - P.v0, nt = nr > P.items ? nr : P.items;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += (uint64_t)gridDim.x * blockDim.x) {
        if (t < nr) {
            const uint32_t v = P.v0 + (uint32_t)t, cnt = P.cnt[v];
            const uint64_t it = P.pre[v] - P.i0;
            uint32_t rlen = 0;
            if (cnt) {
                const uint32_t S = patch_new_size(idx_u32(P.src + P.src_off[v] + P.src_len[v] - 4), P.range_off[v],
                                                  P.patch_len[v]);
                const uint64_t c0 = (uint64_t)P.ka[v] << kPatchLg, e = c0 + (uint64_t)cnt * kIdxChunk;
                rlen = (uint32_t)((e < S ? e : S) - c0);
            }
            P.lv_val[v] = v;
            P.seg0[v] = (uint32_t)(it * kPatchSegs);
            P.roff[v] = it * kIdxChunk;
            P.rlen[v] = rlen;
        }
        if (t < P.items) {
            const uint32_t v = patch_request(P, P.i0 + t);
            for (uint32_t s = 0; s < kPatchSegs; s++) {
                P.seg_val[t * kPatchSegs + s] = v;
                P.seg_tok0[t * kPatchSegs + s] = (t * kPatchSegs + s) * (uint64_t)kIdxSeg;
            }
        }
    }
}

uint32_t patch_decode_lds() { return kRangeLdsBytes; }

__global__ void __launch_bounds__(64) patch_decode_kernel(PatchArgs P) {
    typedef ChunkLayout LL;
    extern __shared__ __attribute__((aligned(16))) uint16_t lcol[];
    PMC_LDS uint16_t *col = to_lds<uint16_t>(lcol + threadIdx.x);
    PMC_LDS uint32_t *ring = to_lds<uint32_t>((uint8_t *)lcol + LL::kRingOff) + threadIdx.x;
    PMC_LDS uint8_t *bcol = to_lds<uint8_t>((uint8_t *)lcol + LL::kBColOff + threadIdx.x);
    PMC_LDS uint32_t *winw = to_lds<uint32_t>((uint8_t *)lcol + LL::kWinOff) + threadIdx.x;
    PMC_LDS uint32_t *s4 = to_lds<uint32_t>((uint8_t *)lcol + kRangeCrcTabOff);
    bool s4_ready = false;
    uint32_t ndec = 0;
    const uint64_t total = 2ull * (P.v1 - P.v0); // lane 2 t + e: edge e of the round's request t
    for (uint64_t ib = (uint64_t)blockIdx.x * 64; ib < total; ib += (uint64_t)gridDim.x * 64) {
        const uint64_t it = ib + threadIdx.x;
        uint32_t st = it < total ? 0u : 3u; // (chunk_decode: 0 an item, 3 none)
        const uint32_t v = st == 0 ? P.v0 + (uint32_t)(it >> 1) : P.v0;
        const uint8_t *m = P.src;
        uint32_t in_len = 0, start = 0, next = 0, clen = 0, want = 0;
        bool lastc = true;
        uint8_t *out = P.stage;
        if (st == 0 && P.cnt[v] == 0) st = 3;
        if (st == 0) {
            const uint8_t *mm = P.src + P.src_off[v];
            const uint32_t len = P.src_len[v];
            const PatchMember M = patch_member(mm, len);
            // (old geometry throughout: a growing write has edge a only, and the old last chunk is decoded as the
            // last one, to the trailer)
            const GrowOf p = grow_of(M.S, kPatchLg, P.range_off[v], P.patch_len[v]);
            if ((it & 1) ? !p.edge_b : !p.edge_a) {
                st = 3;
            } else {
                const uint32_t k = (it & 1) ? p.b : p.a;
                m = mm;
                in_len = len;
                start = patch_old_start(m, M, k);
                next = patch_old_end(m, len, M, k);
                lastc = k + 1 == M.K;
                clen = patch_clen(M.S, k);
                want = idx_u32(m + M.crc_at + 4 * k);
                out = P.stage + (P.pre[v] - P.i0 + (k - p.a)) * kIdxChunk;
                ndec++;
            }
        }
        st = chunk_decode<LL>(col, ring, bcol, winw, st, m, in_len, start, next, clen, lastc, out);
        if (st == 2) P.fail[v] = 1u;
        // the chunk's CRC-32 against its entry while the bytes are there, by the whole wave, one chunk at a time
        const bool vfy = st == 8;
        uint64_t vm = ballot(vfy);
        if (vm) {
            if (!s4_ready) {
                for (uint32_t j = threadIdx.x; j < 4 * 256; j += 64) s4[j] = c_crc_slice8[j];
                s4_ready = true;
            }
            wave_sync_global(); // the lanes' stores of their chunks visible to the wave (and the tables)
            const uint64_t cp = (uint64_t)(uintptr_t)out;
            bool bad = false;
            while (vm) {
                const int j = __builtin_ctzll(vm);
                vm &= vm - 1;
                const uint32_t got = range_crc32((const uint8_t *)(uintptr_t)readlane64(cp, j), readlane(clen, j), s4);
                if ((int)threadIdx.x == j) bad = got != want;
            }
            if (vfy && bad) P.fail[v] = 1u;
        }
    }
    ndec = wave_sum_u32(ndec);
    if (threadIdx.x == 0 && ndec) atomicAdd((unsigned long long *)&P.counts[2], (unsigned long long)ndec);
}

__global__ void __launch_bounds__(256) patch_overlay_kernel(PatchArgs P) {
    for (uint64_t t = blockIdx.x; t < P.items; t += gridDim.x) {
        const uint32_t v = patch_request(P, P.i0 + t);
        const uint32_t k = P.ka[v] + (uint32_t)(P.i0 + t - P.pre[v]);
        const uint32_t S = idx_u32(P.src + P.src_off[v] + P.src_len[v] - 4);
        const uint32_t S2 = patch_new_size(S, P.range_off[v], P.patch_len[v]);
        const uint64_t c0 = (uint64_t)k << kPatchLg, ce = c0 + patch_clen(S2, k);
        const uint64_t o = P.range_off[v], e = o + P.patch_len[v];
        // the chunk's part of the gap between the old end and the patch: zeros (the stage is reused scratch, and the
        // decode of the old last chunk ends at the old end)
        const uint64_t zlo = c0 > S ? c0 : S, zhi = ce < o ? ce : o;
        if (zhi > zlo) patch_block_zero(P.stage + t * kIdxChunk + (zlo - c0), zhi - zlo, threadIdx.x, blockDim.x);
        const uint64_t lo = c0 > o ? c0 : o, hi = ce < e ? ce : e; // the chunk's part of the patch
        if (hi > lo)
            patch_block_copy(P.stage + t * kIdxChunk + (lo - c0), P.patch + P.patch_off[v] + (lo - o), hi - lo,
                             threadIdx.x, blockDim.x);
    }
}

// One chunk's tokens as blocks into the wave's image, from bit 0: run_lv's loop for the chunk at value bytes
// [c0, c0 + clen) of a value of S bytes.  Positions are relative to the chunk (W.b is the chunk's first byte); the
// window base is computed from the absolute ones, as run_lv computes it, and made relative.  A chunk's last block
// ends with its last token; the last chunk's is the final one (no empty block after a 16383rd symbol); every other
// chunk is followed by the empty stored block.  Returns the span's bytes, 0 when the tokens do not cover the chunk.
__device__ uint32_t patch_emit_chunk(DeflateWave<true> &W, uint32_t clen, uint64_t c0, uint64_t S, bool lastc,
                                     const PatchArgs &P, uint64_t sg0, PMC_LDS uint32_t *hist) {
    const int l = lane_id();
    const Tables &T = c_tables;
    for (uint64_t k = l; k < W.out_words; k += 64) W.outw[k] = 0;
    for (int k = l; k < 320; k += 64) hist[k] = 0;
    W.sync();
    uint64_t bitpos = 0, pos = 0, block_start = 0, last_start = 0;
    uint32_t ntok = 0;
    auto flush = [&](bool last) {
        for (int s = l; s < kLCodes; s += 64) W.tr->ltree[s].fc = (uint16_t)(s == kEndBlock ? 1u : hist[s]);
        if (l < kDCodes) W.tr->dtree[l].fc = (uint16_t)hist[kLCodes + l];
        if (l < kBLCodes) W.tr->bltree[l].fc = 0;
        W.sync();
        const uint64_t t = last ? S : c0 + last_start + 1;
        uint64_t B = 0;
        for (;;) {
            const uint64_t wend = S < B + 2 * kWSize ? S : B + 2 * kWSize;
            if (t - B >= kWSize + kMaxDist && t + kMinLookahead > wend) B += kWSize;
            else break;
        }
        wave_sync_global(); // slab stores visible to the emitting lanes
        bitpos = W.flush_block<1>(ntok, block_start, pos, B > c0 ? B - c0 : 0, last, bitpos);
        block_start = pos;
        ntok = 0;
        for (int k = l; k < 320; k += 64) hist[k] = 0;
        W.sync();
    };
    const uint32_t nseg = (clen + kIdxSeg - 1) / kIdxSeg;
    for (uint32_t s = 0; s < nseg; s++) {
        const uint64_t sg = sg0 + s;
        const uint32_t *tk = P.tok + P.seg_tok0[sg];
        uint32_t t = P.seg_tok[sg * 4 + 1];
        const uint32_t te = P.seg_tok[sg * 4 + 2];
        while (t < te) {
            uint32_t take = te - t < 64 ? te - t : 64;
            take = take < kSymsPerBlock - ntok ? take : kSymsPerBlock - ntok;
            const bool in = (uint32_t)l < take;
            const uint32_t x = in ? tk[t + l] : 0u, dist = x >> 16, lc = x & 0xff;
            if (in) {
                W.tok[ntok + l] = x;
                if (dist) {
                    lds_add(&hist[T.length_code[lc] + kLiterals + 1], 1u);
                    lds_add(&hist[kLCodes + d_code(T, dist - 1)], 1u);
                } else {
                    lds_add(&hist[lc], 1u);
                }
            }
            const uint32_t tl = in ? (dist ? lc + kMinMatch : 1u) : 0u;
            const uint32_t incl = wave_incl_scan_dpp(tl);
            last_start = pos + readlane(incl - tl, (int)take - 1);
            pos += readlane(incl, 63);
            ntok += take;
            t += take;
            const bool tail = lastc && pos == clen; // (the value's last token ends the final block)
            if (ntok == kSymsPerBlock && !tail) flush(false);
        }
    }
    if (lastc) {
        flush(true);
    } else {
        if (ntok) flush(false);
        const uint64_t o = (bitpos + 3 + 7) >> 3; // bits 000 (zero in the image), padding, 00 00 ff ff
        if (l < 4) W.outb[o + l] = l < 2 ? (uint8_t)0 : (uint8_t)0xff;
        bitpos = (o + 4) * 8;
        W.sync();
    }
    return pos == clen ? (uint32_t)(bitpos >> 3) : 0u;
}

uint64_t patch_emit_lds(int waves) { return 1024 + (uint64_t)waves * kLvEmitLdsPerWave; }
static_assert(1024 + 4 * kLvEmitLdsPerWave <= 160u * 1024, "patch_emit_kernel: four waves' trees and histograms");

__global__ void __launch_bounds__(256) patch_emit_kernel(PatchArgs P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t *crc_tab = reinterpret_cast<uint32_t *>(lds);
    for (int k = threadIdx.x; k < 256; k += blockDim.x) crc_tab[k] = c_crc_table[k];
    __syncthreads();
    const int wpb = blockDim.x / 64, wib = threadIdx.x / 64, l = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * wpb + wib, nwaves = (uint64_t)gridDim.x * wpb;
    uint8_t *wl = lds + 1024 + (uint64_t)wib * kLvEmitLdsPerWave;
    DeflateWave<true> W;
    W.tr = reinterpret_cast<Trees *>(wl);
    W.out_words = kPatchSlotBytes / 4;
    W.tok = reinterpret_cast<uint32_t *>(P.slabs + wave * kPatchSlabBytes);
    W.crc_tab = crc_tab;
    for (int k = 0; k < 8; k++) W.st[k] = 0;
    PMC_LDS uint32_t *hist = to_lds<uint32_t>(wl + kLvTreesBytes);
    for (uint64_t t = wave; t < P.items; t += nwaves) {
        const uint32_t v = patch_request(P, P.i0 + t);
        uint32_t span = 0;
        if (!P.fail[v] && !P.pfail[v]) { // (set by kernels that have run: uniform over the wave)
            const uint32_t k = P.ka[v] + (uint32_t)(P.i0 + t - P.pre[v]);
            const uint8_t *m = P.src + P.src_off[v];
            const PatchMember M = patch_member(m, P.src_len[v]);
            const uint32_t S2 = patch_new_size(M.S, P.range_off[v], P.patch_len[v]);
            const uint32_t clen = patch_clen(S2, k);
            W.b = P.stage + t * kIdxChunk;
            W.bw = reinterpret_cast<uint32_t *>(W.b);
            W.outb = P.slots + t * kPatchSlotBytes;
            W.outw = reinterpret_cast<uint32_t *>(W.outb);
            const uint32_t crc = wave_crc32(W.b, clen, crc_tab);
            span = patch_emit_chunk(W, clen, (uint64_t)k << kPatchLg, S2, k + 1 == patch_chunks(S2), P, t * kPatchSegs,
                                    hist);
            if (l == 0) P.crc[t] = crc;
        }
        if (l == 0) {
            P.span[t] = span;
            if (!span) P.fail[v] = 1u;
        }
    }
}

__device__ __forceinline__ void patch_put_u32(uint8_t *d, uint32_t x) {
    d[0] = (uint8_t)x;
    d[1] = (uint8_t)(x >> 8);
    d[2] = (uint8_t)(x >> 16);
    d[3] = (uint8_t)(x >> 24);
}

__global__ void __launch_bounds__(256) patch_finish_kernel(PatchArgs P) {
    const int wpb = blockDim.x / 64, wib = threadIdx.x / 64, l = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * wpb + wib, nwaves = (uint64_t)gridDim.x * wpb;
    uint64_t served = 0, declined = 0, compressed = 0, copied = 0; // (lane 0's)
    for (uint64_t v = P.v0 + wave; v < P.v1; v += nwaves) {
        int32_t rc = P.rc[v];
        if (rc != kDeflateRetry) { // answered by the scan
            declined += rc == PMC_E_NO_INDEX ? 1 : 0;
            continue;
        }
        const uint32_t cnt = P.cnt[v], ka = P.ka[v], len = P.src_len[v], cap = P.dst_cap[v];
        const uint8_t *m = P.src + P.src_off[v];
        uint8_t *d = P.dst + P.dst_off[v];
        const PatchMember M = patch_member(m, len);
        uint32_t need = 0, S2 = M.S, K2 = M.K;
        if (P.fail[v] || P.pfail[v]) {
            rc = PMC_E_NO_INDEX;
        } else if (cnt == 0) { // an empty patch: the member as it is (patch_copy_kernel)
            need = len;
            rc = need > cap ? PMC_E_CAPACITY_DEV : PMC_OK;
        } else {
            // the new value's S2 bytes in K2 chunks.  An untouched chunk lies before the patch or, where the value
            // keeps its length, behind it: the old last chunk's span is never carried into a longer value
            S2 = patch_new_size(M.S, P.range_off[v], P.patch_len[v]);
            K2 = patch_chunks(S2);
            const IdxPlan ix = idx_plan(S2, kIdxChunk, true);
            const uint64_t it0 = P.pre[v] - P.i0;
            const uint32_t xc = patch_shift(kIdxChunk);
            // first pass: the spans' sum and the fold of the entries
            uint64_t sum = 0;
            uint32_t crc = 0;
            for (uint32_t kb = 0; kb < K2; kb += 64) {
                const uint32_t k = kb + l;
                uint32_t sp = 0, e = 0;
                if (k < K2) {
                    const bool touched = k >= ka && k < ka + cnt;
                    sp = touched ? P.span[it0 + (k - ka)] : patch_old_end(m, len, M, k) - patch_old_start(m, M, k);
                    e = touched ? P.crc[it0 + (k - ka)] : idx_u32(m + M.crc_at + 4 * k);
                }
                sum += wave_sum_u32(sp);
                const uint32_t nk = K2 - kb < 64 ? K2 - kb : 64;
                for (uint32_t j = 0; j < nk; j++) {
                    const uint32_t clen = patch_clen(S2, kb + j);
                    crc = multmodp(clen == kIdxChunk ? xc : patch_shift(clen), crc) ^ readlane(e, (int)j);
                }
            }
            const uint64_t need64 = (uint64_t)ix.hdr + sum + 8;
            need = (uint32_t)need64;
            rc = need64 > cap ? PMC_E_CAPACITY_DEV : PMC_OK;
            if (rc == PMC_OK) {
                // second pass: header, offsets, entries, trailer (byte stores: d has any alignment)
                if (l < 10) {
                    const uint8_t hdr[10] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 4, 3};
                    d[l] = hdr[l];
                } else if (l < 20) {
                    const uint64_t xlen = ix.hdr - 12, sl = 4 * (uint64_t)ix.K;
                    const uint64_t ext = xlen | (uint64_t)'P' << 16 | (uint64_t)'I' << 24 | sl << 32 | 1ull << 48 |
                                         (uint64_t)kPatchLg << 56;
                    d[l] = l < 18 ? (uint8_t)(ext >> (8 * (l - 10))) : (uint8_t)0;
                } else if (l < 28) {
                    const uint64_t ext = (uint64_t)'P' | (uint64_t)'C' << 8 | (uint64_t)(4 + 4 * ix.K) << 16 | 1ull << 32;
                    d[ix.crc_at - kIdxCrcFixed + (l - 20)] = (uint8_t)(ext >> (8 * (l - 20)));
                } else if (l < 36) {
                    const uint32_t x = l < 32 ? crc : S2;
                    d[need - 8 + (l - 28)] = (uint8_t)(x >> (8 * (l & 3)));
                }
                uint64_t run = ix.hdr;
                for (uint32_t kb = 0; kb < K2; kb += 64) {
                    const uint32_t k = kb + l;
                    uint32_t sp = 0, e = 0;
                    if (k < K2) {
                        const bool touched = k >= ka && k < ka + cnt;
                        sp = touched ? P.span[it0 + (k - ka)] : patch_old_end(m, len, M, k) - patch_old_start(m, M, k);
                        e = touched ? P.crc[it0 + (k - ka)] : idx_u32(m + M.crc_at + 4 * k);
                    }
                    const uint32_t incl = wave_incl_scan_dpp(sp);
                    if (k < K2) {
                        if (k) patch_put_u32(d + kIdxHdrFixed + 4 * (k - 1), (uint32_t)(run + incl - sp));
                        patch_put_u32(d + ix.crc_at + 4 * k, e);
                    }
                    run += readlane(incl, 63);
                }
            }
        }
        if (l == 0) {
            P.rc[v] = rc;
            P.dst_len[v] = rc == PMC_OK || rc == PMC_E_CAPACITY_DEV ? need : 0u;
            served += rc == PMC_OK ? 1 : 0;
            declined += rc == PMC_E_NO_INDEX ? 1 : 0;
            if (rc == PMC_OK) {
                compressed += cnt;
                copied += K2 - cnt;
            }
        }
    }
    if (l == 0) {
        if (served) atomicAdd((unsigned long long *)&P.counts[0], (unsigned long long)served);
        if (declined) atomicAdd((unsigned long long *)&P.counts[1], (unsigned long long)declined);
        if (compressed) atomicAdd((unsigned long long *)&P.counts[3], (unsigned long long)compressed);
        if (copied) atomicAdd((unsigned long long *)&P.counts[4], (unsigned long long)copied);
    }
}

// blockIdx.x strides over the round's requests, blockIdx.y over a request's chunks
__global__ void __launch_bounds__(256) patch_copy_kernel(PatchArgs P) {
    for (uint64_t v = P.v0 + blockIdx.x; v < P.v1; v += gridDim.x) {
        if (P.rc[v] != PMC_OK) continue;
        const uint32_t cnt = P.cnt[v], ka = P.ka[v], len = P.src_len[v];
        const uint8_t *m = P.src + P.src_off[v];
        uint8_t *d = P.dst + P.dst_off[v];
        if (cnt == 0) {
            if (blockIdx.y == 0) patch_block_copy(d, m, len, threadIdx.x, blockDim.x);
            continue;
        }
        const PatchMember M = patch_member(m, len);
        const uint32_t S2 = patch_new_size(M.S, P.range_off[v], P.patch_len[v]);
        const uint32_t hdrn = idx_plan(S2, kIdxChunk, true).hdr;
        const uint64_t it0 = P.pre[v] - P.i0;
        for (uint32_t k = blockIdx.y; k < patch_chunks(S2); k += gridDim.y) {
            const bool touched = k >= ka && k < ka + cnt;
            const uint32_t os = touched ? 0u : patch_old_start(m, M, k); // (the old member has no chunk k >= K)
            const uint8_t *s = touched ? P.slots + (it0 + (k - ka)) * kPatchSlotBytes : m + os;
            const uint32_t nb = touched ? P.span[it0 + (k - ka)] : patch_old_end(m, len, M, k) - os;
            // (the new offsets are in the header the finish kernel wrote)
            const uint32_t at = k ? idx_u32(d + kIdxHdrFixed + 4 * (k - 1)) : hdrn;
            patch_block_copy(d + at, s, nb, threadIdx.x, blockDim.x);
        }
    }
}

} // namespace pmc

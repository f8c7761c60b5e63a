// pmc_inflate_range.hip -- ranged reads of indexed members (include/pmc_codec.h "ranged reads").
//
// An indexed member can be entered at every chunk, so a byte range of its value costs the chunks that hold it
// and nothing else: one LANE per (request, covered chunk), decoding with the chunk pass's routine
// (pmc_inflate_chunk.hip chunk_decode -- the same structural test, the same LDS layout).
//   inflate_range_scan_kernel    one thread per request: the index check, the clamped range, the early verdicts
//                                (an empty range, a capacity too small) and the number of covered chunks
//   (exclusive prefix sum of the counts: scan_u32, pmc_capi.hip)
//   inflate_range_kernel         one lane per covered chunk; a wave takes 64 consecutive items
//   inflate_range_finish_kernel  one thread per request: rc, dst_len and the context's three counters
// A chunk that lies wholly inside the range is decoded straight into its place in dst.  A chunk the range
// covers only in part (at most two per request) is decoded whole into an edge row of the call's scratch -- its
// matches may reach anywhere in the chunk -- and the lane then copies the wanted slice.  Nothing outside
// [dst_off, dst_off + L) is written; the member's CRC is not checked (it covers bytes this call did not produce),
// and no verdict on the stream is given: a chunk that does not decode exactly as its index says declines the
// request (PMC_E_NO_INDEX), and the caller's full read says why.
// A member that carries chunk CRCs (the 'P' 'C' subfield, pmc_plan.hpp idx_crc_parse) has every chunk this call
// decoded checked against its entry, in inflate_range_kernel<true> itself: after the wave's 64 lanes have decoded,
// the wave walks the chunks of such members one at a time, all lanes on one chunk (range_crc32), while an edge
// chunk is still in its row -- a row is reused in the lane's next round, so no later kernel could see it.  A
// mismatch declines the request as a structural failure does.  The tables (4 KiB behind the decoder's LDS) are
// loaded by the first round that needs them; a wave of plain members pays one ballot per round.  The scan counts
// the requests that will need the check (RangeArgs::ncrc); a call that has none runs inflate_range_kernel<false>,
// which is the kernel without any of this, and the other instance returns at its first instruction.
#include <hip/hip_runtime.h>

#include "pmc_device.hpp"
#include "pmc_kernels.hpp"

namespace pmc {

__global__ void __launch_bounds__(256) inflate_range_scan_kernel(InflateArgs a, RangeArgs R) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < a.n; v += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lg, k, isz, hdr, at, items = 0, dl = 0;
        int32_t rc = PMC_E_NO_INDEX;
        const uint8_t *m = a.src + a.src_off[v];
        bool crcs = false;
        if (!R.off && idx_parse(m, a.src_len[v], &lg, &k, &isz, &hdr) && lg <= kRangeLog2Max &&
            ((crcs = idx_crc_sub(m, k, hdr, &at)) || !R.require)) {
            const RangeOf r = range_of(isz, lg, R.range_off[v], R.range_len[v]);
            if (r.L == 0) {
                rc = PMC_OK;
            } else if (r.L > a.dst_cap[v]) {
                rc = PMC_E_CAPACITY;
                dl = r.L;
            } else { // (until the finish kernel: pending, with the length it will answer)
                rc = kInflateRetry;
                dl = r.L;
                items = r.items;
            }
        }
        R.cnt[v] = items;
        R.fail[v] = crcs ? 2u : 0u;
        if (crcs && items) atomicAdd(R.ncrc, 1u);
        a.rc[v] = rc;
        a.dst_len[v] = dl;
    }
}

// n bytes from byte s of the 16-byte aligned row (which has 16 readable bytes behind its chunk) to d
// (global pointers, as the decoder's own stores to the row: see gload16)
__device__ __forceinline__ void range_copy(uint8_t *dst, const uint8_t *src, uint32_t s, uint32_t n) {
    PMC_GLB uint8_t *d = (PMC_GLB uint8_t *)dst;
    PMC_GLB const uint8_t *row = (PMC_GLB const uint8_t *)src;
    while (n && ((uintptr_t)d & 3)) {
        *d++ = row[s++];
        n--;
    }
    PMC_GLB const uint32_t *rw = (PMC_GLB const uint32_t *)row;
    PMC_GLB uint32_t *dw = (PMC_GLB uint32_t *)d;
    const uint32_t nw = n >> 2, k = s >> 2, sh = s & 3;
#pragma unroll 4
    for (uint32_t j = 0; j < nw; j++) dw[j] = __builtin_amdgcn_alignbyte(rw[k + j + 1], rw[k + j], sh);
    for (uint32_t j = nw * 4; j < n; j++) d[j] = row[s + j];
}

// CRC-32 of the n >= 1 bytes at p (global memory, any alignment; p and n wave-uniform) by the whole wave.  The
// bytes are read as the 16-byte aligned pieces that hold them (a piece never crosses a page, so the bytes of the
// first and last piece outside [p, p + n) are readable; they are masked out).  Lane l takes a run of
// consecutive whole pieces and carries one register through them, slicing-by-4 (s4: the first four tables of
// c_crc_slice8, in LDS), from register 0 with the bytes before p as zeros, which leave such a register
// unchanged; the run's register is shifted past the pieces behind it by one GF(2) multiply and the wave XORs.
// The bytes of the last, partial piece and the init value's share 0xFFFFFFFF x^(8 n) are added once.
__device__ inline uint32_t range_crc32(const uint8_t *p, uint32_t n, PMC_LDS const uint32_t *s4) {
    constexpr CrcX8 kX8 = make_crc_x8();
    const uint32_t lead = (uint32_t)((uintptr_t)p & 15);
    PMC_GLB const uint4 *q = (PMC_GLB const uint4 *)((uintptr_t)p - lead);
    const uint32_t E = lead + n, nf = E >> 4, tail = E & 15;
    const uint32_t per = (nf + 63) >> 6, l = (uint32_t)lane_id();
    const uint32_t b = l * per < nf ? l * per : nf, e = b + per < nf ? b + per : nf;
    auto masked = [&](uint4 w, uint32_t j) { // piece j's words, the bytes before p zeroed
        if (j == 0 && lead) {
            uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int32_t r = (int32_t)lead - 4 * i;
                x[i] = r <= 0 ? x[i] : (r >= 4 ? 0u : x[i] & (0xFFFFFFFFu << (8 * r)));
            }
            w = make_uint4(x[0], x[1], x[2], x[3]);
        }
        return w;
    };
    auto step = [&](uint32_t c) {
        return s4[3 * 256 + (c & 0xff)] ^ s4[2 * 256 + ((c >> 8) & 0xff)] ^ s4[256 + ((c >> 16) & 0xff)] ^ s4[c >> 24];
    };
    uint32_t c = 0;
#pragma unroll 4
    for (uint32_t j = b; j < e; j++) {
        const uint4 w = masked(gload16(q + j), j);
        c = step(c ^ w.x);
        c = step(c ^ w.y);
        c = step(c ^ w.z);
        c = step(c ^ w.w);
    }
    uint32_t acc = e > b ? (nf - e ? multmodp(crc_shift_chunks(nf - e), c) : c) : 0u;
    acc = wave_xor_dpp(acc);
    if (tail) { // (uniform: every lane computes the same)
        const uint4 w = masked(gload16(q + nf), nf);
        const uint32_t x[4] = {w.x, w.y, w.z, w.w};
        uint32_t t = 0;
#pragma unroll
        for (uint32_t i = 0; i < 15; i++)
            if (i < tail) t = s4[(t ^ (x[i >> 2] >> (8 * (i & 3)))) & 0xff] ^ (t >> 8);
        acc = multmodp(kX8.v[tail], acc) ^ t;
    }
    const uint32_t ones = multmodp(multmodp(crc_shift_chunks(n >> 4), kX8.v[n & 15]), 0xFFFFFFFFu);
    return ~(acc ^ ones);
}

// the range kernel's dynamic LDS: the chunk decoder's, then the four slicing tables of range_crc32.  Three
// blocks per CU as before: 3 x kRangeLdsBytes stays below the CU's 160 KiB
constexpr uint32_t kRangeCrcTabOff = (kChunkLdsBytes + 15) & ~15u;
constexpr uint32_t kRangeLdsBytes = kRangeCrcTabOff + 4 * 256 * 4;
static_assert(3 * ((kRangeLdsBytes + 511) & ~511u) <= 160u * 1024, "inflate_range_kernel: three blocks per CU");

template <bool kVerify>
__global__ void __launch_bounds__(64) inflate_range_kernel(InflateArgs a, RangeArgs R) {
    typedef ChunkLayout LL;
    if ((*R.ncrc != 0) != kVerify) return; // (the other instance's call)
    extern __shared__ __attribute__((aligned(16))) uint16_t lcol[];
    PMC_LDS uint16_t *col = to_lds<uint16_t>(lcol + threadIdx.x);
    PMC_LDS uint32_t *ring = to_lds<uint32_t>((uint8_t *)lcol + LL::kRingOff) + threadIdx.x;
    PMC_LDS uint8_t *bcol = to_lds<uint8_t>((uint8_t *)lcol + LL::kBColOff + threadIdx.x);
    PMC_LDS uint32_t *winw = to_lds<uint32_t>((uint8_t *)lcol + LL::kWinOff) + threadIdx.x;
    PMC_LDS uint32_t *s4 = to_lds<uint32_t>((uint8_t *)lcol + kRangeCrcTabOff);
    bool s4_ready = false;
    uint32_t vok = 0, vbad = 0; // chunks of this lane whose CRC matched / did not
    const uint64_t total = *R.total;
    for (uint64_t ib = (uint64_t)blockIdx.x * 64; ib < total; ib += (uint64_t)gridDim.x * 64) {
        const uint64_t it = ib + threadIdx.x;
        uint32_t st = it < total ? 0u : 3u; // (chunk_decode: 0 an item, 3 none)
        // the item's request: the last one whose prefix is <= it (requests of no items share their successor's)
        uint64_t v = 0;
        if (st == 0) {
            uint64_t lo = 0, hi = a.n - 1;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if (R.pre[mid] <= it) lo = mid;
                else hi = mid - 1;
            }
            v = lo;
        }
        const uint8_t *m = st == 0 ? a.src + a.src_off[v] : a.src;
        const uint32_t in_len = st == 0 ? a.src_len[v] : 0u;
        uint32_t start = 0, next = 0, clen = 0, c0 = 0, lo = 0, hi = 0, o0 = 0, want = 0;
        bool lastc = true, whole = false, crcs = false;
        uint8_t *row = R.rows, *slot = a.dst;
        if (st == 0) {
            const uint32_t lg = m[17];
            const uint32_t isz = idx_u32(m + in_len - 4);
            const uint32_t xlen = (uint32_t)m[10] | (uint32_t)m[11] << 8;
            const RangeOf r = range_of(isz, lg, R.range_off[v], R.range_len[v]);
            const uint32_t k = r.k0 + (uint32_t)(it - R.pre[v]);
            const uint32_t K = (uint32_t)(((uint64_t)isz + (1u << lg) - 1) >> lg);
            start = k == 0 ? 12 + xlen : idx_u32(m + kIdxHdrFixed + 4 * (k - 1));
            lastc = k + 1 == K;
            next = lastc ? in_len - 8 : idx_u32(m + kIdxHdrFixed + 4 * k);
            c0 = k << lg; // (k < K: below ISIZE)
            clen = isz - c0 < (1u << lg) ? isz - c0 : (1u << lg);
            // the chunk's part of the range: value bytes [lo, hi), hi - lo >= 1
            o0 = r.o;
            lo = c0 > r.o ? c0 : r.o;
            const uint64_t ce = (uint64_t)c0 + clen, re = (uint64_t)r.o + r.L;
            hi = (uint32_t)(ce < re ? ce : re);
            whole = lo == c0 && hi - lo == clen;
            slot = a.dst + a.dst_off[v];
            const uint64_t ri = R.row_per_request ? 2 * v + (k != r.k0 ? 1 : 0) : (uint64_t)blockIdx.x * 64 + threadIdx.x;
            row = R.rows + ri * kRangeRowBytes;
            // (bit 1 is the scan's and every later store keeps it; the entries lie inside the header, idx_crc_sub)
            if (kVerify) {
                crcs = (R.fail[v] & 2u) != 0;
                if (crcs) want = idx_u32(m + 16 + 4 * K + kIdxCrcFixed + 4 * k);
            }
        }
        st = chunk_decode<LL>(col, ring, bcol, winw, st, m, in_len, start, next, clen, lastc,
                              whole ? slot + (c0 - o0) : row);
        if (st == 2) R.fail[v] = crcs ? 3u : 1u;
        // an edge chunk: the lane copies its own slice (its own stores, so no other lane's are waited for)
        if (st == 8 && !whole) range_copy(slot + (lo - o0), row, lo - c0, hi - lo);
        // chunk CRCs: every decoded chunk of a member that carries them, whole (in dst or in its row), by the
        // whole wave, before the next round reuses the row
        const bool vfy = kVerify && st == 8 && crcs;
        uint64_t vm = kVerify ? ballot(vfy) : 0ull;
        if (vm) {
            if (!s4_ready) {
                for (uint32_t j = threadIdx.x; j < 4 * 256; j += 64) s4[j] = c_crc_slice8[j];
                s4_ready = true;
            }
            wave_sync_global(); // the lanes' stores of their chunks visible to the wave (and the tables)
            const uint64_t cp = (uint64_t)(uintptr_t)(whole ? slot + (c0 - o0) : row);
            bool bad = false;
            while (vm) {
                const int j = __builtin_ctzll(vm);
                vm &= vm - 1;
                const uint32_t got = range_crc32((const uint8_t *)(uintptr_t)readlane64(cp, j), readlane(clen, j), s4);
                if ((int)threadIdx.x == j) bad = got != want;
            }
            if (vfy) {
                if (bad) R.fail[v] = 3u;
                vbad += bad ? 1u : 0u;
                vok += bad ? 0u : 1u;
            }
        }
    }
    if (kVerify) { // one atomic per wave and counter
        vok = wave_sum_u32(vok);
        vbad = wave_sum_u32(vbad);
        if (threadIdx.x == 0) {
            if (vok) atomicAdd((unsigned long long *)&R.vcounts[0], (unsigned long long)vok);
            if (vbad) atomicAdd((unsigned long long *)&R.vcounts[1], (unsigned long long)vbad);
        }
    }
}
template __global__ void inflate_range_kernel<false>(InflateArgs, RangeArgs);
template __global__ void inflate_range_kernel<true>(InflateArgs, RangeArgs);

__global__ void __launch_bounds__(256) inflate_range_finish_kernel(InflateArgs a, RangeArgs R) {
    // (every thread runs the same number of rounds: the ballots below are whole waves')
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, rounds = (a.n + stride - 1) / stride;
    uint64_t served = 0, declined = 0, chunks = 0;
    for (uint64_t q = 0; q < rounds; q++) {
        const uint64_t v = q * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        int32_t rc = 1;
        if (v < a.n) {
            const uint32_t c = R.cnt[v];
            rc = a.rc[v];
            if (c) {
                chunks += c;
                rc = (R.fail[v] & 1u) ? PMC_E_NO_INDEX : PMC_OK;
                a.rc[v] = rc;
                if (rc) a.dst_len[v] = 0;
            }
        }
        served += rc == PMC_OK ? 1 : 0;
        declined += rc == PMC_E_NO_INDEX ? 1 : 0;
    }
    // one atomic per wave and counter
    for (int d = 32; d >= 1; d >>= 1) {
        served += __shfl_xor((unsigned long long)served, d);
        declined += __shfl_xor((unsigned long long)declined, d);
        chunks += __shfl_xor((unsigned long long)chunks, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (served) atomicAdd((unsigned long long *)&R.counts[0], (unsigned long long)served);
        if (declined) atomicAdd((unsigned long long *)&R.counts[1], (unsigned long long)declined);
        if (chunks) atomicAdd((unsigned long long *)&R.counts[2], (unsigned long long)chunks);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *R.ncrc = 0; // (both range kernels have run: the next call's scan counts anew)
}

} // namespace pmc

// pmc_deflate_fast.hip -- the fast level's front (PMC_LEVEL_FAST): one wave per value of up to
// 16382 bytes, same contract as deflate_front_kernel (token slab cT, counts cN, histogram rows cH,
// used-symbol counts cZ, the same work-counter grabs and the same lane-order guard), but a parse
// shaped for the GPU instead of zlib's deflate_slow.  The trees and back kernels take its tokens
// unchanged; the member is a valid gzip member, not the reference's bytes.
//
// The parse (tests/fast_model.py is its normative statement, DESIGN.md §4 "Front, fast level"):
//   cands(p)  the up-to-kFastK nearest earlier positions with p's hash, nearest first: the entries
//             just before p in its run of the stable hash-sorted order S (position 0 never)
//   ml(p)     the longest common prefix with a candidate, capped at kFastCap and the bytes left;
//             0 below 3, 0 for a length-3 match more than 4096 back; mq(p) its (nearest) candidate
//   walk      at p: a match of ml(p) (extended to 258 when it hit the cap) unless ml(p + 1) is
//             longer (one-step lazy rule); else the literal
// ml and mq depend on the value only, so one pass over S computes them for all positions, 64 per
// step: lane k holds the 32 bytes at S[k], its candidates' bytes arrive from lanes k - 1, k - 2 by
// whole-wave DPP shifts (no LDS reads for them).  The walk then runs per 64-position window: the
// positions that would emit a match are one ballot; the scalar side hops from match to match (a
// find-first-set, a v_readlane of the length) and clears the positions the matches cover, and all
// tokens of the window are stored by their lanes at once (literal runs are implied by the mask).
#include <hip/hip_runtime.h>

#include "pmc_device.hpp"
#include "pmc_kernels.hpp"

namespace pmc {

constexpr uint32_t kFastK = 2, kFastLazy = 1, kFastCap = 32;

// bytes | S | R | X as the exact front (front_layout), so the sort runs unchanged.  R holds mq per
// position; ml sits in R's top 6 bits for values of <= 1 KiB (positions take 10), else in a u8 array
// at X (over the sort's 512-byte table, dead by then).  No EV, no eval scratch.
struct FastLayout {
    uint64_t bytes, S, R, X, ml, freq, total;
    int pk; // 6: ml packed into R; 4: S packed as 12-bit fields (front_s12); 0: plain
};
__host__ __device__ inline FastLayout fast_layout(uint64_t n) {
    auto a = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    const FrontLayout F = front_layout(n);
    FastLayout L;
    L.bytes = F.bytes;
    L.S = F.S;
    L.R = F.R;
    L.X = F.X;
    L.ml = F.X;
    L.freq = F.freq;
    L.pk = n <= 1024 ? 6 : front_s12(n) ? 4 : 0;
    const uint64_t mlb = L.pk == 6 ? 0 : a(n + 2);
    const uint64_t xe = F.X + (mlb > 512 ? mlb : 512), t2 = F.freq + 352 * 4;
    L.total = a(xe > t2 ? xe : t2);
    return L;
}
uint64_t deflate_front_fast_wave_bytes(uint64_t n) { return fast_layout(n).total; }

struct FastWave {
    SmallWave &w;
    PMC_LDS uint8_t *ML;

    // lane l - 1's v; lane 0 takes `carry` (the previous chunk's lane 63)
    __device__ static __forceinline__ uint32_t shr1(uint32_t carry, uint32_t v) {
        return (uint32_t)__builtin_amdgcn_update_dpp((int)carry, (int)v, 0x138, 0xf, 0xf, false); // wave_shr:1
    }

    // ml / mq of every position, in sorted order.  Returns 1 (uniform) when S is not the stable hash
    // order (the sort's lane-order guard, as build_cn's).
    template <int PK>
    __device__ __forceinline__ uint32_t table(uint32_t npos, uint32_t len) {
        const uint32_t l = (uint32_t)lane_id();
        uint32_t ch[kFastK], cp[kFastK], ca[kFastK][8]; // lane 63 of the previous chunk, shifted j times
#pragma unroll
        for (uint32_t j = 0; j < kFastK; j++) {
            ch[j] = 0xffffffffu;
            cp[j] = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) ca[j][i] = 0;
        }
        uint32_t bad = 0;
        for (uint32_t c0 = 0; c0 < npos; c0 += 64) {
            const uint32_t k = c0 + l;
            const bool valid = k < npos;
            const uint32_t p = valid ? w.sget<PK>(k) : 0u;
            uint32_t a[8];
            {
                uint64_t A0, A1, A2, A3;
                w.load16(p, A0, A1);
                w.load16(p + 16, A2, A3);
                a[0] = (uint32_t)A0, a[1] = (uint32_t)(A0 >> 32), a[2] = (uint32_t)A1, a[3] = (uint32_t)(A1 >> 32);
                a[4] = (uint32_t)A2, a[5] = (uint32_t)(A2 >> 32), a[6] = (uint32_t)A3, a[7] = (uint32_t)(A3 >> 32);
            }
            const uint32_t h = valid ? hash3(a[0]) : 0xfffffffeu;
            const uint32_t left = len - p, cap = left < kFastCap ? left : kFastCap;
            uint32_t best = 0, bq = 0;
            uint32_t sh = h, sp = p, sa[8];
#pragma unroll
            for (int i = 0; i < 8; i++) sa[i] = a[i];
#pragma unroll
            for (uint32_t j = 0; j < kFastK; j++) { // candidate j: the entry j + 1 places before k
                const uint32_t nh = shr1(ch[j], sh), nq = shr1(cp[j], sp);
                ch[j] = readlane(sh, 63);
                cp[j] = readlane(sp, 63);
                uint32_t x8[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const uint32_t nb = shr1(ca[j][i], sa[i]);
                    ca[j][i] = readlane(sa[i], 63);
                    sa[i] = nb;
                    x8[i] = a[i] ^ nb;
                }
                if (j == 0) // (hash, position) must increase along S (k = 0 has no predecessor)
                    bad |= (valid && k != 0 && (h < nh || (h == nh && p <= nq))) ? 1u : 0u;
                // leading equal bytes: the first differing dword's lowest set byte (32 when none)
                uint32_t m = 32u;
#pragma unroll
                for (int i = 7; i >= 0; i--) m = x8[i] ? 4u * i + ((uint32_t)__builtin_ctz(x8[i]) >> 3) : m;
                m = m < cap ? m : cap;
                // same run, inside the array (k > j), not zlib's NIL; a collision keeps its slot
                m = valid && k > j && nh == h && nq != 0u ? m : 0u;
                const bool better = m > best; // (nearest first: ties stay)
                best = better ? m : best;
                bq = better ? nq : bq;
                sh = nh;
                sp = nq;
            }
            if (best == 3u && p - bq > 4096u) best = 0u; // TOO_FAR
            if (best < 3u) best = 0u;
            if (valid) {
                if (PK == 6) {
                    w.R[p] = (uint16_t)(bq | best << 10);
                } else {
                    w.R[p] = (uint16_t)bq;
                    ML[p] = (uint8_t)best;
                }
            }
        }
        if (l < 2) { // the last two positions hash nothing: ml = 0 (npos + 1 < len)
            if (PK == 6) w.R[npos + l] = 0;
            else ML[npos + l] = 0;
        }
        wave_sync();
        return ballot(bad != 0u) ? 1u : 0u;
    }

    // a match at x with candidate q that hit the cap: its length up to min(258, len - x).  Lane l
    // compares the 4 bytes at offset kFastCap + 4 l (offsets up to 287 cover 258 in one step).
    __device__ __forceinline__ uint32_t extend(uint32_t x, uint32_t q, uint32_t len) const {
        const uint32_t l = (uint32_t)lane_id();
        const uint32_t lim = len - x < 258u ? len - x : 258u;
        const uint32_t off = kFastCap + 4u * l;
        const bool act = off < lim; // (x + off < len: the loads stay inside the staged bytes)
        const uint32_t d = act ? w.load4(x + off) ^ w.load4(q + off) : 0u;
        const uint64_t sm = ballot(act && d != 0u);
        uint32_t L = lim;
        if (sm) {
            const int fl = __builtin_ctzll(sm);
            const uint32_t dl = readlane(d, fl);
            L = kFastCap + 4u * (uint32_t)fl + ((uint32_t)__builtin_ctz(dl) >> 3);
            L = L < lim ? L : lim;
        }
        return L;
    }

    // (p0: the walk's first position -- 0, or the dictionary's length when `len` bytes of dictionary ||
    // value are staged; literal tokens are stored relative to p0, in the value's coordinates.  LITB: a
    // literal token is the byte itself, the form the large-value emit reads -- pmc_deflate_fast_large.hip)
    template <int PK, bool LITB = false>
    __device__ __forceinline__ uint32_t walk(uint32_t len, uint32_t p0 = 0) {
        const uint32_t l = (uint32_t)lane_id();
        uint32_t p = p0, ntok = 0;
        for (uint32_t w0 = p0; w0 < len; w0 += 64) {
            if (p >= w0 + 64u) continue; // a match covers the whole window
            const uint32_t x = w0 + l;
            const bool in = x < len;
            const uint32_t xc = in ? x : 0u, x1 = x + 1u < len ? x + 1u : 0u;
            uint32_t m, q, m1;
            if (PK == 6) {
                const uint32_t r = w.R[xc], r1 = w.R[x1];
                m = r >> 10, q = r & 1023u, m1 = r1 >> 10;
            } else {
                m = ML[xc], q = w.R[xc], m1 = ML[x1];
            }
            m = in ? m : 0u;
            m1 = x + 1u < len ? m1 : 0u;
            const bool ism = m >= 3u && !(kFastLazy && m1 > m);
            const uint64_t mm = ballot(ism);
            const uint32_t pp0 = p - w0; // (p >= w0 here: every window leaves p at its end or beyond)
            uint32_t pp = pp0, mlen = m;
            uint64_t cov = 0;
            for (;;) {
                const uint64_t rem = mm & (~0ull << pp);
                if (!rem) { // literals to the end of the window
                    pp = 64;
                    break;
                }
                const uint32_t t = (uint32_t)__builtin_ctzll(rem);
                uint32_t L = readlane(m, (int)t);
                if (L == kFastCap) {
                    L = extend(w0 + t, readlane(q, (int)t), len);
                    mlen = writelane(mlen, L, (int)t);
                }
                const uint32_t e = t + L; // the match covers t + 1 .. e - 1
                cov |= (e >= 64u ? ~0ull : (1ull << e) - 1ull) & ((~0ull << t) << 1);
                pp = e;
                if (pp >= 64u) break;
            }
            p = w0 + pp;
            const uint64_t starts = (~0ull << pp0) & ballot(in) & ~cov;
            if ((starts >> l) & 1ull)
                w.tok[ntok + popc_lt(starts)] = ism ? (x - q) << 16 | (mlen - 3u) : LITB ? (uint32_t)w.b[x] : x - p0;
            ntok += (uint32_t)__builtin_popcountll(starts);
        }
        return ntok;
    }

    template <int PK, bool LITB = false>
    __device__ __forceinline__ uint32_t parse(uint32_t npos, uint32_t len, uint32_t p0 = 0) {
        if (sflag(table<PK>(npos, len))) return kNtokRetry;
        return walk<PK, LITB>(len, p0);
    }

    // (inlined into the kernel: called through a pointer, the SmallWave would live in scratch memory)
    __device__ __forceinline__ uint32_t run_front(const uint8_t *src, uint32_t len, int pk) {
        w.stage(src, len);
        w.stamp(0);
        const uint32_t npos = len >= 3 ? len - 2 : 0;
        uint32_t ntok;
        if (npos) {
            w.sort_positions2(npos, (PMC_LDS uint32_t *)w.CN);
            w.stamp(1);
            ntok = pk == 6 ? parse<6>(npos, len) : pk == 4 ? parse<4>(npos, len) : parse<0>(npos, len);
            if (sflag(ntok == kNtokRetry ? 1u : 0u)) return kNtokRetry; // (sort guard: no histogram)
        } else {
            w.lit_run(0, 0, len);
            ntok = len;
        }
        wave_sync_global();
        w.stamp(2);
        w.histogram(ntok, len);
        w.stamp(6);
        return ntok;
    }

    // ---- with a preset dictionary (DESIGN.md §4 "Front, fast level with a dictionary") ----------------
    // The wave's byte area holds dictionary || value: the dictionary's D bytes are staged once per wave
    // (stage_dict), every value behind them (stage_value).  The sort and table() run over all D + len
    // bytes; the walk, the histogram and the tokens' literal positions start at D.

    // (`dict` is the context's buffer: 16-byte aligned, zero padded to a multiple of 4 bytes)
    __device__ __forceinline__ void stage_dict(const uint8_t *dict, uint32_t D) {
        PMC_GLB const uint32_t *d4 = (PMC_GLB const uint32_t *)dict;
        for (uint32_t k = (uint32_t)lane_id(); k < (D + 3) >> 2; k += 64) w.bw[k] = d4[k];
        wave_sync();
    }
    // value bytes to b[D, D + len), zeros on to the padded end (as SmallWave::stage); the word that
    // straddles D keeps its dictionary bytes.  Source dwords are read aligned, and only those that hold
    // at least one byte of the value: unlike SmallWave::stage this reads up to 3 bytes before src and up to
    // 3 past src + len, on purpose -- an aligned dword lies in the page of the value byte it holds, and the
    // bytes outside the value are masked off (keep) before the store.
    __device__ __forceinline__ void stage_value(const uint8_t *src, uint32_t len, uint32_t D) {
        const uint32_t T = D + len, k1 = ((T + 32) & ~3u) >> 2;
        const uintptr_t sa = (uintptr_t)src - D; // where byte 0 of the concatenation would lie
        const uint32_t sh = (uint32_t)(sa & 3);
        const uintptr_t g = sa & ~(uintptr_t)3;  // dword k of g holds concatenation bytes 4 k - sh ..
        for (uint32_t k = (D >> 2) + (uint32_t)lane_id(); k < k1; k += 64) {
            const int32_t c0 = (int32_t)(4u * k) - (int32_t)sh;
            const bool inlo = c0 + 3 >= (int32_t)D && c0 < (int32_t)T;
            const bool inhi = sh != 0u && c0 + 7 >= (int32_t)D && c0 + 4 < (int32_t)T;
            const uint32_t lo = inlo ? *(PMC_GLB const uint32_t *)(g + 4ull * k) : 0u;
            const uint32_t hi = inhi ? *(PMC_GLB const uint32_t *)(g + 4ull * k + 4) : 0u;
            const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh);
            const uint32_t c = 4u * k;
            uint32_t keep = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) keep |= (c + j >= D && c + j < T) ? 0xffu << (8 * j) : 0u;
            const uint32_t dmask = c < D ? (1u << (8 * ((D - c) & 3u))) - 1u : 0u; // (D - c is 1..3 here)
            const uint32_t old = c < D ? w.bw[k] & dmask : 0u;
            w.bw[k] = old | (v & keep);
        }
        wave_sync();
    }
    __device__ __forceinline__ uint32_t run_front_dict(const uint8_t *src, uint32_t len, uint32_t D, int pk) {
        stage_value(src, len, D);
        w.stamp(0);
        const uint32_t T = D + len, npos = T >= 3 ? T - 2 : 0;
        uint32_t ntok;
        if (npos) {
            w.sort_positions2(npos, (PMC_LDS uint32_t *)w.CN);
            w.stamp(1);
            ntok = pk == 6 ? parse<6>(npos, T, D) : pk == 4 ? parse<4>(npos, T, D) : parse<0>(npos, T, D);
            if (sflag(ntok == kNtokRetry ? 1u : 0u)) return kNtokRetry; // (sort guard: no histogram)
        } else {
            w.lit_run(0, 0, len);
            ntok = len;
        }
        wave_sync_global();
        w.stamp(2);
        PMC_LDS uint8_t *b0 = w.b;
        w.b = b0 + D; // (literal tokens are in the value's coordinates)
        w.histogram(ntok, len);
        w.b = b0;
        w.stamp(6);
        return ntok;
    }
};

template <uint32_t CAPC>
__global__ void __launch_bounds__(256, 7) deflate_front_fast_kernel(DeflateArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int wib = threadIdx.x / 64, l = lane_id();
    const uint64_t lcap = CAPC ? (uint64_t)CAPC : a.cap_len;
    const FastLayout F = fast_layout(lcap);
    uint8_t *base = lds + (uint64_t)wib * (CAPC ? F.total : a.wave_bytes);
    const SmallLayout L = small_layout(lcap);
    SmallWave w;
    small_wave_init(w, base, L, a, nullptr);
    w.S = to_lds<uint16_t>(base + F.S);
    w.R = to_lds<uint16_t>(base + F.R);
    w.CN = to_lds<uint8_t>(base + F.X); // (the sort's 512-byte table)
    w.s12 = F.pk == 4 ? 1u : 0u;
    w.lfreq = to_lds<uint32_t>(base + F.freq);
    w.dfreq = w.lfreq + 288;
    w.blfreq = w.dfreq + 32;
    FastWave fw{w, to_lds<uint8_t>(base + F.ml)};
    // (work-counter grabs as deflate_front_kernel's)
    const uint32_t kBatch = a.front_batch;
    uint32_t nx = l == 0 ? atomicAdd(a.cQ, kBatch) : 0u;
    for (;;) {
        const uint64_t g = readlane(nx, 0);
        if (g >= a.count) break;
        nx = l == 0 ? atomicAdd(a.cQ, kBatch) : 0u;
        const uint64_t vl = g + (uint64_t)l;
        const bool in = (uint32_t)l < kBatch && vl < a.count;
        const uint32_t myl = in ? a.src_len[a.first + vl] : 0u;
        const uint64_t myo = in ? a.src_off[a.first + vl] : 0u;
        uint64_t todo = ballot(myl != 0 && myl > a.min_len && myl <= a.lds_max_len);
        while (todo) {
            const int jj = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t v = g + (uint64_t)jj, gv = a.first + v;
            const uint32_t len = readlane(myl, jj);
            w.tok = (PMC_GLB uint32_t *)(a.cT + v * a.cap_len);
#ifdef PMC_FAULT_LANE_ORDER // (odd values fail the sort's guard, as in the exact front)
            w.fault_rev = (uint32_t)(gv & 1);
#endif
            const uint8_t *vsrc = a.src + readlane64(myo, jj);
            const uint32_t ntok = fw.run_front(vsrc, len, F.pk);
            if (ntok == kNtokRetry) { // the sort's lane-order guard fired: the HBM kernel redoes the value (exact)
                if (l == 0) {
                    a.cN[v] = kNtokRetry;
                    a.cZ[v] = 0;
                    atomicAdd(a.guard, 1u);
                }
                continue;
            }
            uint32_t nz = 0;
            for (int s = l; s < kLCodes + kDCodes; s += 64) {
                const uint32_t f = s < kLCodes ? w.lfreq[s] : w.dfreq[s - kLCodes];
                a.cH[v * kSplitRows + s] = (uint16_t)f;
                nz += (uint32_t)__builtin_popcountll(ballot(s < kLCodes && f != 0));
            }
            if (l == 0) {
                a.cN[v] = ntok < kSymsPerBlock ? ntok : kNtokMultiBlock;
                a.cZ[v] = nz;
            }
        }
    }
    small_wave_stamps_out(w, a);
}
// The dictionary instance: the values of a.min_len < len <= a.lds_max_len (the host keeps
// a.dict_len + a.lds_max_len <= 16382), each parsed behind the a.dict_len bytes at a.dict.  The LDS
// layout, the ml packing and the sort follow a.front_cap >= a.dict_len + a.lds_max_len; the token slab's
// stride stays a.cap_len (a value has at most len tokens).
__global__ void __launch_bounds__(256, 7) deflate_front_fast_dict_kernel(DeflateArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int wib = threadIdx.x / 64, l = lane_id();
    const uint64_t lcap = a.front_cap;
    const uint32_t D = a.dict_len;
    const FastLayout F = fast_layout(lcap);
    uint8_t *base = lds + (uint64_t)wib * a.wave_bytes;
    const SmallLayout L = small_layout(lcap);
    SmallWave w;
    small_wave_init(w, base, L, a, nullptr);
    w.S = to_lds<uint16_t>(base + F.S);
    w.R = to_lds<uint16_t>(base + F.R);
    w.CN = to_lds<uint8_t>(base + F.X); // (the sort's 512-byte table)
    w.s12 = F.pk == 4 ? 1u : 0u;
    w.lfreq = to_lds<uint32_t>(base + F.freq);
    w.dfreq = w.lfreq + 288;
    w.blfreq = w.dfreq + 32;
    FastWave fw{w, to_lds<uint8_t>(base + F.ml)};
    fw.stage_dict(a.dict, D);
    const uint32_t kBatch = a.front_batch;
    uint32_t nx = l == 0 ? atomicAdd(a.cQ, kBatch) : 0u;
    for (;;) {
        const uint64_t g = readlane(nx, 0);
        if (g >= a.count) break;
        nx = l == 0 ? atomicAdd(a.cQ, kBatch) : 0u;
        const uint64_t vl = g + (uint64_t)l;
        const bool in = (uint32_t)l < kBatch && vl < a.count;
        const uint32_t myl = in ? a.src_len[a.first + vl] : 0u;
        const uint64_t myo = in ? a.src_off[a.first + vl] : 0u;
        // (D + len <= front_cap is what keeps every LDS index inside the wave's working set)
        uint64_t todo = ballot(myl != 0 && myl > a.min_len && myl <= a.lds_max_len && (uint64_t)D + myl <= lcap);
        while (todo) {
            const int jj = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t v = g + (uint64_t)jj;
            const uint32_t len = readlane(myl, jj);
            w.tok = (PMC_GLB uint32_t *)(a.cT + v * a.cap_len);
#ifdef PMC_FAULT_LANE_ORDER
            w.fault_rev = (uint32_t)((a.first + v) & 1);
#endif
            const uint8_t *vsrc = a.src + readlane64(myo, jj);
            const uint32_t ntok = fw.run_front_dict(vsrc, len, D, F.pk);
            if (ntok == kNtokRetry) { // the sort's lane-order guard fired: the HBM kernel redoes the value (exact)
                if (l == 0) {
                    a.cN[v] = kNtokRetry;
                    a.cZ[v] = 0;
                    atomicAdd(a.guard, 1u);
                }
                continue;
            }
            uint32_t nz = 0;
            for (int s = l; s < kLCodes + kDCodes; s += 64) {
                const uint32_t f = s < kLCodes ? w.lfreq[s] : w.dfreq[s - kLCodes];
                a.cH[v * kSplitRows + s] = (uint16_t)f;
                nz += (uint32_t)__builtin_popcountll(ballot(s < kLCodes && f != 0));
            }
            if (l == 0) {
                a.cN[v] = ntok < kSymsPerBlock ? ntok : kNtokMultiBlock;
                a.cZ[v] = nz;
            }
        }
    }
    small_wave_stamps_out(w, a);
}

template __global__ void deflate_front_fast_kernel<0>(DeflateArgs);
template __global__ void deflate_front_fast_kernel<1024>(DeflateArgs);
template __global__ void deflate_front_fast_kernel<4096>(DeflateArgs);

} // namespace pmc

// pmc_deflate_fast_large.hip -- the fast parse for values above 16382 bytes (PMC_LEVEL_FAST_ALL): the
// value is cut into segments of kFlSeg bytes, and one wave per segment runs the fast level's front
// (pmc_deflate_fast.hip: FastWave) over "the kFlHist bytes before the segment || the segment", walked
// from the segment's first byte -- the dictionary front's parse with the value's own bytes as the
// dictionary.  A segment's tokens depend on the value only; matches end at their segment's end and reach
// at most kFlSeg + kFlHist - 1 back.  tests/fast_large_model.py is the parse's normative statement
// (DESIGN.md §4 "Front, fast level, large values").
//
// The tokens go to the segment's buffer in the form deflate_lv_emit_kernel reads (a literal is its byte,
// a match dist << 16 | len - 3); that kernel, one wave per value, then writes the member: blocks of 16383
// symbols, a stored block where it is smaller, CRC-32 and trailer.  A segment whose sort fails the
// lane-order guard marks its value in L.fail: the emit kernel hands it to the retry pass (level 9).
#include <hip/hip_runtime.h>

#include "pmc_device.hpp"
#include "pmc_kernels.hpp"

namespace pmc {

// kFlSeg + kFlHist <= 16382 (the fast front's span: u16 positions, position 0 never a candidate).  The
// working set is ~6 bytes of LDS per staged byte, so the span sets the waves a CU holds: 2048 + 2048 (the
// 12-bit packed sort of the 4 KiB front, 22.6 KB per wave, 7 waves per CU) parsed 40K x 64 KiB in 92 ms where
// 8192 + 4096 (2 waves per CU) took 202 ms, for members 2.6 % larger (DESIGN.md §4 has the table).
constexpr uint32_t kFlSeg = 2048, kFlHist = 2048;
constexpr uint32_t kFlCap = (kFlSeg + kFlHist + 63) & ~63u; // the LDS layout's capacity
static_assert(kFlSeg + kFlHist <= kSmallMax && kFlCap <= 16384, "fast large-value segment span");
static_assert(kIdxSeg == kFlSeg && kIdxChunk % kFlSeg == 0, "an index chunk is whole segments");

uint64_t lv_fast_wave_bytes() { return fast_layout(kFlCap).total; }

__global__ void __launch_bounds__(256) lv_fast_parse_kernel(DeflateArgs a, LargeArgs L) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int wib = threadIdx.x / 64, l = lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const FastLayout F = fast_layout(kFlCap);
    uint8_t *base = lds + (uint64_t)wib * a.wave_bytes;
    const SmallLayout SL = small_layout(kFlCap);
    SmallWave w;
    small_wave_init(w, base, SL, a, nullptr);
    w.S = to_lds<uint16_t>(base + F.S);
    w.R = to_lds<uint16_t>(base + F.R);
    w.CN = to_lds<uint8_t>(base + F.X); // (the sort's 512-byte table)
    w.s12 = F.pk == 4 ? 1u : 0u;
    FastWave fw{w, to_lds<uint8_t>(base + F.ml)};
    for (uint64_t sg = wave; sg < L.nseg; sg += nwaves) {
        const uint32_t ov = L.seg_val[sg];
        const uint32_t v = L.lv_val[ov];
        const uint32_t len = a.src_len[v];
        const uint64_t s0 = (sg - L.lv_seg0[ov]) * (uint64_t)kFlSeg;
        uint32_t ntok = 0;
        if (s0 < len) { // (the host cut the value into ceil(len / kFlSeg) segments)
            // (an indexed value's history stops at its chunk's first byte: chunks decode independently)
            const uint64_t hs = idx_plan(len, L.idx_chunk).indexed ? s0 & (uint64_t)(L.idx_chunk - 1) : s0;
            const uint32_t h = hs < kFlHist ? (uint32_t)hs : kFlHist;
            const uint32_t seglen = len - s0 < kFlSeg ? (uint32_t)(len - s0) : kFlSeg;
            const uint32_t T = h + seglen; // staged bytes: <= kFlHist + kFlSeg <= kFlCap
            w.tok = (PMC_GLB uint32_t *)(L.tok + L.seg_tok0[sg]);
#ifdef PMC_FAULT_LANE_ORDER // (odd values fail the sort's guard, as in the other fronts)
            w.fault_rev = v & 1u;
#endif
            w.stage(a.src + a.src_off[v] + s0 - h, T);
            if (T >= 3) {
                const uint32_t npos = T - 2;
                w.sort_positions2(npos, (PMC_LDS uint32_t *)w.CN);
                ntok = F.pk == 6   ? fw.parse<6, true>(npos, T, h)
                       : F.pk == 4 ? fw.parse<4, true>(npos, T, h)
                                   : fw.parse<0, true>(npos, T, h);
            } else { // (one or two bytes behind nothing: an indexed value's last chunk)
                if ((uint32_t)l < T) w.tok[l] = w.b[l];
                ntok = T;
            }
            if (sflag(ntok == kNtokRetry ? 1u : 0u)) { // the sort's lane-order guard fired
                if (l == 0) {
                    L.fail[ov] = 1;
                    atomicAdd(a.guard, 1u);
                }
                ntok = 0;
            }
        }
        if (l == 0) {
            L.seg_tok[sg * 4] = ntok;
            L.seg_tok[sg * 4 + 1] = 0;
            L.seg_tok[sg * 4 + 2] = ntok;
        }
    }
}

} // namespace pmc

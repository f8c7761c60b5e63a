// pmc_plan.hpp -- the host-side planning arithmetic of a compress call: which path claims which lengths
// (Route), where the split pipeline's chunk arrays lie (SplitLayout) and how the large values are cut
// into rounds (LvRound); and of a decompress call: which route it takes (inflate_latency), which stages
// run and every grid, group and scratch size of them (InflatePlan); and of a host-memory call: where the
// arrays of its staging lie (StageCarver, HostStage, PinnedSlot), which route it takes (plan_host_batch) and
// what a pinned call's chunks cover (plan_pinned_chunk).  Plain C++17 with no HIP in it: pmc_capi.hip and
// pmc_host.hip turn these plans into launches, and tests/host/plan_check.cpp prints them for
// tests/test_host_plan.py and tests/test_host_batch_plan.py, which need no GPU.
#pragma once
#include <assert.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/pmc_codec.h"

namespace pmc {

// ---- large-value rounds ------------------------------------------------------------------------------
// exact level (pmc_deflate_large.hip): segments of kLvSeg positions, each parsed on through kLvOverlap
// positions of the next; the hash sort works in chunks of kLvChunk positions
constexpr uint32_t kLvSeg = 16384, kLvOverlap = 2048, kLvChunk = 4096;

// One round of a call's large values: the values vals[v0 .. v1) whose tables and scratch fit the budget,
// with the layout of the table buffer (host-filled, copied to the device) and of the round scratch.
// Every region starts on a multiple of 256 bytes; a region of no elements takes no space, so the fast
// level's rounds (no pbase / ch0 / ch_val tables, no sort scratch) are the same routine's.
struct LvRound {
    const std::pair<uint32_t, uint32_t> *vals; // the call's large values (batch index, length), sorted
    uint32_t fast_seg;                         // 0: exact level; else the fast level's segment bytes
    size_t v0, v1;
    uint32_t nv;
    uint64_t nseg, nch;  // segments, sort chunks (fast: none)
    uint64_t P;          // positions, sum of len - 2 (fast: not counted, 0)
    uint64_t tb;         // tokens the segment buffers hold
    uint64_t maxlen;
    // tables: val[nv] u32 | pbase[nv] u64 | seg0[nv + 1] u32 | ch0[nv + 1] u32 | seg_val[nseg] u32 |
    // seg_tok0[nseg] u64 | ch_val[nch] u32
    uint64_t o_val, o_pbase, o_seg0, o_ch0, o_seg_val, o_seg_tok0, o_ch_val, tab_bytes;
    // scratch: tmp | S | R (4P each) | HC (P) | hist | tok | map | seg_tok | fail
    uint64_t b_tmp, b_S, b_R, b_HC, b_hist, b_tok, b_map, b_seg_tok, b_fail, scratch_bytes;

    bool exact() const { return fast_seg == 0; }
    uint64_t nseg_of(uint64_t len) const {
        return exact() ? std::max<uint64_t>(1, len / kLvSeg) : (len + fast_seg - 1) / fast_seg;
    }
    uint64_t nch_of(uint64_t len) const { return exact() ? (len - 2 + kLvChunk - 1) / kLvChunk : 0; }
    // token capacity of the value's segment j: an exact segment may parse on through the overlap (+2: the
    // positions without a hash); a fast segment has at most as many tokens as bytes
    uint64_t seg_tok_cap(uint64_t len, uint64_t j) const {
        if (exact()) return j + 1 < nseg_of(len) ? kLvSeg + kLvOverlap + 2 : len - j * kLvSeg + 2;
        return std::min<uint64_t>(fast_seg, len - j * fast_seg);
    }
    uint64_t tok_of(uint64_t len) const { // the sum of seg_tok_cap over the value's segments
        const uint64_t ns = nseg_of(len);
        return exact() ? (ns - 1) * (kLvSeg + kLvOverlap + 2) + (len - (ns - 1) * kLvSeg) + 2 : len;
    }
    // what a value adds to a round's need: its sort arrays (13 bytes per position), token buffers, state
    // maps, per-segment rows, histograms and table rows (fast: 4 bytes of tokens per byte, 32 per segment)
    uint64_t cost(uint64_t len) const {
        if (exact())
            return 13 * (len - 2) + 4 * tok_of(len) + nseg_of(len) * (2 * kLvOverlap * 4 + 16) + nch_of(len) * 1024 + 64;
        return 4 * len + nseg_of(len) * 32 + 64;
    }

    // Writes the tables at their offsets into `h` (tab_bytes bytes, 8-byte aligned).
    void fill(uint8_t *h) const {
        uint32_t *t_val = (uint32_t *)(h + o_val), *t_seg0 = (uint32_t *)(h + o_seg0), *t_ch0 = (uint32_t *)(h + o_ch0),
                 *t_sval = (uint32_t *)(h + o_seg_val), *t_cval = (uint32_t *)(h + o_ch_val);
        uint64_t *t_pb = (uint64_t *)(h + o_pbase), *t_stok = (uint64_t *)(h + o_seg_tok0);
        uint64_t pb = 0, t = 0;
        uint32_t sg = 0, ch = 0;
        for (uint32_t ov = 0; ov < nv; ov++) {
            const uint64_t len = vals[v0 + ov].second, ns = nseg_of(len), nc = nch_of(len);
            t_val[ov] = vals[v0 + ov].first;
            t_seg0[ov] = sg;
            if (exact()) {
                t_pb[ov] = pb;
                t_ch0[ov] = ch;
            }
            for (uint64_t j = 0; j < ns; j++, sg++) {
                t_sval[sg] = ov;
                t_stok[sg] = t;
                t += seg_tok_cap(len, j);
            }
            for (uint64_t c = 0; c < nc; c++, ch++) t_cval[ch] = ov;
            pb += len - 2;
        }
        t_seg0[nv] = sg;
        if (exact()) t_ch0[nv] = ch;
    }
};

// The round that starts at vals[v0] (v0 < nvals): values are taken while need + cost <= budget, and the
// first one always.  The next round starts at the returned v1.
inline LvRound lv_plan_round(const std::pair<uint32_t, uint32_t> *vals, size_t nvals, size_t v0, uint32_t fast_seg,
                             uint64_t budget) {
    LvRound r{};
    r.vals = vals;
    r.fast_seg = fast_seg;
    r.v0 = r.v1 = v0;
    uint64_t need = 0;
    while (r.v1 < nvals && (r.v1 == v0 || need + r.cost(vals[r.v1].second) <= budget)) {
        const uint64_t len = vals[r.v1].second;
        need += r.cost(len);
        if (r.exact()) r.P += len - 2;
        r.nseg += r.nseg_of(len);
        r.nch += r.nch_of(len);
        r.tb += r.tok_of(len);
        r.maxlen = std::max(r.maxlen, len);
        r.v1++;
    }
    r.nv = (uint32_t)(r.v1 - v0);
    const uint64_t nv = r.nv, ex = r.exact() ? 1 : 0;
    uint64_t o = 0;
    auto region = [&o](uint64_t bytes) { // the region's offset; `o` moves to the next region's
        const uint64_t at = o;
        o = (o + bytes + 255) & ~(uint64_t)255;
        return at;
    };
    r.o_val = region(4 * nv);
    r.o_pbase = region(ex * 8 * nv);
    r.o_seg0 = region(4 * (nv + 1));
    r.o_ch0 = region(ex * 4 * (nv + 1));
    r.o_seg_val = region(4 * r.nseg);
    r.o_seg_tok0 = region(8 * r.nseg);
    r.o_ch_val = region(4 * r.nch);
    r.tab_bytes = o;
    o = 0;
    r.b_tmp = region(4 * r.P);
    r.b_S = region(4 * r.P);
    r.b_R = region(4 * r.P);
    r.b_HC = region(r.P);
    r.b_hist = region(1024 * r.nch);
    r.b_tok = region(4 * r.tb);
    r.b_map = region(ex * 2 * kLvOverlap * 4 * r.nseg);
    r.b_seg_tok = region(16 * r.nseg);
    r.b_fail = region(4 * nv);
    r.scratch_bytes = o;
    return r;
}

// ---- member index (include/pmc_codec.h "member index") ---------------------------------------------------
#if defined(__HIPCC__)
#define PMC_HD __host__ __device__
#else
#define PMC_HD
#endif
// chunk bytes of the members this library writes (a power of two, a multiple of the fast parse's segment;
// the decoder reads every 2^12 .. 2^24 from the header)
#ifndef PMC_IDX_CHUNK
#define PMC_IDX_CHUNK 32768
#endif
constexpr uint32_t kIdxChunk = PMC_IDX_CHUNK;
constexpr uint32_t kIdxMaxChunks = 16382;          // XLEN = 8 + 4 (K - 1) fits 16 bits
constexpr uint32_t kIdxHdrFixed = 20;              // header bytes before the offsets
constexpr uint32_t kIdxSeg = 2048;                 // the fast parse's segment (kFlSeg): a chunk is whole segments
constexpr uint32_t kIdxLog2Min = 12, kIdxLog2Max = 24;
static_assert((kIdxChunk & (kIdxChunk - 1)) == 0 && kIdxChunk >= (1u << kIdxLog2Min) && kIdxChunk <= (1u << kIdxLog2Max),
              "index chunk size");

// chunk CRCs (include/pmc_codec.h "member index", chunk CRCs): a second FEXTRA subfield 'P' 'C' of 8 + 4 K bytes
// directly behind the 'P' 'I' one; XLEN = 8 K + 12 fits 16 bits
constexpr uint32_t kIdxCrcMaxChunks = 8190;
constexpr uint32_t kIdxCrcFixed = 8;               // the subfield's bytes before its K entries

// What the index switch makes of a fast-all value of `len` bytes with chunks of C bytes (C 0: switch off):
// K chunks behind a header of hdr bytes when indexed, else the plain member (K 1, hdr 10).  With the chunk-CRC
// switch (crc) an indexed value of K <= kIdxCrcMaxChunks chunks also carries their CRC-32s (crcs), at byte
// crc_at of the member; a longer one stays the plain indexed member.
struct IdxPlan {
    bool indexed;
    uint32_t K, hdr;
    bool crcs;
    uint32_t crc_at;
};
PMC_HD inline IdxPlan idx_plan(uint64_t len, uint32_t C, bool crc = false) {
    IdxPlan p{false, 1, 10, false, 0};
    if (C == 0 || len <= C) return p;
    const uint64_t K = (len + C - 1) / C;
    if (K > kIdxMaxChunks) return p;
    p.indexed = true;
    p.K = (uint32_t)K;
    p.hdr = kIdxHdrFixed + 4 * (p.K - 1);
    if (crc && p.K <= kIdxCrcMaxChunks) {
        p.crcs = true;
        p.crc_at = p.hdr + kIdxCrcFixed;
        p.hdr = p.crc_at + 4 * p.K;
    }
    return p;
}

// The index a member carries, by the rules of inflate_chunk_scan_kernel (all but the capacity one): bytes
// 0..3 = 1f 8b 08 04, the first FEXTRA subfield 'P' 'I' of version 1 with XLEN >= LEN + 4, LEN = 4 + 4 (K - 1),
// reserved bytes 0, 12 <= log2 C <= 24, K = ceil(ISIZE / C) >= 2, offsets strictly increasing from behind
// the header to below len - 8.  *hdr: the first byte behind the header.  (P: any pointer to bytes)
template <class P>
PMC_HD inline bool idx_parse(P m, uint64_t len, uint32_t *log2c, uint32_t *K, uint32_t *isize, uint32_t *hdr) {
    if (len < kIdxHdrFixed + 4 + 8 + 1) return false;
    if (m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) return false;
    const uint32_t xlen = (uint32_t)m[10] | (uint32_t)m[11] << 8, sl = (uint32_t)m[14] | (uint32_t)m[15] << 8;
    if (m[12] != 'P' || m[13] != 'I' || sl < 8 || (sl & 3) != 0 || xlen < sl + 4) return false;
    if (m[16] != 1 || m[18] != 0 || m[19] != 0) return false;
    const uint32_t lg = m[17], k = sl / 4, h = 12 + xlen;
    if (lg < kIdxLog2Min || lg > kIdxLog2Max || (uint64_t)h + 8 >= len) return false;
    const uint32_t isz = (uint32_t)m[len - 4] | (uint32_t)m[len - 3] << 8 | (uint32_t)m[len - 2] << 16 |
                         (uint32_t)m[len - 1] << 24;
    if (k < 2 || (uint32_t)(((uint64_t)isz + (1u << lg) - 1) >> lg) != k) return false;
    uint64_t prev = h;
    for (uint32_t j = 0; j + 1 < k; j++) {
        const uint32_t at = kIdxHdrFixed + 4 * j;
        const uint64_t o = (uint32_t)m[at] | (uint32_t)m[at + 1] << 8 | (uint32_t)m[at + 2] << 16 | (uint32_t)m[at + 3] << 24;
        if (o <= prev || o + 8 >= len) return false;
        prev = o;
    }
    *log2c = lg;
    *K = k;
    *isize = isz;
    *hdr = h;
    return true;
}

// The chunk CRCs a member carries: idx_parse holds, and the subfield 'P' 'C' lies directly behind the 'P' 'I'
// one (at byte 16 + LEN_PI) and wholly inside the FEXTRA field, with LEN = 4 + 4 K, version 1 and three reserved
// bytes 0.  *crc_at: the byte of chunk 0's entry (K entries of u32 LE follow).  Any other member carries none.
// (idx_crc_sub: the subfield's own rules, for a member whose idx_parse gave k chunks and the header's end hdr)
template <class P>
PMC_HD inline bool idx_crc_sub(P m, uint32_t k, uint32_t hdr, uint32_t *crc_at) {
    const uint32_t p = 16 + 4 * k; // (LEN_PI = 4 k)
    if ((uint64_t)p + kIdxCrcFixed + 4 * (uint64_t)k > hdr) return false;
    if (m[p] != 'P' || m[p + 1] != 'C' || ((uint32_t)m[p + 2] | (uint32_t)m[p + 3] << 8) != 4 + 4 * k) return false;
    if (m[p + 4] != 1 || m[p + 5] != 0 || m[p + 6] != 0 || m[p + 7] != 0) return false;
    *crc_at = p + kIdxCrcFixed;
    return true;
}
template <class P>
PMC_HD inline bool idx_crc_parse(P m, uint64_t len, uint32_t *K, uint32_t *crc_at) {
    uint32_t lg, k, isz, hdr;
    if (!idx_parse(m, len, &lg, &k, &isz, &hdr) || !idx_crc_sub(m, k, hdr, crc_at)) return false;
    *K = k;
    return true;
}

// ---- ranged reads (include/pmc_codec.h "ranged reads"; pmc_inflate_range.hip) ----------------------------
// the largest chunk a ranged read serves: the three sizes the library can be built with, and an edge row of
// 64 KiB
constexpr uint32_t kRangeLog2Max = 16;
// an edge row: one chunk, and the 16 bytes LaneOut::get8's three-dword reads may reach past a position
constexpr uint64_t kRangeRowBytes = (1ull << kRangeLog2Max) + 16;
// all the edge rows of a call, whatever its n (allocated as far as a call's plan needs them, and then kept by
// the context until pmc_ctx_destroy: its buffers grow and never shrink).  The budget cuts the range kernel's
// grid, one row per lane, so it is a trade of HBM against decode rate: 2 GiB is 511 blocks, two thirds of the
// resident lanes of a 256-CU device at three waves per CU; a call of n <= 16379 requests plans 2 n rows
// (125 MiB for 1000) and is not cut
constexpr uint64_t kRangeScratchBudget = 2048ull << 20;
// the device scratch the store's fallback (whole reads of the extents the ranged call declined) uses per round;
// an extent larger than this gets a round of its own
constexpr uint64_t kRangeFallbackBudget = 64ull << 20;

// The bytes [o, o + L) a request for [off, off + len) of a value of isize bytes gets (Redis GETRANGE: a range
// that reaches past the end is shortened, one that starts at or past it is empty), and the chunks of 2^lg bytes
// that hold them: k0 .. k0 + items - 1 (L 0: none).  No 32-bit wrap: off + len may exceed 2^32.
struct RangeOf {
    uint32_t o, L, k0, items;
};
PMC_HD inline RangeOf range_of(uint32_t isize, uint32_t lg, uint32_t off, uint32_t len) {
    RangeOf r{};
    r.o = off < isize ? off : isize;
    r.L = len < isize - r.o ? len : isize - r.o;
    if (r.L == 0) return r;
    r.k0 = r.o >> lg;
    r.items = (uint32_t)(((uint64_t)r.o + r.L - 1) >> lg) - r.k0 + 1;
    return r;
}

// A ranged call over n requests.  Rows as the chunk pass's (InflatePlan::Idx), then the edge rows: a chunk that
// the range covers only in part is decoded whole into a row, and its slice copied out.  A request has at most
// two such chunks.  While 2 n rows fit the budget every request owns rows 2 i and 2 i + 1 and the range kernel
// runs at the resident waves; a larger call gives every lane of the grid a row, reused across its grid-stride
// loop, and cuts the grid to the rows the budget holds.  So the edge rows never exceed kRangeScratchBudget.
struct RangePlan {
    uint32_t mb, cb;   // blocks of 256 of the request kernels (scan, finish); blocks of 64 of the range kernel
    bool row_per_request;
    uint64_t rows;
    struct Idx {
        uint64_t cnt, fail, pre, bsum, total, bytes;
    } idx;
    uint64_t rows_off, edge_bytes, bytes; // the rows' offset (16-byte aligned), their bytes, the whole scratch
};
inline RangePlan plan_range(uint64_t n, uint64_t cus, uint64_t range_per_cu, uint64_t scan_block) {
    RangePlan P{};
    const uint64_t max_rows = kRangeScratchBudget / kRangeRowBytes;
    const uint64_t resident = std::max<uint64_t>(1, cus * range_per_cu);
    const uint64_t need = (std::min<uint64_t>(n, 1ull << 32) * kIdxMaxChunks + 63) / 64;
    P.mb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, cus * 8));
    P.row_per_request = 2 * n <= max_rows;
    uint64_t cb = std::max<uint64_t>(1, std::min(need, resident));
    if (!P.row_per_request) cb = std::max<uint64_t>(1, std::min(cb, max_rows / 64));
    P.cb = (uint32_t)cb;
    P.rows = P.row_per_request ? 2 * n : cb * 64;
    const uint64_t nb = (n + scan_block - 1) / scan_block;
    P.idx.cnt = 0;
    P.idx.fail = 4 * n;
    P.idx.pre = (8 * n + 7) & ~(uint64_t)7;
    P.idx.bsum = P.idx.pre + 8 * n;
    P.idx.total = P.idx.bsum + 8 * nb;
    P.idx.bytes = P.idx.total + 8;
    P.rows_off = (P.idx.bytes + 15) & ~(uint64_t)15;
    P.edge_bytes = P.rows * kRangeRowBytes;
    P.bytes = P.rows_off + P.edge_bytes;
    return P;
}

// ---- split pipeline chunk arrays (DeflateArgs cT .. cQ; pmc_deflate_split.hip) -------------------------
constexpr uint32_t kSplitRows = 336;  // 286 lit/len + 30 dist + 19 bit-length (+1)
constexpr uint32_t kMergeRows = 572;  // 2 heap entries per merge, <= 285 merges
// a dynamic block's tree header (HLIT..send_tree, at most 14 + 19 * 3 + 316 * 7 = 2283 bits): word 0 the
// bit count, then the bits LSB-first (76 words: 16-byte rows)
constexpr uint32_t kHdrWords = 76;
// lane-inflate / trees visit order: indices grouped into this many bins (by compressed length, so a
// wave's 64 lanes decode members of similar length and finish their decode loops together; by used symbols)
constexpr uint32_t kOrderBins = 2048;

// The one statement of where a chunk's arrays lie in the context's split scratch: byte offsets for a
// pass of cap `pcap` over chunks of `chunk` values (a multiple of 64).  The rows of cH / cL / cB / cG
// are per value, `chunk` of them.  cB's 16-byte rows are aligned because every array before it is a
// multiple of 16 bytes per 64 values.
struct SplitLayout {
    uint64_t cT, cN, cP, cG, cH, cL, cB, cC, cD, cZ, ord, obins, cQ;
    SplitLayout(uint64_t pcap, uint64_t chunk) {
        uint64_t o = 0;
        auto array = [&o](uint64_t bytes) {
            const uint64_t at = o;
            o += bytes;
            return at;
        };
        cT = array(chunk * pcap * 4);
        cN = array(chunk * 4);
        cP = array(chunk * 4);
        cG = array(chunk * kMergeRows * 4);
        cH = array(chunk * kSplitRows * 2);
        cL = array(chunk * kSplitRows);
        cB = array(chunk * kHdrWords * 4);
        cC = array(chunk * 4);
        cD = array((chunk + 1) * 4); // (+1: the number of deferred values)
        cZ = array(chunk * 4);
        ord = array(chunk * 4);
        obins = array(kOrderBins * 4);
        cQ = o; // the two work counters
    }
    // the scratch a pass needs: the arrays, cQ's 64 bytes and 1 KiB of slack
    uint64_t bytes() const { return cQ + 64 + 1024; }
};

// What the chunk budget is divided by to get the values per chunk: the per-value arrays that dominated
// when the budget was calibrated -- not the footprint (SplitLayout::bytes() is; it also holds cB, cC,
// cZ and ord).  Chunk sizes are behaviour: tests/test_gpu_fullsize.py sizes its budgets by this.
inline uint64_t split_value_bytes(uint64_t cap) {
    return cap * 4 + 4 + kSplitRows * 2 + kSplitRows + 4 + kMergeRows * 4 + 4 + 8;
}
// values per chunk of a pass of cap `cap` over a batch of n (a multiple of 64, at least 4096 unless n is less)
inline uint64_t split_chunk_of(uint64_t n, uint64_t budget, uint64_t cap) {
    const uint64_t ch = std::min<uint64_t>(n, std::max<uint64_t>(4096, budget / split_value_bytes(cap)));
    return (ch + 63) & ~(uint64_t)63;
}

// ---- the compress route ----------------------------------------------------------------------------------
// the levels whose values of <= 16382 bytes take the fast front (PMC_LEVEL_FAST_ALL: the longer ones too)
inline bool level_is_fast(int level) { return level == PMC_LEVEL_FAST || level == PMC_LEVEL_FAST_ALL; }

// the longest value a dictionary of D bytes is used for (D + len <= 16382)
constexpr uint32_t kDictSpan = 16382;

struct RouteIn {
    uint64_t n, max_len;  // values in the batch; the caller's bound on their lengths (>= 1)
    int level;            // PMC_LEVEL_*
    bool lane_order_ok;   // the context's create-time probe passed
    uint32_t dict_len;    // the context's dictionary (0: none)
    uint64_t cus;
    bool latency, small;  // the host calls' latency path; a device-resident batch within its limits
    bool force_v1, mono_env; // PMC_DEFLATE_V1, PMC_DEFLATE_MONO
    int big_env;          // PMC_BIG_PASS: 1 / 0 forces the large pass on / off, -1 unset
    // deflate_small_limit(), deflate_big_limit(), deflate_lds_limit() (they follow the kernels' LDS layouts)
    uint64_t small_lim, big_lim, v1_lim;
    uint64_t single_block_max; // kSmallMax: a longer value may need several DEFLATE blocks
    uint64_t hbm_wb;           // the HBM kernel's working set per wave at max_len
};

// one pass of the split pipeline over the batch: the values with lo < len <= hi, working sets sized for
// pcap (dictp: the fast front behind the context's dictionary; its LDS layout follows D + hi, the token
// slabs, trees and back pcap as ever -- a value has at most len tokens)
struct SplitPass {
    uint64_t lo, hi, pcap;
    bool fastp, dictp;
};

// Which path claims which lengths of (0, max_len].  kSplit: `pass[0 .. npass)`; kMono / kV1: one kernel
// for (0, lds_cut] (deflate_small_kernel / deflate_kernel<false>).  Above hbm_cut: the large-value rounds
// (lv), or on the V1 path the HBM kernel by length (!gated).  Otherwise the HBM kernel runs gated, as
// the retry pass, with hbm_waves waves (0: no pass).
struct Route {
    enum Kind { kSplit, kMono, kV1 } kind;
    SplitPass pass[3];
    int npass;
    uint64_t lds_cut, cap; // kMono / kV1: the kernel's longest value and its working-set cap
    uint32_t dict_len;     // the dictionary the dictionary pass uses (0: no such pass)
    bool lv, fast_all;     // large-value rounds run; at the fast level (large_values' mode)
    uint64_t hbm_cut;
    bool gated, rlist;     // rlist: the call needs a retry list (a gated pass will run)
    uint64_t hbm_waves;
};

inline Route plan_route(const RouteIn &in) {
    Route R{};
    const uint64_t n = in.n, max_len = in.max_len;
    const bool force_v1 = in.force_v1;
    // Values <= small_lim (16382): the split pipeline's small pass; 16382 < len <= big_lim (~31.9K,
    // the front's 160 KiB LDS; MAX_DIST caps it at 32506): its large pass; the rest -- and
    // large-pass values of >= 16383 symbols, which need several DEFLATE blocks -- the general
    // kernel with its working set in HBM (pmc_deflate.hip).  PMC_DEFLATE_V1=1 routes everything
    // through the general kernels (A/B and safety net); PMC_DEFLATE_MONO=1 the single-kernel path.
    // (a context whose lane-order probe failed compresses through the single-kernel path, whose
    // sort and codes use per-lane counters and ballots instead of returning-atomic ranks)
    // (small: a device-resident batch within the latency path's limits -- the one-kernel path, as for
    // host calls, but with the argument check and the retry pass of the device-resident API)
    // Fast level: every value of <= 16382 bytes goes through the split pipeline with the fast front, whatever
    // the batch (so a value's member does not depend on the entry point); longer values take the paths below
    // unchanged.  (PMC_DEFLATE_V1, the A/B safety net, stays exact.)
    // PMC_LEVEL_FAST_ALL: the same for values of <= 16382 bytes; every longer value goes to the large-value
    // rounds' fast mode (segments through the fast front), so the batch-dependent large pass below is off.
    const bool fast = level_is_fast(in.level) && in.lane_order_ok && !force_v1;
    R.fast_all = fast && in.level == PMC_LEVEL_FAST_ALL;
    // With a dictionary (fast level only): values of D + len <= 16382 take the dictionary front, a pass of
    // its own by length; longer ones the plain fast front (a second pass) or the exact paths, as without one.
    R.dict_len = fast ? in.dict_len : 0u;
    const bool mono = !fast && (in.mono_env || in.latency || in.small || !in.lane_order_ok);
    const bool split = !force_v1 && !mono;
    R.kind = split ? Route::kSplit : force_v1 ? Route::kV1 : Route::kMono;
    const uint64_t small_lim = force_v1 ? 0 : in.small_lim;
    const uint64_t big_lim = split ? in.big_lim : small_lim;
    R.lds_cut = std::min<uint64_t>(force_v1 ? in.v1_lim : small_lim, std::max<uint64_t>(max_len, 1));
    R.cap = std::min<uint64_t>((R.lds_cut + 63) & ~(uint64_t)63, force_v1 ? in.v1_lim : small_lim);
    // large pass: values in (small_lim, big_hi]
    // The split pipeline's large pass (16382 < len <= ~31.8K through the front at one wave per CU, the
    // front's working set filling the CU's LDS) is off since round 5: the large-value pipeline compresses
    // these values 1.8x faster (100K x 30 KB: 1.55 -> 2.84 GiB/s, 500K x 20 KB 1.58 -> 3.07, same box,
    // profiles/r05/large) -- except in small batches: one wave per value of the large pass finishes a
    // lone 30 KB value in ~5 ms, the large-value pipeline's two 16 KiB segment parses (global-memory
    // chains) in ~10 ms, so batches of up to 2 values per CU that hold no value above the large pass's
    // limit keep it (a batch with longer values runs the large-value pipeline anyway and sends all its
    // values above small_lim there).  PMC_BIG_PASS=1 / 0 forces it on / off.
    const bool big_pick = in.big_env >= 0 ? in.big_env != 0 : n <= 2 * in.cus && max_len <= big_lim;
    const bool big_pass = split && !R.fast_all && big_pick && max_len > small_lim && big_lim > small_lim;
    const uint64_t big_hi = big_pass ? std::min<uint64_t>(big_lim, max_len) : 0;
    R.hbm_cut = big_pass ? big_hi : R.lds_cut; // the HBM kernel takes lengths above this
    if (split) {
        if (R.dict_len) {
            // (the dictionary pass: its values' lengths and the cap of its token slabs and back)
            const uint64_t dict_hi = std::min<uint64_t>(R.lds_cut, kDictSpan - R.dict_len);
            R.pass[R.npass++] = {0, dict_hi, std::min<uint64_t>(R.cap, (dict_hi + 63) & ~(uint64_t)63), true, true};
            if (R.lds_cut > dict_hi) R.pass[R.npass++] = {dict_hi, R.lds_cut, R.cap, true, false};
        } else {
            R.pass[R.npass++] = {0, R.lds_cut, R.cap, fast, false};
        }
        if (big_pass)
            R.pass[R.npass++] = {small_lim, big_hi, std::min<uint64_t>((big_hi + 63) & ~(uint64_t)63, big_lim), false,
                                 false};
    }
    // values above hbm_cut: the large-value path (pmc_deflate_large.hip), except on the V1 A/B path
    R.lv = !force_v1 && max_len > R.hbm_cut;
    // The HBM kernel takes values by length only on the V1 path.  Otherwise it runs gated, as the retry
    // pass of the values this call's other paths declined (a lane-order guard fired, a large-pass value
    // of several blocks, a large value whose segments did not stitch): it visits the call's retry list
    // (DeflateArgs::rlist) and returns at once when the list is empty.  The latency path launches no
    // retry pass: host_batch reads the verdicts and redoes a declined call through the pipeline.
    R.gated = !(force_v1 && max_len > R.hbm_cut);
    if (!R.gated || !in.latency) {
        // as many waves as the kernel's 196 VGPRs let a CU hold (2 per SIMD) within a scratch budget
        // (32 GiB for the V1 path's length-routed values; 8 GiB for retries, whose waves exit at once
        // when there are none): at 2 waves per CU (round 1-2) the latency-bound walk left 64 KiB values
        // at 0.52 GiB/s, and a 64-wave retry pass left periodic 1 MiB values and multi-block 24 KB
        // values 32x short of that
        // A batch of single-block values (max_len <= kSmallMax) can have retries only from a lane-order
        // guard, which never fired on gfx950 (and a context whose create-time probe sees the order broken
        // sends every batch to the per-lane-counter kernels instead): 64 waves, and 64 waves' scratch,
        // cover that.  Only batches with longer values (multi-block large-pass values, large values whose
        // segments did not stitch) size the pass for throughput (the scratch a gated pass
        // allocates stays with the context).
        const uint64_t cap_waves = R.gated && max_len <= in.single_block_max ? 64ull : in.cus * 8;
        R.hbm_waves = std::max<uint64_t>(
            1, std::min<uint64_t>(cap_waves, ((R.gated ? 8ull : 32ull) << 30) / std::max<uint64_t>(in.hbm_wb, 1)));
    }
    R.hbm_waves = std::min<uint64_t>(R.hbm_waves, n);
    R.rlist = R.gated && R.hbm_waves;
    return R;
}

// ---- the decompress plan ---------------------------------------------------------------------------------
// Worst case gzip member size (same formula as oracle_gzip_bound): stored fallback adds
// 5 B per 16383-symbol block; after a window slide fixed/dynamic blocks stay <= 9/8 len.
PMC_HD inline uint64_t gzip_bound(uint64_t len) { return len + (len >> 3) + 6 * (len / 16383 + 1) + 32; }

// ---- ranged writes (include/pmc_codec.h "ranged writes"; pmc_deflate_patch.hip) --------------------------
// The bytes [off, off + len) of a value of isize bytes that a patch replaces (no growth: ok is false when the
// patch reaches past the end; no 32-bit wrap), and the chunks of 2^lg bytes it touches: a .. b (len 0: none).
// A touched chunk the patch covers only in part is an edge chunk (decoded before the patch is laid over it):
// edge_a is chunk a, edge_b is chunk b where b != a.
struct PatchOf {
    bool ok;
    uint32_t a, b, items;
    bool edge_a, edge_b;
};
PMC_HD inline PatchOf patch_of(uint32_t isize, uint32_t lg, uint32_t off, uint32_t len) {
    PatchOf p{};
    p.ok = (uint64_t)off + len <= isize;
    if (!p.ok || len == 0) return p;
    const uint64_t end = (uint64_t)off + len, C = 1ull << lg;
    p.a = off >> lg;
    p.b = (uint32_t)((end - 1) >> lg);
    p.items = p.b - p.a + 1;
    const uint64_t be = ((uint64_t)p.b + 1) * C < isize ? ((uint64_t)p.b + 1) * C : isize; // chunk b's end
    const bool head = (off & (C - 1)) != 0, tail = end != be;
    p.edge_a = head || (p.a == p.b && tail);
    p.edge_b = p.a != p.b && tail;
    return p;
}

// The same for a write that may make the value longer (include/pmc_codec.h "growing writes"): the patch's bytes
// become [off, off + len) of a value of S2 = max(isize, off + len) bytes in K2 chunks, with zeros in [isize, off).
// verdict: kGrowServe -- touched chunks a .. a + items - 1; kGrowSame -- an empty patch, the member as it is,
// whatever off is; kGrowArg -- S2 would not fit ISIZE; kGrowNoIndex -- K2 chunks are more than a member with chunk
// CRCs may have.  Within the value (off + len <= isize) everything is patch_of's.  A growing write touches every
// chunk from a = min(off >> lg, K - 1) on, the old last chunk always (it stops being the last); chunk a is its
// only edge chunk, and is one where some of its old bytes survive: min(off, isize) > a 2^lg.
enum : uint32_t { kGrowServe = 0, kGrowSame = 1, kGrowArg = 2, kGrowNoIndex = 3 };
struct GrowOf {
    uint32_t verdict;
    bool grows;
    uint32_t S2, K2;
    uint32_t a, b, items;
    bool edge_a, edge_b;
};
PMC_HD inline GrowOf grow_of(uint32_t isize, uint32_t lg, uint32_t off, uint32_t len) {
    GrowOf g{};
    const uint64_t end = (uint64_t)off + len, C = 1ull << lg;
    g.S2 = isize;
    g.K2 = (uint32_t)(((uint64_t)isize + C - 1) >> lg);
    if (len == 0) {
        g.verdict = kGrowSame;
        return g;
    }
    if (end <= isize) {
        const PatchOf p = patch_of(isize, lg, off, len);
        g.a = p.a, g.b = p.b, g.items = p.items, g.edge_a = p.edge_a, g.edge_b = p.edge_b;
        return g;
    }
    g.grows = true;
    if (end > 0xFFFFFFFFull) {
        g.verdict = kGrowArg;
        return g;
    }
    const uint32_t K = g.K2;
    g.S2 = (uint32_t)end;
    g.K2 = (uint32_t)((end + C - 1) >> lg);
    if (g.K2 > kIdxCrcMaxChunks) {
        g.verdict = kGrowNoIndex;
        return g;
    }
    g.a = K && (off >> lg) > K - 1 ? K - 1 : off >> lg;
    g.b = g.K2 - 1;
    g.items = g.K2 - g.a;
    g.edge_a = (off < isize ? off : isize) > (uint64_t)g.a << lg;
    return g;
}

// The member's CRC-32 folded from its K chunk CRCs as crc32_combine does, chunk lengths from isize and C = 2^lg:
// crc = crc * x^(8 clen) + e[k] in GF(2)[x] mod P, reflected (the host form of the emit kernel's recurrence).
inline uint32_t crc_multmodp_host(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) {
        p ^= ((a >> k) & 1u) ? b : 0u;
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}
inline uint32_t crc_x8n_host(uint64_t n) { // x^(8 n) mod P
    uint32_t r = 0x80000000u, sq = 0x00800000u; // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1) r = crc_multmodp_host(sq, r);
        sq = crc_multmodp_host(sq, sq);
    }
    return r;
}
inline uint32_t crc_fold_host(const uint32_t *e, uint32_t K, uint32_t isize, uint32_t lg) {
    uint32_t crc = 0;
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t c0 = (uint64_t)k << lg;
        const uint64_t clen = isize - c0 < (1ull << lg) ? isize - c0 : (1ull << lg);
        crc = crc_multmodp_host(crc_x8n_host(clen), crc) ^ e[k];
    }
    return crc;
}

// A rewrite call over n requests.  Per request 44 bytes of rows (the scan's verdict state, the prefix sum of the
// touched chunks, the parse's tables).  The touched chunks are worked on in rounds of whole requests, at most
// kPatchRoundChunks chunks each (a request has at most kIdxCrcMaxChunks, so every request fits a round); a round's
// scratch per chunk is the staged bytes (C), the parse's token buffers (4 C, and 28 bytes per segment), the
// emitted span's slot (gzip_bound(C) + 16, rounded to 16) and two words, and per emitting wave a symbol slab --
// within kPatchScratchBudget whatever n and the patches are.
constexpr uint64_t kPatchRoundChunks = 8192;
constexpr uint64_t kPatchScratchBudget = 2048ull << 20;
constexpr uint64_t kPatchSlabBytes = 65536;  // (kSlabSyms u32: pmc_kernels.hpp)
constexpr uint64_t kPatchMaxWaves = 2048;    // emitting waves of a round
// (gzip_bound(kIdxChunk) + 16, rounded to 16: the large-value emit's image of a value of one chunk)
constexpr uint64_t kPatchSlotBytes =
    ((uint64_t)kIdxChunk + (kIdxChunk >> 3) + 6 * (kIdxChunk / 16383 + 1) + 32 + 16 + 15) & ~(uint64_t)15;
constexpr uint32_t kPatchSegs = kIdxChunk / kIdxSeg; // the parse's segments per chunk
static_assert(kPatchRoundChunks >= kIdxCrcMaxChunks, "a request's touched chunks fit one round");
struct PatchPlan {
    uint32_t mb; // blocks of 256 of the request kernels
    // rows per request: cnt | ka | fail | pfail | lv_val | seg0 | rlen (u32 each), roff | pre (u64 each), then
    // scan_u32's block sums and the total
    uint64_t cnt, ka, fail, pfail, lv_val, seg0, rlen, roff, pre, bsum, total, bytes;
};
inline PatchPlan plan_patch(uint64_t n, uint64_t cus, uint64_t scan_block) {
    PatchPlan P{};
    P.mb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, cus * 8));
    const uint64_t nb = (n + scan_block - 1) / scan_block;
    P.cnt = 0;
    P.ka = 4 * n;
    P.fail = 8 * n;
    P.pfail = 12 * n;
    P.lv_val = 16 * n;
    P.seg0 = 20 * n;
    P.rlen = 24 * n;
    P.roff = (28 * n + 7) & ~(uint64_t)7;
    P.pre = P.roff + 8 * n;
    P.bsum = P.pre + 8 * n;
    P.total = P.bsum + 8 * nb; // (scan_u32: bsum[nb] is the total)
    P.bytes = P.total + 8;
    return P;
}
// A round of `items` touched chunks (<= kPatchRoundChunks) emitted by `waves` waves.
struct PatchRound {
    uint64_t waves;
    uint64_t stage, tok, seg_val, seg_tok0, seg_tok, slots, span, crc, slabs, bytes;
};
inline PatchRound plan_patch_round(uint64_t items, uint64_t cus) {
    PatchRound R{};
    items = std::max<uint64_t>(1, items);
    R.waves = std::max<uint64_t>(4, std::min<uint64_t>({(items + 3) / 4 * 4, cus * 8, kPatchMaxWaves}));
    uint64_t o = 0;
    auto region = [&o](uint64_t bytes) {
        const uint64_t at = o;
        o = (o + bytes + 255) & ~(uint64_t)255;
        return at;
    };
    R.stage = region(items * kIdxChunk + 4096); // (the parse's staging and the decoder read a few bytes past a chunk)
    R.tok = region(items * kIdxChunk * 4);
    R.seg_val = region(items * kPatchSegs * 4);
    R.seg_tok0 = region(items * kPatchSegs * 8);
    R.seg_tok = region(items * kPatchSegs * 16);
    R.slots = region(items * kPatchSlotBytes);
    R.span = region(items * 4);
    R.crc = region(items * 4);
    R.slabs = region(R.waves * kPatchSlabBytes);
    R.bytes = o;
    return R;
}

// The one statement of the wave-only route: the batches that go through the wave-per-member kernels alone
// instead of the lane / record pipeline (InflateIn::latency).  lat_batch / lat_max_len: the compress side's
// latency limits (1,024 values of 4 KiB; PMC_LATENCY_BATCH / PMC_LATENCY_MAX_LEN, 0 disables the path);
// out_limit: the LDS wave kernel's output image (48 KiB), the decompress side's length limit.  A host call
// passes the sum of its capacities as out_bytes, the device-resident entry n * max_len.
// The batch limit is 4x the compress side's, with at most 4x the output in all (4,096 x 4 KiB members: 0.81 ms
// device-resident through the wave kernel against 1.69 ms through the pipeline; compress at 4,096 x 4 KiB is
// faster through the pipeline, 2.86 against 3.33 ms -- round 5, same box).
// device_call: a server-sized GET batch (<= 4,096 members, capacities within the wave kernel's LDS image and
// <= 16 MiB of output in all, the host calls' limits) takes the wave-per-member kernel alone there too
// (whole-wave Huffman decode per member instead of one lane's; 400 x 4 KiB: 1.47 -> ~0.5 ms, round 5), then
// the HBM variant for anything it declined (the lengths are device-resident).  A device-resident batch of at
// most 4 members per CU also takes the wave kernels whatever its sizes: one wave per member beats one lane
// per member until the lanes' density pays (1000 x 1 MiB: 220 ms against 453 ms through the multi-block lane
// pass; 40K x 64 KiB: 542 ms against 25 ms -- round 5, same box).  (PMC_LATENCY_BATCH=0 turns both clauses
// off, so A/B runs and fault tests can still reach the lane / record pipeline with small batches -- ADVICE r5)
inline bool inflate_latency(uint64_t n, uint64_t max_len, uint64_t out_bytes, uint64_t cus, uint64_t lat_batch,
                            uint64_t lat_max_len, bool device_call, uint64_t out_limit) {
    const uint64_t lb = 4 * lat_batch, lm = lat_max_len;
    const uint64_t max_out = lm ? std::max(lm, out_limit) : 0;
    if (n <= lb && max_len <= max_out && (max_len <= lm || out_bytes <= lb * lm)) return true;
    return device_call && lat_batch != 0 && n <= 4 * cus;
}

struct InflateIn {
    uint64_t n, max_len;  // members in the batch (>= 1); the caller's bound on their decompressed sizes
    uint64_t cus;
    bool latency;         // the wave-only route (inflate_latency)
    bool need_hbm;        // false: a host-memory caller says no member needs more than the LDS pass (inflate_need_hbm)
    uint32_t dict_len;    // the context's dictionary (0: it has no dictionary id)
    bool wave_only, no_order, no_rec; // PMC_INFLATE_WAVE=1, PMC_INFLATE_ORDER=0, PMC_INFLATE_REC=0
    // resident blocks per CU, as the runtime says: inflate_rec_kernel<1024>, <kRecOutMax>, inflate_chunk_kernel
    uint64_t rec_per_cu_1k, rec_per_cu_4k, chunk_per_cu;
    // the kernels' own constants: kRecMax, kRecOutMax, scan_u32's block (1024), the LDS wave kernel's largest
    // output image (48 KiB)
    uint64_t rec_max, rec_out_max, scan_block, out_limit;
};

// Which stages of a decompress call run, with their grids, groups and scratch sizes.  Grids and sizes are
// stated for every call, whether or not the stage they belong to runs.
struct InflatePlan {
    // lane_route: the lane-per-member fast paths (order, record, lane passes), then the CRC check; whatever
    // they decline (rc = kInflateRetry) goes through the wave-per-member kernels.  Off on the wave-only route
    // and with PMC_INFLATE_WAVE=1 (everything through the wave kernels).
    // (round 4 measured routing batches of <= 2048 members to the wave kernels instead: 256 x 4 KiB took
    // 12.5 ms there against 3.2 ms for 4096 members through the lane / record paths -- not done)
    bool lane_route;
    // The chunk pass over indexed members runs in every call that may hold one (a member of more than one
    // chunk decodes to more than kIdxChunk bytes), on either route; with PMC_INFLATE_WAVE=1 it is off, like
    // the other fast paths.  A call with max_len <= kIdxChunk launches nothing for it.
    // chunk_all: the wave-only route (a small batch, or at most 4 members per CU -- where 1000 x 1 MiB lands):
    // the pass looks at every member, takes the indexed ones and marks every other one kInflateRetry; on the
    // lane route it looks at those the lane passes left kInflateRetry.
    bool chunk_pass, chunk_all;
    bool order;       // visit order by compressed length (PMC_INFLATE_ORDER=0: index order)
    // members of <= rec_max_out output bytes: the two-phase record kernel, one block per resident wave (each
    // block owns 64 record rows); larger ones: the lane kernel (PMC_INFLATE_REC=0: all of them)
    bool rec;
    // members of several blocks exist only above 16383 output bytes (zlib flushes every 16383 symbols): then
    // a third lane pass decodes them block after block
    bool multi_pass;
    bool verify;      // the CRC check of the members the lane decoders and the chunk pass finished
    bool dict_second; // the second LDS pass, sized for the longest dictionary member (below)
    bool hbm;         // the wave kernels' HBM variant
    // the wave kernels take only members a stage before them marked kInflateRetry; those they decode are
    // counted (pmc_ctx_guard_counts counts[4]: the lane route's, the wave-only route's chunk pass is uncounted)
    bool retry_only, count_retried;

    uint32_t ob;      // order kernels: blocks of 256
    uint32_t lb;      // lane kernels: blocks of 64
    // record kernel: the 1 KiB image instance when no member may decode to more (max_len: the largest
    // capacity), else the 4 KiB one; rstride records per row.  rb: exactly the resident blocks -- a block owns
    // its rows for the whole grid-stride loop, and blocks beyond residency would start only when the first
    // ones have finished.  G, members per grab: the smallest power of two whose grabs fit the resident blocks
    // once, so a small batch (a server's few hundred GETs) spreads one or a few members per wave instead of
    // 64 on a few CUs with phase B's member-serial loop exposed.
    bool out1k;
    uint32_t rstride, G, rb, rec_max_out;
    // verify kernel: members per wave as for the record kernel (a small batch takes one wave per member);
    // blocks of 512
    uint32_t VG, vb;
    // chunk pass: blocks of 256 of its member kernels (scan, finish, count); blocks of 64 of the chunk kernel
    // (the item count stays on the device: a grid of the resident waves strides over the items, and returns
    // at once when there are none)
    uint32_t mb, cb;
    uint64_t hbm_waves;
    uint32_t hbm_blocks; // of 4 waves
    // scratch bytes: CRC-32 trailers, visit order (bins | member indices), record rows, the record kernel's
    // list (count | members)
    uint64_t crcx_bytes, order_bytes, recs_bytes, bigl_bytes;
    // the chunk pass's rows in the context's idx buffer (byte offsets): cnt[n] u32 | fail[n] u32 | pre[n] u64 |
    // bsum[nb] u64 (scan_u32's block sums, one per scan_block members) | total u64
    struct Idx {
        uint64_t cnt, fail, pre, bsum, total, bytes;
    } idx;
    // The LDS wave pass.  out_cap: output image capacity; the compressed input of a member whose output fits
    // is at most gzip_bound(out) unless it is not a deflate member at all (lds_max_in).
    // dict_out, the image: the dictionary, rounded to 16 bytes, in front of the plain members' out_cap bytes.
    // A dictionary member starts at the image's first byte and needs dict_len + min(capacity, ISIZE) of it:
    // that fits while its capacity is within max_len, which a device-resident caller need not keep -- max_len
    // bounds the decompressed sizes, a slab passes its own.  The members this pass cannot hold go to a second
    // launch sized for the longest dictionary member, dict_len + ISIZE = 16382; like the HBM variant it is
    // always launched, the lengths being device-resident, unless this pass has that size already or a
    // host-memory caller, who knows lengths and capacities, says that no member needs it.
    uint64_t out_cap, lds_max_in;
    uint32_t dict_out;
    struct Second { // the second pass's InflateArgs fields of these names
        uint64_t lds_max_out, lds_max_in;
        uint32_t dict_out, first_img, first_in;
    } second;
};

// the LDS wave pass's output image for a call with this max_len, and the staged input that goes with an image
inline uint64_t inflate_out_cap(uint64_t max_len, uint64_t out_limit) {
    return (std::min<uint64_t>(out_limit, std::max<uint64_t>(max_len, 1)) + 63) & ~(uint64_t)63;
}
inline uint64_t inflate_lds_in(uint64_t out_cap) { return gzip_bound(out_cap) + 64; }

// A host-memory caller, who knows the lengths (max_in: the longest member), launches the wave kernels' HBM
// variant (and the second dictionary pass) only when some member may exceed the LDS pass's image or input;
// off the latency route they are always launched.
inline bool inflate_need_hbm(bool latency, uint64_t max_len, uint64_t max_in, uint64_t out_limit) {
    const uint64_t out_cap = inflate_out_cap(max_len, out_limit);
    return !latency || max_len > out_cap || max_in > inflate_lds_in(out_cap);
}

inline InflatePlan plan_inflate(const InflateIn &in) {
    InflatePlan P{};
    const uint64_t n = in.n, max_len = in.max_len, cus = in.cus;
    auto grid = [](uint64_t need, uint64_t cap) { return (uint32_t)std::min<uint64_t>(need, cap); };
    // the smallest power of two G <= 64 with ceil(n / G) <= slots (64 if there is none)
    auto group = [n](uint64_t slots) {
        uint32_t G = 1;
        while (G < 64 && (n + G - 1) / G > slots) G *= 2;
        return G;
    };
    P.lane_route = !in.wave_only && !in.latency;
    P.chunk_pass = !in.wave_only && max_len > kIdxChunk;
    P.chunk_all = P.chunk_pass && in.latency;
    P.order = P.lane_route && !in.no_order && n >= 4096;
    P.rec = P.lane_route && !in.no_rec;
    P.multi_pass = max_len > 16383;
    P.verify = P.lane_route || P.chunk_pass;
    P.hbm = in.need_hbm;
    P.retry_only = P.lane_route || P.chunk_pass;
    P.count_retried = P.lane_route;

    P.ob = grid((n + 1023) / 1024, cus * 4);
    P.lb = grid((n + 63) / 64, cus * 16);
    P.out1k = max_len <= 1024;
    P.rstride = (uint32_t)std::min<uint64_t>(in.rec_max, std::max<uint64_t>(64, (max_len + 63) & ~(uint64_t)63));
    const uint64_t slots = cus * (P.out1k ? in.rec_per_cu_1k : in.rec_per_cu_4k);
    P.G = group(slots);
    P.rb = grid((n + P.G - 1) / P.G, slots);
    P.rec_max_out = (uint32_t)(P.out1k ? 1024 : in.rec_out_max);
    P.VG = group(cus * 32);
    P.vb = grid((n + 8ull * P.VG - 1) / (8ull * P.VG), cus * 4);
    P.mb = grid((n + 255) / 256, cus * 8);
    P.cb = grid((n * kIdxMaxChunks + 63) / 64, cus * in.chunk_per_cu);
    P.hbm_waves = std::min<uint64_t>(cus * 4, n);
    P.hbm_blocks = (uint32_t)((P.hbm_waves + 3) / 4);

    P.crcx_bytes = n * 4;
    P.order_bytes = (uint64_t)kOrderBins * 4 + n * 4;
    P.recs_bytes = (uint64_t)P.rb * 64 * P.rstride * 4 + 256;
    P.bigl_bytes = n * 4 + 256;
    const uint64_t nb = (n + in.scan_block - 1) / in.scan_block;
    P.idx.cnt = 0;
    P.idx.fail = 4 * n;
    P.idx.pre = (8 * n + 7) & ~(uint64_t)7;
    P.idx.bsum = P.idx.pre + 8 * n;
    P.idx.total = P.idx.bsum + 8 * nb;
    P.idx.bytes = P.idx.total + 8;

    const uint32_t dD = in.dict_len;
    P.out_cap = inflate_out_cap(max_len, in.out_limit);
    P.lds_max_in = inflate_lds_in(P.out_cap);
    P.dict_out = (uint32_t)(P.out_cap + ((dD + 15u) & ~15u));
    const uint64_t dict_in = dD ? inflate_lds_in(kDictSpan - dD) : 0;
    P.dict_second = dD && in.need_hbm && (P.dict_out < kDictSpan || P.lds_max_in < dict_in);
    P.second.lds_max_out = (kDictSpan + 63) & ~63u;
    P.second.dict_out = (uint32_t)P.second.lds_max_out;
    P.second.lds_max_in = dict_in;
    P.second.first_img = P.dict_out;
    P.second.first_in = (uint32_t)P.lds_max_in;
    return P;
}

// ---- staging layouts ---------------------------------------------------------------------------------------
// A call's staging is one pinned host buffer and one device buffer of the same layout: arrays of m elements,
// each starting on a multiple of 256 bytes, then the call's bytes from `meta` on.  The host side is filled and
// copied over in one piece.  An array knows its offset, its host pointer (from the host base) and its device
// pointer (from the device base).
inline uint64_t al256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
template <class T>
struct StageArr {
    uint64_t off;
    T *h, *d;
};
// two arrays that one copy fetches: `bytes` from the first one's start
struct StageSpan {
    void *h, *d;
    uint64_t bytes;
};
// Hands out the arrays in declaration order.  (Without bases -- to learn `meta` before the buffers are
// sized -- the pointers are the offsets.)
struct StageCarver {
    uint64_t m, meta = 0;
    uintptr_t hp, dp;
    explicit StageCarver(uint64_t m, void *host = nullptr, void *dev = nullptr)
        : m(m), hp((uintptr_t)host), dp((uintptr_t)dev) {}
    // a run of `count` elements between the arrays: raw bytes, or an array of another length than m
    template <class T = uint8_t>
    StageArr<T> run(uint64_t count) {
        const StageArr<T> a{meta, (T *)(hp + meta), (T *)(dp + meta)};
        meta += al256(count * sizeof(T));
        return a;
    }
    template <class T>
    StageArr<T> take() {
        return run<T>(m);
    }
    StageArr<uint64_t> u64() { return take<uint64_t>(); }
    StageArr<uint32_t> u32() { return take<uint32_t>(); }
    StageArr<int32_t> i32() { return take<int32_t>(); }
    // a's and b's bytes as one span: b lies directly behind a
    template <class A, class B>
    StageSpan span(const StageArr<A> &a, const StageArr<B> &b) const {
        assert(a.off + al256(m * sizeof(A)) == b.off);
        return StageSpan{a.h, a.d, al256(m * sizeof(A)) + al256(m * sizeof(B))};
    }
};
// A layout of arrays alone, one per call site (members are initialised in declaration order: that order is
// the layout).  pmc_store_plan.hpp states the store's with it.
#define PMC_STAGE(Name)                                                                            \
    explicit Name(uint64_t m, void *host = nullptr, void *dev = nullptr) : c(m, host, dev) {} \
    StageCarver c

// ---- a host-memory call (pmc_host.hip: pmc_gzip_*_batch_host, pmc_gzip_compress / _decompress) --------------
// Its staging, in the order of the two copies: [offsets, lengths, caps | source bytes] go down in one H2D of
// `down` bytes, [output lengths, verdicts | output bytes] come back in one D2H of `up` bytes from dlen on.
struct HostStage {
    HostStage(uint64_t n, uint64_t in_bytes, uint64_t out_bytes, void *host = nullptr, void *dev = nullptr)
        : c(n, host, dev), in_bytes(in_bytes), out_bytes(out_bytes) {}
    StageCarver c;
    uint64_t in_bytes, out_bytes;
    StageArr<uint64_t> soff = c.u64(), doff = c.u64();
    StageArr<uint32_t> slen = c.u32(), dcap = c.u32();
    StageArr<uint8_t> src = c.run(in_bytes + 16);
    uint64_t down = c.meta;
    StageArr<uint32_t> dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    StageArr<uint8_t> dst = c.run(out_bytes + 16);
    uint64_t up = c.meta - down;
    uint64_t bytes() const { return down + up; }

    // the host arrays of n values packed back to back: source i at the sum of the lengths before it, slot i
    // at the sum of the capacities before it
    void fill(const uint32_t *src_len, const uint32_t *dst_cap) const {
        uint64_t so = 0, dof = 0;
        for (uint64_t i = 0; i < c.m; i++) {
            soff.h[i] = so;
            slen.h[i] = src_len[i];
            so += src_len[i];
            doff.h[i] = dof;
            dcap.h[i] = dst_cap[i];
            dof += dst_cap[i];
        }
    }
};

struct HostBatchIn {
    bool compress;
    uint32_t n;
    const uint32_t *src_len, *dst_cap;
    uint64_t cus;
    bool level_fast, lane_order_ok; // level_is_fast of the context's level; its lane-order probe passed
    // latency_batch(), latency_max_len() and the LDS wave kernel's output image (kInflateLdsOut)
    uint64_t lat_batch, lat_max_len, out_limit;
    bool force_pipeline;            // the throughput route whatever the batch's size
};
struct HostBatchPlan {
    uint64_t in_bytes, out_bytes; // the sums of src_len and of dst_cap
    uint64_t max_len, max_in;     // the largest source length (decompress: capacity); the largest source length
    bool latency;                 // the one-kernel route, in coherent host memory and without copies
    bool need_hbm;                // decompress: inflate_need_hbm (compress: unused, false)
    int path;                     // the pmc_ctx_path_counts counter of this call
};
// Routing (limits measured with scripts/few_sweep.py).  Compress: up to 1,024 values of <= 4 KiB the
// one-kernel path (deflate_small_kernel) beats the pipeline; above 4 KiB the wave-per-value kernel would
// work from HBM, far slower than the split pipeline's large pass; a fast level always takes the pipeline
// (the one-kernel path is exact only).  Decompress: the wave-per-member inflate kernel holds a member's
// output in LDS up to out_limit (48 KiB), so a member up to that size stays on the latency path (a 30 KB
// member: 0.81 ms there against 3.8 ms through the pipeline); its batch limit is 4,096
// members / 16 MiB of output (inflate_latency: round 5 measured the wave kernel still 2x ahead there).
inline HostBatchPlan plan_host_batch(const HostBatchIn &in) {
    HostBatchPlan P{};
    for (uint32_t i = 0; i < in.n; i++) {
        P.in_bytes += in.src_len[i];
        P.out_bytes += in.dst_cap[i];
        P.max_len = std::max<uint64_t>(P.max_len, in.compress ? in.src_len[i] : in.dst_cap[i]);
        P.max_in = std::max<uint64_t>(P.max_in, in.src_len[i]);
    }
    const bool fast = in.compress && in.level_fast && in.lane_order_ok;
    P.latency = !in.force_pipeline &&
                (in.compress ? !fast && in.n <= in.lat_batch && P.max_len <= in.lat_max_len
                             : inflate_latency(in.n, P.max_len, P.out_bytes, in.cus, in.lat_batch, in.lat_max_len, false,
                                               in.out_limit));
    // the wave kernels' HBM variant only for members the LDS image cannot hold
    P.need_hbm = !in.compress && inflate_need_hbm(P.latency, P.max_len, P.max_in, in.out_limit);
    P.path = (P.latency ? 0 : 2) + (in.compress ? 0 : 1);
    return P;
}

// ---- a pinned call's chunks (pmc_host.hip: pmc_gzip_*_batch_pinned) -----------------------------------------
constexpr uint32_t kIdxScanBlock = 1024; // (= kScanBlock: scan_u32's block sums, one per so many members)

// values per chunk (the caller's, or by default a sixteenth of the batch and at least 65,536) and chunks
struct PinnedChunks {
    uint32_t chunk, nchunks;
};
inline PinnedChunks pinned_chunk_of(uint32_t n, uint32_t chunk) {
    if (chunk == 0) chunk = std::max<uint32_t>(65536, (uint32_t)(((uint64_t)n + 15) / 16));
    return PinnedChunks{chunk, (uint32_t)((n + (uint64_t)chunk - 1) / chunk)};
}

// What the chunk of values [a, a + m) covers (m >= 1).  Source: the range [sb, se) = [min src_off, max src_off +
// src_len) of its values.  Destination [db, de): tiled slots (dst_off given, dst_off[i + 1] == dst_off[i] +
// dst_cap[i] throughout the chunk) are that range of dst, copied back whole; any other slot layout, and packed
// mode (dst_off null), is compacted: the device lays the slots out back to back from 0 by a scan of dst_cap.
struct PinnedChunk {
    uint64_t sb, se, db, de;
    bool compact;
    uint32_t nb; // scan_u32's blocks over the chunk
};
inline PinnedChunk plan_pinned_chunk(const uint64_t *src_off, const uint32_t *src_len, const uint64_t *dst_off,
                                     const uint32_t *dst_cap, uint32_t a, uint32_t m) {
    PinnedChunk k{~0ull, 0, 0, 0, dst_off == nullptr, (m + kIdxScanBlock - 1) / kIdxScanBlock};
    const uint64_t end = (uint64_t)a + m;
    for (uint64_t i = a; i < end; i++) {
        k.sb = std::min(k.sb, src_off[i]);
        k.se = std::max(k.se, src_off[i] + src_len[i]);
    }
    for (uint64_t i = a; i + 1 < end && !k.compact; i++) k.compact = dst_off[i + 1] != dst_off[i] + dst_cap[i];
    if (k.compact) {
        for (uint64_t i = a; i < end; i++) k.de += dst_cap[i];
    } else {
        k.db = dst_off[a];
        k.de = dst_off[end - 1] + dst_cap[end - 1];
    }
    return k;
}

// A chunk's device slot: its arrays, scan_u32's block sums (the chunk's byte total behind them), its source
// range, its slots and -- a compacted chunk only -- its outputs back to back, as large as the slots.
struct PinnedSlot {
    PinnedSlot(uint64_t m, const PinnedChunk &k, void *dev = nullptr) : c(m, nullptr, dev), k(k) {}
    StageCarver c;
    PinnedChunk k;
    StageArr<uint64_t> soff = c.u64(), doff = c.u64(), poff = c.u64();
    StageArr<uint32_t> slen = c.u32(), dcap = c.u32(), dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    StageArr<uint64_t> bsum = c.run<uint64_t>(k.nb + 1ull);
    uint64_t meta = c.meta;
    StageArr<uint8_t> src = c.run(k.se - k.sb + 16), dst = c.run(k.de - k.db + 16);
    StageArr<uint8_t> packed = c.run(k.compact ? k.de - k.db + 16 : 0);
    uint64_t need = c.meta;
};

// ---- dictionary training (pmc_dict_train.hip; include/pmc_codec.h "dictionary training") ---------------------
constexpr uint32_t kTrainKmer = 8, kTrainSeg = 64, kTrainBits = 20; // d, K, F
constexpr uint32_t kTrainWin = kTrainSeg - kTrainKmer + 1;          // W = 57 positions per segment
constexpr uint64_t kTrainMult = 0x9E3779B185EBCA87ull;
constexpr uint32_t kTrainSlotBytes = 16;   // a block's best: u64 score, u32 sample, u32 start
constexpr uint32_t kTrainWavesPerCu = 16;  // one-wave blocks of the count and score kernels per CU
constexpr uint64_t kTrainHostBytes = 256ull << 20; // pmc_dict_train_host: the most sample bytes of a call

inline bool dict_train_args_ok(uint64_t n, uint64_t dict_size) {
    return n >= 1 && n <= PMC_DICT_TRAIN_MAX_SAMPLES && dict_size >= kTrainSeg && dict_size <= PMC_DICT_MAX &&
           dict_size % kTrainSeg == 0;
}

// A training call over n samples for a dictionary of dict_size bytes (dict_train_args_ok).  E epochs; epoch e owns
// the samples [lo(e), hi(e)), one wave per sample up to the resident waves, and every block of its score launch
// writes one slot, so max_blocks slots serve every epoch.  Scratch: the table (2^F u32), the count of selected
// segments (u32, in a 256-byte row of its own), the slots, E rows of 64 bytes.  At most 4 MiB + 256 + 16 *
// kTrainWavesPerCu * cus + 8 KiB bytes, whatever the samples are.
struct DictTrainPlan {
    uint32_t E;
    uint32_t n;
    uint32_t count_blocks, max_blocks;
    uint64_t table, nsel, slots, rows, bytes; // offsets into the scratch; its size
    uint32_t lo(uint32_t e) const { return (uint32_t)((uint64_t)e * n / E); }
    uint32_t hi(uint32_t e) const { return (uint32_t)(((uint64_t)e + 1) * n / E); }
    uint32_t blocks(uint32_t e) const { return std::min<uint32_t>(hi(e) - lo(e), max_blocks); } // 0: nothing to launch
};
inline DictTrainPlan plan_dict_train(uint32_t n, uint32_t dict_size, uint64_t cus) {
    DictTrainPlan P{};
    P.E = dict_size / kTrainSeg;
    P.n = n;
    const uint64_t resident = std::max<uint64_t>(1, cus) * kTrainWavesPerCu;
    P.count_blocks = (uint32_t)std::min<uint64_t>(n, resident);
    P.max_blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + P.E - 1) / P.E, resident);
    P.table = 0;
    P.nsel = P.table + (4ull << kTrainBits);
    P.slots = P.nsel + 256;
    P.rows = (P.slots + (uint64_t)kTrainSlotBytes * P.max_blocks + 255) & ~(uint64_t)255;
    P.bytes = P.rows + (uint64_t)P.E * kTrainSeg;
    return P;
}

} // namespace pmc

// pmc_capi.hip -- host side of the C-ABI declared in include/pmc_codec.h.
//
// Owns per-device state (stream, symbol slabs, HBM working sets, pinned staging) and
// turns a batch into at most two launches per direction: the LDS-resident kernel for
// values whose working set fits a wave's LDS share, and the HBM-resident variant for
// the rest (large values; same device code, working set in a per-wave HBM slab).
#include <hip/hip_runtime.h>

#include <vector>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/pmc_codec.h"
#include "pmc_device.hpp"
#include "pmc_kernels.hpp"

#define PMC_API extern "C" __attribute__((visibility("default")))

namespace pmc {

__constant__ Tables c_tables = make_tables();
__constant__ uint32_t c_crc_table[256];
__constant__ uint32_t c_crc_shift16[kCrcShiftEntries];
__constant__ uint32_t c_crc_shift64k[kCrcShiftEntries];
__constant__ uint32_t c_crc_slice8[8 * 256];
__constant__ uint32_t c_crc_zpiece[4 * 4 * 256];
__constant__ uint32_t c_crc_ones[kCrcQuarterMax + 1];

static thread_local std::string g_err;
static void set_err(const char *what, hipError_t e) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, e == hipSuccess ? "" : hipGetErrorString(e));
    g_err = buf;
}
#define HIP_TRY(x)                    \
    do {                              \
        hipError_t e_ = (x);          \
        if (e_ != hipSuccess) {       \
            set_err(#x, e_);          \
            return PMC_E_NO_DEVICE;   \
        }                             \
    } while (0)

// ---- CRC-32 constants (zlib crc32.c / 1.2.12 crc32_combine_gen) -------------------------
static uint32_t h_multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
static uint32_t h_x2nmodp(uint64_t n, unsigned k) { // x^(n * 2^k) mod P
    uint32_t x2n[64];
    uint32_t p = 1u << 30; // x^1
    x2n[0] = p;
    for (int i = 1; i < 64; i++) x2n[i] = p = h_multmodp(p, p);
    p = 1u << 31; // x^0
    while (n) {
        if (n & 1) p = h_multmodp(x2n[k & 63], p);
        n >>= 1;
        k++;
    }
    return p;
}

static int upload_constants() {
    uint32_t tab[256];
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t c = n;
        for (int k = 0; k < 8; k++) c = c & 1 ? kCrcPoly ^ (c >> 1) : c >> 1;
        tab[n] = c;
    }
    static uint32_t s16[kCrcShiftEntries], s64k[kCrcShiftEntries];
    // x^(8*16*d) = x^(d * 2^7);  x^(8*65536*d) = x^(d * 2^19)
    for (int d = 0; d < kCrcShiftEntries; d++) {
        s16[d] = h_x2nmodp((uint64_t)d, 7);
        s64k[d] = h_x2nmodp((uint64_t)d, 19);
    }
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_crc_table), tab, sizeof tab));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_crc_shift16), s16, sizeof s16));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_crc_shift64k), s64k, sizeof s64k));
    static uint32_t s8[8 * 256], zp[4 * 4 * 256], ones[kCrcQuarterMax + 1];
    for (int b = 0; b < 256; b++) {
        s8[b] = tab[b];
        for (int k = 1; k < 8; k++) s8[k * 256 + b] = (s8[(k - 1) * 256 + b] >> 8) ^ tab[s8[(k - 1) * 256 + b] & 0xff];
    }
    for (int k = 0; k < 4; k++) {
        const uint32_t m = h_x2nmodp(1, 9 + k); // x^(8 * 64 * 2^k)
        for (int j = 0; j < 4; j++)
            for (int b = 0; b < 256; b++) zp[(k * 4 + j) * 256 + b] = h_multmodp(m, (uint32_t)b << (8 * j));
    }
    for (uint32_t len = 0; len <= kCrcQuarterMax; len++) ones[len] = h_multmodp(h_x2nmodp(len, 3), 0xFFFFFFFFu);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_crc_slice8), s8, sizeof s8));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_crc_zpiece), zp, sizeof zp));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_crc_ones), ones, sizeof ones));
    return PMC_OK;
}

constexpr uint64_t kLdsPerCu = 160 * 1024;
constexpr uint64_t kCrcTabBytes = 1024;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return PMC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max(n, (size_t)4096);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            set_err("hipMalloc", e);
            return PMC_Z_MEM_ERROR;
        }
        cap = want;
        return PMC_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};
struct HostBuf {
    void *p = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;
    int ensure(size_t n) {
        if (n <= cap) return PMC_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max(n, (size_t)4096);
        hipError_t e = hipHostMalloc(&p, want, flags);
        if (e != hipSuccess) {
            set_err("hipHostMalloc", e);
            return PMC_Z_MEM_ERROR;
        }
        cap = want;
        return PMC_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

} // namespace pmc

using namespace pmc;

struct pmc_ctx {
    int device = 0;
    int cus = 0;
    hipStream_t stream = nullptr;
    DevBuf tokens, dscratch;     // deflate symbol slabs / HBM working sets
    DevBuf fbscratch;            // per-wave Trees for the small kernel's serial fallback
    DevBuf split;                // chunk arrays of the split small-value pipeline
    DevBuf crcx;                 // inflate: CRC-32 trailers from the lane kernel
    DevBuf order;                // inflate: lane visit order (bins | member indices)
    DevBuf recs;                 // inflate: the record kernel's per-lane record rows
    DevBuf bigl;                 // inflate: count + list of the members the record kernel leaves to the lane kernel
    // lane-order guards (DeflateArgs::guard): u32 [0] sort, [1] code ranks, [2] the create-time probe's
    // violations, [3] values sent to the HBM kernel's retry pass by the other paths, [4] members the
    // decompress fast paths handed to the wave kernels; lane_order_ok = the probe passed (else compress takes the kernels that do not need it)
    DevBuf guard;
    DevBuf rlist;                // compress: the per-call retry list (DeflateArgs::rlist)
    bool lane_order_ok = true;
    // compression level of the calls issued from now on (pmc_ctx_set_level): PMC_LEVEL_EXACT, PMC_LEVEL_FAST
    // or PMC_LEVEL_FAST_ALL
    std::atomic<int> level{PMC_LEVEL_EXACT};
    // the index switch of the calls issued from now on (pmc_ctx_set_index; include/pmc_codec.h "member index")
    std::atomic<int> index{0};
    // the chunk-CRC switch of the compress calls (pmc_ctx_set_index_crc) and the verification mode of the ranged
    // reads (pmc_ctx_set_range_verify: 0 check where present, 1 require) issued from now on
    std::atomic<int> index_crc{0}, range_verify{0};
    DevBuf idx;                  // inflate: the chunk pass's rows (counts | fail | prefix | block sums)
    // inflate: resident blocks per CU of inflate_chunk_kernel and of the record kernel's 4 KiB [0] and 1 KiB [1]
    // instances (0: not asked yet; asked under the decompress lock)
    int chunk_per_cu = 0, rec_per_cu[2] = {0, 0};
    // ranged reads (pmc_inflate_range.hip): the request rows and the edge rows (pmc_plan.hpp RangePlan); resident
    // blocks per CU of inflate_range_kernel (0: not asked yet; asked under the decompress lock)
    DevBuf rng;
    int range_per_cu = 0;
    // ranged writes (pmc_deflate_patch.hip): the request rows and a round's chunk rows (pmc_plan.hpp PatchPlan,
    // PatchRound); resident blocks per CU of patch_decode_kernel (0: not asked yet; asked under the compress lock)
    DevBuf pat, patr;
    int patch_per_cu = 0;
    // preset dictionary (pmc_ctx_set_dictionary): its bytes on the device (zero padded to a multiple of 16),
    // length and id (CRC-32; 0 = none).  Written with host_mu and both dir_mu held, read under a dir_mu.
    DevBuf dict;
    uint32_t dict_len = 0, dict_id = 0;
    // dictionary training (pmc_dict_train.hip): the table, block slots and rows (pmc_plan.hpp DictTrainPlan); a
    // compress-direction scratch
    DevBuf train;
    // host-call routing (pmc_ctx_path_counts): [0] / [1] compress / decompress calls on the latency
    // path, [2] / [3] on the throughput pipeline
    uint64_t path_calls[4] = {0, 0, 0, 0};
    uint64_t latency_redone = 0; // latency-path compress calls whose declined values a pipeline call redid
    // large values (pmc_deflate_large.hip): selection list, round tables, round scratch, emit scratch
    DevBuf lvsel, lvtab, lvbuf, lvemit;
    HostBuf lvpin;
    // per direction (0 compress, 1 decompress): the event recorded after the last batch call and its
    // stream; a call on another stream waits for it, since both use the direction's scratch
    hipEvent_t dir_ev[2] = {};
    hipStream_t dir_st[2] = {};
    bool dir_used[2] = {false, false};
    bool prof = false;           // pmc_ctx_profile: bracket every launch with events
    struct KRec {
        int kind;
        hipEvent_t a, b;
    };
    std::vector<KRec> krecs;
    std::mutex host_mu;          // host-API calls (host_batch, pinned_batch) of this context, one at a time
    // per direction: the scratch buffers above (DevBuf::ensure may free and reallocate them) and
    // dir_ev / dir_st / dir_used are touched by one enqueueing thread at a time, whichever API
    // (device batch, host batch, pinned, store, slab) it came through; a compress and a decompress
    // still enqueue concurrently.  Recursive: the slab and store calls hold it around their own
    // dir_enter / dir_leave and call the batch entry points inside.
    std::recursive_mutex dir_mu[2];
    DevBuf staging;              // device side of host-API calls
    uint64_t *dbg = nullptr;     // diagnostic stamp sums (PMC_STAMPS builds)
    HostBuf pinned;              // host side of host-API calls
    HostBuf zc;                  // latency path: coherent host memory the kernel reads and writes in place
    void *zc_dev = nullptr;      // its device address
    // pmc_gzip_*_batch_pinned: chunk c's H2D (stream h2d), kernels (stream) and D2H (stream d2h)
    // overlap those of chunks c +- 1; slot c & 1 of `pipe` holds chunk c's arrays and bytes.
    struct Pipe {
        hipStream_t h2d = nullptr, d2h = nullptr;
        hipEvent_t in[2] = {}, out[2] = {}, done[2] = {};
        DevBuf slot[2];
        HostBuf total;           // compacted chunks: each slot's chunk total, read by the host
        HostBuf bounce[2];       // slot mode, compacted chunk: outputs on their way to dst_off
        bool busy[2] = {false, false};
    } pipe;
};

namespace {

// Runs `launch` (which enqueues one kernel on st); with profiling on, brackets it with events.
template <class F>
void klaunch(pmc_ctx *ctx, int kind, hipStream_t st, F launch) {
    if (!ctx->prof) {
        launch();
        return;
    }
    pmc_ctx::KRec r{kind, nullptr, nullptr};
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
        launch();
        return;
    }
    (void)hipEventRecord(r.a, st);
    launch();
    (void)hipEventRecord(r.b, st);
    ctx->krecs.push_back(r);
}

// Same-direction batch calls of one context share its scratch: a call issued on a different stream
// than the previous one of its direction first waits (on the device) for that call to finish.
int dir_enter(pmc_ctx *ctx, int dir, hipStream_t st) {
    if (ctx->dir_used[dir] && ctx->dir_st[dir] != st)
        if (hipStreamWaitEvent(st, ctx->dir_ev[dir], 0) != hipSuccess) return PMC_E_NO_DEVICE;
    return PMC_OK;
}
int dir_leave(pmc_ctx *ctx, int dir, hipStream_t st) {
    if (hipEventRecord(ctx->dir_ev[dir], st) != hipSuccess) return PMC_E_NO_DEVICE;
    ctx->dir_st[dir] = st;
    ctx->dir_used[dir] = true;
    return PMC_OK;
}

struct Launch {
    int wpb;        // waves per block
    int blocks;     // grid size
    uint64_t wave_bytes;
    size_t lds;     // dynamic LDS per block
};

// (fallback: the answer when the runtime gives none)
int occupancy_blocks(const void *kernel, int threads, size_t lds, int fallback = 1) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, lds) != hipSuccess || nb < 1) nb = fallback;
    return nb;
}

// values with len <= this go through the LDS deflate kernel (one wave needs the whole
// working set: value, sorted keys, ranks, output image, Huffman trees)
uint64_t deflate_lds_limit() {
    uint64_t lo = 64, hi = 65535;
    while (lo < hi) {
        uint64_t mid = (lo + hi + 1) / 2;
        if (deflate_wave_bytes(false, mid) + kCrcTabBytes <= kLdsPerCu) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// values up to this length take the single-block small kernel (pmc_deflate_small.hip)
uint64_t deflate_small_limit() {
    uint64_t lo = 64, hi = 16382;
    while (lo < hi) {
        uint64_t mid = (lo + hi + 1) / 2;
        if (deflate_small_wave_bytes(mid) + kCrcTabBytes <= kLdsPerCu) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// `extra` = dynamic LDS per block besides the waves' working sets (the CRC table; 0 for the front).
// values up to this length take the split pipeline's large pass: the front's working set (no chain
// counts) and the back's must fit a CU's LDS, and every match distance must stay <= MAX_DIST
// (32506; longer values would need zlib's window limit in the candidate walk)
uint64_t deflate_big_limit() {
    uint64_t lo = kSmallMax, hi = 32506;
    while (lo < hi) {
        uint64_t mid = (lo + hi + 1) / 2;
        if (deflate_front_wave_bytes(mid) <= kLdsPerCu && deflate_back_wave_bytes(mid) + kBackTabBytes <= kLdsPerCu)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

Launch plan_lds(pmc_ctx *ctx, const void *kernel, uint64_t wave_bytes, uint64_t n_items,
                uint64_t extra = kCrcTabBytes) {
    Launch L;
    L.wave_bytes = wave_bytes;
    uint64_t fit = (kLdsPerCu - extra) / wave_bytes;
    // waves per block: the most resident waves per CU, then the widest block.  At 4 KiB values the
    // front needs 25 KB per wave: 4-wave blocks (102 KB) fit once per CU (4 waves), 2-wave blocks
    // three times (6 waves).
    L.wpb = (int)std::max<uint64_t>(1, std::min<uint64_t>(4, fit));
    int per_cu = occupancy_blocks(kernel, 64 * L.wpb, extra + L.wpb * wave_bytes);
    for (int w = L.wpb - 1; w >= 1; w--) {
        const int pc = occupancy_blocks(kernel, 64 * w, extra + w * wave_bytes);
        if (w * pc > L.wpb * per_cu) {
            L.wpb = w;
            per_cu = pc;
        }
    }
    L.lds = extra + L.wpb * wave_bytes;
    uint64_t need_blocks = (n_items + L.wpb - 1) / L.wpb;
    L.blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->cus * per_cu, need_blocks));
    return L;
}

} // namespace

// ================================================================== API
PMC_API const char *pmc_last_error(void) { return g_err.c_str(); }
PMC_API const char *pmc_version(void) { return "pmc_codec 0.1 gfx950 (zlib-1.2.11 level-9 gzip, bit-exact)"; }
PMC_API size_t pmc_gzip_bound(size_t len) { return (size_t)gzip_bound(len); }

// PMC_LEVEL: the initial level of every context created from now on (unset: exact).  -1: not a level.
static int env_level() {
    const char *e = getenv("PMC_LEVEL");
    if (!e) return PMC_LEVEL_EXACT;
    if (!strcmp(e, "fast") || !strcmp(e, "1")) return PMC_LEVEL_FAST;
    if (!strcmp(e, "fast-all") || !strcmp(e, "2")) return PMC_LEVEL_FAST_ALL;
    if (!strcmp(e, "exact") || !strcmp(e, "9")) return PMC_LEVEL_EXACT;
    return -1;
}

// PMC_INDEX: the initial index switch of every context created from now on (unset: off).  -1: neither 0 nor 1.
static int env_index() {
    const char *e = getenv("PMC_INDEX");
    if (!e) return 0;
    return !strcmp(e, "1") ? 1 : !strcmp(e, "0") ? 0 : -1;
}

// PMC_INDEX_CRC: the same for the chunk-CRC switch.
static int env_index_crc() {
    const char *e = getenv("PMC_INDEX_CRC");
    if (!e) return 0;
    return !strcmp(e, "1") ? 1 : !strcmp(e, "0") ? 0 : -1;
}

static int env_dictionary(std::vector<uint8_t> &bytes);
static uint32_t host_crc32(const uint8_t *p, size_t n);
static int set_dictionary_locked(pmc_ctx *ctx, const void *dict, size_t len, uint32_t id);

PMC_API int pmc_ctx_create(int device, pmc_ctx **out) {
    *out = nullptr;
    const int lvl = env_level();
    if (lvl < 0) {
        g_err = std::string("PMC_LEVEL=") + getenv("PMC_LEVEL") + ": expected fast, 1, fast-all, 2, exact or 9";
        return PMC_E_ARG;
    }
    const int idx = env_index();
    if (idx < 0) {
        g_err = std::string("PMC_INDEX=") + getenv("PMC_INDEX") + ": expected 1 or 0";
        return PMC_E_ARG;
    }
    const int idx_crc = env_index_crc();
    if (idx_crc < 0) {
        g_err = std::string("PMC_INDEX_CRC=") + getenv("PMC_INDEX_CRC") + ": expected 1 or 0";
        return PMC_E_ARG;
    }
    std::vector<uint8_t> env_dict; // PMC_DICT: checked before any device is touched, as PMC_LEVEL
    if (env_dictionary(env_dict) < 0) return PMC_E_ARG;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= device) {
        set_err("hipGetDeviceCount", e);
        return PMC_E_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_err = std::string("device is ") + prop.gcnArchName + ", library built for gfx950";
        return PMC_E_NO_DEVICE;
    }
    int rc = upload_constants();
    if (rc) return rc;
    // the LDS-resident kernels may use the whole 160 KiB of a CU
    HIP_TRY(hipFuncSetAttribute((const void *)deflate_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)deflate_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kLdsPerCu));
    for (const void *fk : {(const void *)deflate_front_kernel<0>, (const void *)deflate_front_kernel<1024>,
                           (const void *)deflate_front_kernel<4096>})
        HIP_TRY(hipFuncSetAttribute(fk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    for (const void *fk : {(const void *)deflate_front_fast_kernel<0>, (const void *)deflate_front_fast_kernel<1024>,
                           (const void *)deflate_front_fast_kernel<4096>})
        HIP_TRY(hipFuncSetAttribute(fk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)deflate_front_fast_dict_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)lv_fast_parse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)deflate_back_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)deflate_trees_kernel<kTreesCap1K>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)deflate_trees_kernel<kTreesCap>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)deflate_trees_kernel<kLCodes>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)inflate_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)inflate_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)inflate_dict_kernel<false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    HIP_TRY(hipFuncSetAttribute((const void *)inflate_dict_kernel<true>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
    pmc_ctx *c = new pmc_ctx;
    c->device = device;
    c->cus = prop.multiProcessorCount;
    c->index = idx;
    c->index_crc = idx_crc;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->dir_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->dir_ev[1], hipEventDisableTiming) != hipSuccess) {
        delete c;
        return PMC_E_NO_DEVICE;
    }
    // guard counters, and the lane-order self-test (lane_order_probe_kernel: 4 waves x 512 trials)
    uint32_t probe = 0;
    // (bytes 32..47: the chunk pass's two u64 counters, pmc_ctx_index_counts; bytes 64..87: the ranged reads'
    // three, pmc_ctx_range_counts; bytes 96..111: their two verification counters, pmc_ctx_range_verify_counts;
    // bytes 112..115: RangeArgs::ncrc of the ranged call in flight; bytes 128..167: the ranged writes' five u64
    // counters, pmc_ctx_rewrite_counts)
    if (c->guard.ensure(192) || hipMemsetAsync(c->guard.p, 0, 192, c->stream) != hipSuccess) {
        pmc_ctx_destroy(c);
        return PMC_E_NO_DEVICE;
    }
    hipLaunchKernelGGL(lane_order_probe_kernel, dim3(1), dim3(256), 0, c->stream, 512u, (uint32_t *)c->guard.p + 2);
    if (hipMemcpyAsync(&probe, (uint32_t *)c->guard.p + 2, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        set_err("lane_order_probe_kernel", hipGetLastError());
        pmc_ctx_destroy(c);
        return PMC_E_NO_DEVICE;
    }
    c->lane_order_ok = probe == 0;
    if (level_is_fast(lvl)) {
        // (the fast fronts share the sort whose lane order the probe just checked: a context that failed it
        // stays exact, as pmc_ctx_set_level would answer)
        if (c->lane_order_ok) c->level = lvl;
        else g_err = "PMC_LEVEL=fast / fast-all ignored: the lane-order probe failed, the context stays at level 9";
    }
    if (!env_dict.empty()) {
        rc = set_dictionary_locked(c, env_dict.data(), env_dict.size(), host_crc32(env_dict.data(), env_dict.size()));
        if (rc) {
            pmc_ctx_destroy(c);
            return rc;
        }
    }
    *out = c;
    return PMC_OK;
}

PMC_API int pmc_ctx_set_level(pmc_ctx *ctx, int level) {
    if (!ctx || (level != PMC_LEVEL_EXACT && !level_is_fast(level))) return PMC_E_ARG;
    if (level_is_fast(level) && !ctx->lane_order_ok) return PMC_E_ARG;
    ctx->level = level;
    return PMC_OK;
}

PMC_API int pmc_ctx_get_level(pmc_ctx *ctx, int *level) {
    if (!ctx || !level) return PMC_E_ARG;
    *level = ctx->level;
    return PMC_OK;
}

// ---- member index (include/pmc_codec.h "member index") ---------------------------------------------------
PMC_API int pmc_ctx_set_index(pmc_ctx *ctx, int on) {
    if (!ctx || (on != 0 && on != 1)) return PMC_E_ARG;
    ctx->index = on;
    return PMC_OK;
}

PMC_API int pmc_ctx_get_index(pmc_ctx *ctx, int *on) {
    if (!ctx || !on) return PMC_E_ARG;
    *on = ctx->index;
    return PMC_OK;
}

PMC_API int pmc_gzip_index_info(const void *member, size_t len, uint32_t *chunk_bytes, uint32_t *nchunks) {
    uint32_t lg = 0, K = 0, isz = 0, hdr = 0;
    if (!member || !idx_parse((const uint8_t *)member, len, &lg, &K, &isz, &hdr)) return PMC_E_ARG;
    if (chunk_bytes) *chunk_bytes = 1u << lg;
    if (nchunks) *nchunks = K;
    return PMC_OK;
}

// chunk CRCs (include/pmc_codec.h "member index", chunk CRCs)
PMC_API int pmc_ctx_set_index_crc(pmc_ctx *ctx, int on) {
    if (!ctx || (on != 0 && on != 1)) return PMC_E_ARG;
    ctx->index_crc = on;
    return PMC_OK;
}

PMC_API int pmc_ctx_get_index_crc(pmc_ctx *ctx, int *on) {
    if (!ctx || !on) return PMC_E_ARG;
    *on = ctx->index_crc;
    return PMC_OK;
}

PMC_API int pmc_gzip_index_crc_info(const void *member, size_t len, uint32_t *crcs, uint32_t cap, uint32_t *nchunks) {
    uint32_t K = 0, at = 0;
    if (!member || !idx_crc_parse((const uint8_t *)member, len, &K, &at)) return PMC_E_ARG;
    if (nchunks) *nchunks = K;
    if (cap < K) return PMC_E_CAPACITY;
    const uint8_t *e = (const uint8_t *)member + at;
    for (uint32_t k = 0; crcs && k < K; k++, e += 4)
        crcs[k] = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
    return PMC_OK;
}

PMC_API int pmc_ctx_index_counts(pmc_ctx *ctx, uint64_t counts[2]) {
    if (!ctx || !counts) return PMC_E_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, (uint8_t *)ctx->guard.p + 32, 16, hipMemcpyDeviceToHost));
    return PMC_OK;
}

// ---- preset dictionary (include/pmc_codec.h "preset dictionary") ---------------------------------------
static uint32_t host_crc32(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = c & 1 ? kCrcPoly ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

// PMC_DICT: the initial dictionary of every context created from now on.  0: unset, 1: `bytes` holds a
// valid dictionary, -1: the file is unreadable, empty, oversized or has CRC-32 0 (g_err says which).
static int env_dictionary(std::vector<uint8_t> &bytes) {
    const char *path = getenv("PMC_DICT");
    if (!path) return 0;
    FILE *f = fopen(path, "rb");
    if (!f) {
        g_err = std::string("PMC_DICT=") + path + ": cannot be read";
        return -1;
    }
    bytes.resize(PMC_DICT_MAX + 1);
    const size_t n = fread(bytes.data(), 1, bytes.size(), f);
    fclose(f);
    bytes.resize(n);
    if (n == 0 || n > PMC_DICT_MAX) {
        g_err = std::string("PMC_DICT=") + path + (n ? ": more than PMC_DICT_MAX (8192) bytes" : ": empty");
        return -1;
    }
    if (host_crc32(bytes.data(), n) == 0) {
        g_err = std::string("PMC_DICT=") + path + ": CRC-32 is 0, which stands for no dictionary";
        return -1;
    }
    return 1;
}

// A dictionary is set in two steps, so that a failure leaves the context with the dictionary it had:
// dict_upload copies the bytes to a fresh buffer on the context's device and touches nothing of the context;
// dict_wait waits for the context's enqueued work; dict_swap, which cannot fail, makes the buffer the context's.
// (dict_wait and dict_swap: the caller holds host_mu and both dir_mu, or owns a context nobody else has seen.)
static int dict_upload(pmc_ctx *ctx, const void *dict, size_t len, DevBuf &nb) {
    if (!len) return PMC_OK;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    int r = PMC_OK;
    const size_t padded = (len + 15) & ~(size_t)15;
    std::vector<uint8_t> h(padded + 16, 0);
    memcpy(h.data(), dict, len);
    if (hipSetDevice(ctx->device) != hipSuccess) {
        set_err("pmc_ctx_set_dictionary", hipGetLastError());
        r = PMC_E_NO_DEVICE;
    } else if (!(r = nb.ensure(h.size())) && hipMemcpy(nb.p, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_err("pmc_ctx_set_dictionary", hipGetLastError());
        r = PMC_E_NO_DEVICE;
    }
    if (r) {
        if (prev >= 0) (void)hipSetDevice(ctx->device);
        nb.release();
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    return r;
}
static int dict_wait(pmc_ctx *ctx) {
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    int r = PMC_OK;
    if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        set_err("pmc_ctx_set_dictionary", hipGetLastError());
        r = PMC_E_NO_DEVICE;
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    return r;
}
static void dict_swap(pmc_ctx *ctx, DevBuf &nb, size_t len, uint32_t id) { // (len 0 clears)
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(ctx->device);
    ctx->dict.release();
    ctx->dict = nb;
    nb = DevBuf();
    ctx->dict_len = (uint32_t)len;
    ctx->dict_id = len ? id : 0u;
    if (prev >= 0) (void)hipSetDevice(prev);
}
static int set_dictionary_locked(pmc_ctx *ctx, const void *dict, size_t len, uint32_t id) {
    DevBuf nb;
    int r = dict_upload(ctx, dict, len, nb);
    if (!r && (r = dict_wait(ctx))) {
        int prev = -1;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(ctx->device);
        nb.release();
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    if (!r) dict_swap(ctx, nb, len, id);
    return r;
}

PMC_API int pmc_ctx_set_dictionary(pmc_ctx *ctx, const void *dict, size_t len) {
    if (!ctx || len > PMC_DICT_MAX) return PMC_E_ARG;
    if (!dict) len = 0;
    uint32_t id = 0;
    if (len && (id = host_crc32((const uint8_t *)dict, len)) == 0) return PMC_E_ARG;
    std::lock_guard<std::mutex> host_lock(ctx->host_mu);
    std::lock_guard<std::recursive_mutex> c_lock(ctx->dir_mu[0]), d_lock(ctx->dir_mu[1]);
    return set_dictionary_locked(ctx, dict, len, id);
}

PMC_API int pmc_ctx_get_dictionary_id(pmc_ctx *ctx, uint32_t *id) {
    if (!ctx || !id) return PMC_E_ARG;
    std::lock_guard<std::recursive_mutex> c_lock(ctx->dir_mu[0]);
    *id = ctx->dict_id;
    return PMC_OK;
}

PMC_API int pmc_ctx_guard_counts(pmc_ctx *ctx, uint32_t counts[5]) {
    if (!ctx || !counts) return PMC_E_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, ctx->guard.p, 20, hipMemcpyDeviceToHost));
    return PMC_OK;
}

PMC_API int pmc_ctx_path_counts(pmc_ctx *ctx, uint64_t counts[4]) {
    if (!ctx || !counts) return PMC_E_ARG;
    std::lock_guard<std::mutex> lock(ctx->host_mu);
    for (int k = 0; k < 4; k++) counts[k] = ctx->path_calls[k];
    return PMC_OK;
}

PMC_API int pmc_ctx_latency_redone(pmc_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return PMC_E_ARG;
    std::lock_guard<std::mutex> lock(ctx->host_mu);
    *n = ctx->latency_redone;
    return PMC_OK;
}

PMC_API void pmc_ctx_destroy(pmc_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->tokens.release();
    c->dscratch.release();
    c->fbscratch.release();
    c->split.release();
    c->crcx.release();
    c->recs.release();
    c->bigl.release();
    c->idx.release();
    c->rng.release();
    c->pat.release();
    c->patr.release();
    c->dict.release();
    c->train.release();
    c->guard.release();
    c->rlist.release();
    c->lvsel.release();
    c->lvtab.release();
    c->lvbuf.release();
    c->lvemit.release();
    c->lvpin.release();
    for (auto &r : c->krecs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    c->krecs.clear();
    c->staging.release();
    c->pinned.release();
    c->zc.release();
    if (c->pipe.h2d) {
        (void)hipStreamSynchronize(c->pipe.d2h);
        for (int k = 0; k < 2; k++) {
            (void)hipEventDestroy(c->pipe.in[k]);
            (void)hipEventDestroy(c->pipe.out[k]);
            (void)hipEventDestroy(c->pipe.done[k]);
            c->pipe.slot[k].release();
        }
        c->pipe.total.release();
        c->pipe.bounce[0].release();
        c->pipe.bounce[1].release();
        (void)hipStreamDestroy(c->pipe.h2d);
        (void)hipStreamDestroy(c->pipe.d2h);
    }
    for (int k = 0; k < 2; k++)
        if (c->dir_ev[k]) (void)hipEventDestroy(c->dir_ev[k]);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

PMC_API pmc_ctx *pmc_default_ctx(void) {
    static std::once_flag once;
    static pmc_ctx *ctx = nullptr;
    std::call_once(once, [] {
        if (pmc_ctx_create(0, &ctx) != PMC_OK) ctx = nullptr;
    });
    return ctx;
}

PMC_API uint32_t pmc_gzip_isize(const void *in, size_t in_len) {
    if (!in || in_len < 18) return 0;
    const uint8_t *p = (const uint8_t *)in + in_len - 4;
    return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Batches of at most this many values, from the host-memory calls (the drop-in's single values, a
// server's small batches), take the latency path: one wave-per-value kernel that does the whole
// value (deflate_small_kernel; inflate_kernel for decompress) instead of the throughput pipeline's
// chain of launches (front, order sort, trees, back; record / lane kernels, CRC verify), which only
// pays once a batch fills the CUs.
constexpr uint32_t kLatencyBatch = 1024;
constexpr uint64_t kLatencyMaxLen = 4096;
// (PMC_LATENCY_MAX_LEN / PMC_LATENCY_BATCH override them; 0 disables the path)
static uint64_t latency_max_len() {
    static const uint64_t v = getenv("PMC_LATENCY_MAX_LEN") ? (uint64_t)atoll(getenv("PMC_LATENCY_MAX_LEN")) : kLatencyMaxLen;
    return v;
}
static uint64_t latency_batch() {
    static const uint64_t v = getenv("PMC_LATENCY_BATCH") ? (uint64_t)atoll(getenv("PMC_LATENCY_BATCH")) : kLatencyBatch;
    return v;
}
// the largest output image of the wave-per-member inflate kernel's LDS variant: the decompress side's length
// limit on the latency path (inflate_latency, pmc_plan.hpp, states the route)
constexpr uint64_t kInflateLdsOut = 48 * 1024;

// ---- kernel instances ----------------------------------------------------------------------------------
// Each is chosen once, as a typed pointer: the same pointer feeds the occupancy plan and the launch.
using DeflateKernel = void (*)(DeflateArgs);
using InflateKernel = void (*)(InflateArgs);
// the split pipeline's front of a pass (fcap: front_cap_class(pcap); the dictionary front has one instance)
static DeflateKernel front_kernel(bool dictp, bool fastp, uint32_t fcap) {
    if (dictp) return deflate_front_fast_dict_kernel;
    if (fastp)
        return fcap == 1024 ? deflate_front_fast_kernel<1024>
               : fcap == 4096 ? deflate_front_fast_kernel<4096> : deflate_front_fast_kernel<0>;
    return fcap == 1024 ? deflate_front_kernel<1024> : fcap == 4096 ? deflate_front_kernel<4096> : deflate_front_kernel<0>;
}
// the one-kernel paths: the general LDS kernel (PMC_DEFLATE_V1) or the small kernel
static DeflateKernel mono_kernel(bool v1) { return v1 ? deflate_kernel<false> : deflate_small_kernel; }
// the record kernel's 1 KiB image instance, or the 4 KiB one
static InflateKernel rec_kernel(bool out1k) { return out1k ? inflate_rec_kernel<1024> : inflate_rec_kernel<kRecOutMax>; }
// the wave-per-member kernels (LDS / HBM working set), of a context with or without a dictionary
static InflateKernel wave_kernel(bool hbm, bool dict) {
    if (hbm) return dict ? inflate_dict_kernel<true> : inflate_kernel<true>;
    return dict ? inflate_dict_kernel<false> : inflate_kernel<false>;
}

// ---- large values (pmc_deflate_large.hip, pmc_deflate_fast_large.hip) ------------------------------------
// The batch's values of lo < len <= hi.  Their lengths live on the device: one small readback (a count,
// then the (index, length) list) lets the host plan rounds of values whose tables and scratch fit a
// budget (LvRound, pmc_plan.hpp).  This is the only synchronous step of a device-resident compress
// call, taken only when max_len says such values may be present.
// Exact level: each round sorts the values' positions, parses segments speculatively and stitches them.
// fast (PMC_LEVEL_FAST_ALL): no sort, rank, map or stitch scratch -- one wave per segment parses it in LDS.
// Either way the large-value emit kernel then writes the members (header byte 8 = 2 / 4).
// The loop body depends on the round only through its plan.
// A round's tables and scratch fit 24 GiB (PMC_LV_ROUND_MB lowers or raises that, for tests: a budget of a few
// values' cost cuts a small batch into several rounds; a value above the budget is a round of its own).
static uint64_t lv_round_budget() {
    static const uint64_t budget = [] {
        const char *e = getenv("PMC_LV_ROUND_MB");
        const long long mb = e ? atoll(e) : 0;
        return mb > 0 && mb < (1ll << 24) ? (uint64_t)mb << 20 : 24ull << 30; // (unset, not a number, <= 0: the default)
    }();
    return budget;
}
static int large_values(pmc_ctx *ctx, const DeflateArgs &a, uint64_t lo, uint64_t hi, bool fast, hipStream_t st) {
    const uint64_t n = a.n;
    int r = ctx->lvsel.ensure(8 + 8 * n);
    if (r) return r;
    uint32_t *sel = (uint32_t *)ctx->lvsel.p;
    HIP_TRY(hipMemsetAsync(sel, 0, 8, st));
    hipLaunchKernelGGL(lv_select_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                       a.src_len, n, lo, hi, sel);
    uint32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, sel, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!cnt) return PMC_OK;
    std::vector<uint32_t> list(2 * (size_t)cnt);
    HIP_TRY(hipMemcpy(list.data(), sel + 2, 8 * (size_t)cnt, hipMemcpyDeviceToHost));
    std::vector<std::pair<uint32_t, uint32_t>> vals(cnt);
    for (uint32_t k = 0; k < cnt; k++) vals[k] = {list[2 * k], list[2 * k + 1]};
    std::sort(vals.begin(), vals.end());
    const uint64_t budget = lv_round_budget();
    // (the index switch acts on the segmented fast members only; read once per call)
    const uint32_t idx_chunk = fast && ctx->index ? kIdxChunk : 0u;
    const uint32_t idx_crc = idx_chunk && ctx->index_crc ? 1u : 0u;
    const uint64_t fwb = fast ? lv_fast_wave_bytes() : 0;
    const Launch Lp = fast ? plan_lds(ctx, (const void *)lv_fast_parse_kernel, fwb, 1ull << 40, 0) : Launch{};
    for (size_t v0 = 0; v0 < vals.size();) {
        const LvRound R = lv_plan_round(vals.data(), vals.size(), v0, fast ? kFlSeg : 0u, budget);
        HIP_TRY(hipStreamSynchronize(st)); // (the previous round's kernels read the pinned tables' device copy)
        r = ctx->lvpin.ensure(R.tab_bytes);
        if (!r) r = ctx->lvtab.ensure(R.tab_bytes);
        if (r) return r;
        R.fill((uint8_t *)ctx->lvpin.p);
        uint8_t *dt = (uint8_t *)ctx->lvtab.p;
        HIP_TRY(hipMemcpyAsync(dt, ctx->lvpin.p, R.tab_bytes, hipMemcpyHostToDevice, st));
        r = ctx->lvbuf.ensure(R.scratch_bytes);
        if (r) return r;
        uint8_t *d = (uint8_t *)ctx->lvbuf.p;
        LargeArgs L{};
        L.src = a.src;
        L.src_off = a.src_off;
        L.src_len = a.src_len;
        L.lv_val = (const uint32_t *)(dt + R.o_val);
        L.lv_pbase = (const uint64_t *)(dt + R.o_pbase);
        L.lv_seg0 = (const uint32_t *)(dt + R.o_seg0);
        L.lv_ch0 = (const uint32_t *)(dt + R.o_ch0);
        L.seg_val = (const uint32_t *)(dt + R.o_seg_val);
        L.seg_tok0 = (const uint64_t *)(dt + R.o_seg_tok0);
        L.ch_val = (const uint32_t *)(dt + R.o_ch_val);
        L.nv = R.nv;
        L.nseg = (uint32_t)R.nseg;
        L.nch = (uint32_t)R.nch;
        L.tmp = (uint32_t *)(d + R.b_tmp);
        L.S = (uint32_t *)(d + R.b_S);
        L.R = (uint32_t *)(d + R.b_R);
        L.HC = d + R.b_HC;
        L.hist = (uint32_t *)(d + R.b_hist);
        L.tok = (uint32_t *)(d + R.b_tok);
        L.map = (uint32_t *)(d + R.b_map);
        L.seg_tok = (uint32_t *)(d + R.b_seg_tok);
        L.fail = (int32_t *)(d + R.b_fail);
        // gzip XFL: the reference's header for an exact member; zlib's "fastest algorithm" for a fast one, as
        // the small fast members
        L.xfl = fast ? 4 : 2;
        L.idx_chunk = idx_chunk;
        L.idx_crc = idx_crc;
        if (fast) {
            HIP_TRY(hipMemsetAsync(L.fail, 0, 4ull * R.nv, st));
            DeflateArgs p = a;
            p.cap_len = kFlCap;
            p.wave_bytes = fwb;
            klaunch(ctx, PMC_K_DEFLATE_LARGE, st, [&] {
                const dim3 pg((unsigned)std::min<uint64_t>(Lp.blocks, (R.nseg + Lp.wpb - 1) / Lp.wpb));
                hipLaunchKernelGGL(lv_fast_parse_kernel, pg, dim3(64 * Lp.wpb), Lp.lds, st, p, L);
            });
        } else {
            const unsigned cb = (unsigned)std::min<uint64_t>((R.nch + 3) / 4, (uint64_t)ctx->cus * 8);
            const unsigned sb = (unsigned)std::min<uint64_t>((R.nseg + 3) / 4, (uint64_t)ctx->cus * 8);
            const unsigned vb = (unsigned)std::min<uint64_t>(R.nv, (uint64_t)ctx->cus * 4);
            klaunch(ctx, PMC_K_DEFLATE_LARGE, st, [&] {
                for (int pass = 0; pass < 2; pass++) {
                    hipLaunchKernelGGL(lv_sort_hist_kernel, dim3(cb), dim3(256), 0, st, L, pass);
                    hipLaunchKernelGGL(lv_sort_scan_kernel, dim3(vb), dim3(256), 0, st, L);
                    hipLaunchKernelGGL(lv_sort_scatter_kernel, dim3(cb), dim3(256), 0, st, L, pass);
                }
                hipLaunchKernelGGL(lv_rank_kernel, dim3(cb), dim3(256), 0, st, L);
                hipLaunchKernelGGL(lv_parse_kernel, dim3(sb), dim3(256), 0, st, L);
                hipLaunchKernelGGL(lv_stitch_kernel, dim3(vb), dim3(64), 0, st, L);
            });
        }
        // emit: one wave per value
        DeflateArgs e = a;
        e.cap_len = R.maxlen;
        e.wave_bytes = deflate_lv_emit_wave_bytes(R.maxlen);
        const uint64_t ew = std::max<uint64_t>(4, std::min<uint64_t>(
            {(uint64_t)(R.nv + 3) / 4 * 4, (uint64_t)ctx->cus * 4, std::max<uint64_t>(4, (8ull << 30) / e.wave_bytes / 4 * 4)}));
        r = ctx->lvemit.ensure(ew * e.wave_bytes);
        if (r) return r;
        e.scratch = (uint8_t *)ctx->lvemit.p;
        klaunch(ctx, PMC_K_DEFLATE_LARGE_EMIT, st, [&] {
            hipLaunchKernelGGL(deflate_lv_emit_kernel, dim3((unsigned)(ew / 4)), dim3(256), deflate_lv_emit_lds(4), st, e,
                               L);
        });
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) {
            set_err(fast ? "fast large-value kernels" : "large-value kernels", err);
            return PMC_E_NO_DEVICE;
        }
        v0 = R.v1;
    }
    return PMC_OK;
}

// chunk scratch budget (PMC_SPLIT_CHUNK_MB): 96 GiB of the 288 GiB holds 14M 1-KiB values, so the
// 10M north-star batch is one front/trees/back launch set (~7 KB of chunk arrays per 1 KiB value,
// allocated only as large as the batch needs).  Fewer, larger chunks mean fewer kernel tails:
// 2 / 6 / 9 / 16 / 48 / 96 GiB measured -50 %, -2 %, -1 %, 0, +0.9 %, +1.2 % round trip (same box)
static uint64_t split_chunk_budget() {
    static const uint64_t budget = (getenv("PMC_SPLIT_CHUNK_MB") ? (uint64_t)atoll(getenv("PMC_SPLIT_CHUNK_MB"))
                                                                 : 98304ull) << 20;
    return budget;
}

// One pass of the split pipeline over the batch (SplitPass, pmc_plan.hpp), chunk by chunk: front, visit
// order, trees, back.  dD: the context's dictionary length, for a dictionary pass.  ctx->split holds
// SplitLayout(pcap, chunk).bytes().
static int run_split_pass(pmc_ctx *ctx, DeflateArgs &a, const SplitPass &ps, uint32_t dD, hipStream_t st) {
    const uint64_t n = a.n, pcap = ps.pcap;
    const bool fastp = ps.fastp, dictp = ps.dictp;
    static const bool no_order = getenv("PMC_TREES_ORDER") && !atoi(getenv("PMC_TREES_ORDER"));
    // (the front keeps no CRC table in LDS: its grid is sized for the blocks that really fit)
    const size_t tl_small = (size_t)(kTreesCap + 1) * 64 * 4, tl_1k = (size_t)(kTreesCap1K + 1) * 64 * 4;
    const size_t tl_big = (size_t)(kLCodes + 1) * 64 * 4;
    const uint32_t fcap = dictp ? 0u : front_cap_class(pcap);
    const uint64_t dcap = std::min<uint64_t>(((uint64_t)dD + ps.hi + 63) & ~(uint64_t)63, kDictSpan);
    const uint64_t fwb = dictp   ? deflate_front_fast_wave_bytes(dcap)
                         : fastp ? deflate_front_fast_wave_bytes(fcap ? fcap : pcap)
                                 : deflate_front_wave_bytes(fcap ? fcap : pcap);
    const uint64_t bwb = deflate_back_wave_bytes(pcap);
    a.dict = dictp ? (const uint8_t *)ctx->dict.p : nullptr;
    a.dict_len = dictp ? dD : 0u;
    a.front_cap = dictp ? (uint32_t)dcap : 0u;
    a.mtime = dictp ? ctx->dict_id : 0u; // gzip MTIME: the dictionary's id marks a dictionary member
    a.xfl = fastp ? 4u : 2u; // gzip XFL: zlib's "fastest algorithm" for a fast member
    const DeflateKernel fk = front_kernel(dictp, fastp, fcap);
    const Launch Lf = plan_lds(ctx, (const void *)fk, fwb, n, 0);
    const Launch Lb = plan_lds(ctx, (const void *)deflate_back_kernel, bwb, n, kBackTabBytes);
    const uint64_t chunk = split_chunk_of(n, split_chunk_budget(), pcap);
    const SplitLayout SL(pcap, chunk);
    uint8_t *p = (uint8_t *)ctx->split.p;
    a.cT = (uint32_t *)(p + SL.cT);
    a.cN = (uint32_t *)(p + SL.cN);
    a.cP = (uint32_t *)(p + SL.cP);
    a.cG = (uint32_t *)(p + SL.cG);
    a.cH = (uint16_t *)(p + SL.cH);
    a.cL = p + SL.cL;
    a.cB = (uint32_t *)(p + SL.cB);
    a.cC = (uint32_t *)(p + SL.cC);
    a.cD = (uint32_t *)(p + SL.cD);
    a.cZ = (uint32_t *)(p + SL.cZ);
    uint32_t *ord = (uint32_t *)(p + SL.ord), *obins = (uint32_t *)(p + SL.obins);
    a.cQ = (uint32_t *)(p + SL.cQ);
    a.min_len = ps.lo;
    a.lds_max_len = ps.hi;
    a.cap_len = pcap;
    // front work grabs: several values per grab for small values, whose parse is shorter than
    // the counter's serialised grabs (10M x 256 B: 1 per grab 114 ms, 4 or 8: 51 ms; 1 KiB: 2 per
    // grab -0.3 %, 4 the same)
    a.front_batch = pcap <= 512 ? 4u : pcap <= 2048 ? 2u : 1u;
    for (uint64_t first = 0; first < n; first += chunk) {
        a.first = first;
        a.count = std::min<uint64_t>(chunk, n - first);
        const unsigned tb = (unsigned)((a.count + 63) / 64);
        a.wave_bytes = fwb;
        if (hipMemsetAsync(a.cQ, 0, 8, st) != hipSuccess) return PMC_E_NO_DEVICE;
        klaunch(ctx, PMC_K_DEFLATE_FRONT, st, [&] { // (a fast front is timed as the front it stands in for)
            const dim3 fg((unsigned)std::min<uint64_t>(Lf.blocks, (a.count + Lf.wpb - 1) / Lf.wpb));
            hipLaunchKernelGGL(fk, fg, dim3(64 * Lf.wpb), Lf.lds, st, a);
        });
        if (hipMemsetAsync(a.cD + a.count, 0, 4, st) != hipSuccess) return PMC_E_NO_DEVICE;
        // trees visit order by used literal/length symbols (PMC_TREES_ORDER=0: index order)
        a.cO = nullptr;
        if (!no_order && a.count >= 4096) {
            if (hipMemsetAsync(obins, 0, kOrderBins * 4, st) != hipSuccess) return PMC_E_NO_DEVICE;
            const unsigned ob = (unsigned)std::min<uint64_t>((a.count + 1023) / 1024, (uint64_t)ctx->cus * 4);
            klaunch(ctx, PMC_K_ORDER, st, [&] {
                hipLaunchKernelGGL(order_hist_kernel, dim3(ob), dim3(256), 0, st, (const uint32_t *)a.cZ, a.count, obins);
                hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(1024), 0, st, obins);
                hipLaunchKernelGGL(order_scatter_kernel, dim3(ob), dim3(256), 0, st, (const uint32_t *)a.cZ, a.count,
                                   obins, ord);
            });
            a.cO = ord;
        }
        klaunch(ctx, PMC_K_DEFLATE_TREES, st, [&] {
            if (pcap <= 1024) hipLaunchKernelGGL(deflate_trees_kernel<kTreesCap1K>, dim3(tb), dim3(64), tl_1k, st, a);
            else hipLaunchKernelGGL(deflate_trees_kernel<kTreesCap>, dim3(tb), dim3(64), tl_small, st, a);
            // (the overflow list's walker: its 73.5 KB heap column fits two one-wave blocks per CU)
            hipLaunchKernelGGL(deflate_trees_kernel<kLCodes>, dim3(std::min<unsigned>(tb, 2u * (unsigned)ctx->cus)),
                               dim3(64), tl_big, st, a);
        });
        a.wave_bytes = bwb;
        a.back_nostage = pcap <= kNostageMaxLen ? 1u : 0u;
        // the values' CRC-32 for the back (counted with the back: it is the back's work moved out)
        if (a.back_nostage) klaunch(ctx, PMC_K_DEFLATE_BACK, st, [&] {
            const unsigned cb = (unsigned)std::min<uint64_t>((a.count + 511) / 512, (uint64_t)ctx->cus * 4);
            hipLaunchKernelGGL(crc32_batch_kernel, dim3(cb), dim3(512), 0, st, (const uint8_t *)a.src,
                               (const uint64_t *)(a.src_off + a.first), (const uint32_t *)(a.src_len + a.first),
                               a.count, a.cC);
        });
        klaunch(ctx, PMC_K_DEFLATE_BACK, st, [&] {
            hipLaunchKernelGGL(deflate_back_kernel,
                               dim3((unsigned)std::min<uint64_t>(Lb.blocks, (a.count + Lb.wpb - 1) / Lb.wpb)),
                               dim3(64 * Lb.wpb), Lb.lds, st, a);
        });
    }
    return PMC_OK;
}

// A compress call: route (plan_route, pmc_plan.hpp: which path claims which lengths, and why) -> the split
// pipeline's passes or the one-kernel path -> large values -> the HBM kernel (V1: by length; else the gated
// retry pass).
static int compress_batch_body(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                               uint32_t n, uint8_t *dst, const uint64_t *dst_off, const uint32_t *dst_cap,
                               uint32_t *dst_len, int32_t *rc, uint32_t max_len, void *stream,
                               bool latency = false, bool small = false) {
    if (!ctx) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    if (max_len == 0) max_len = 1;
    hipStream_t st = (hipStream_t)stream;
    // src_len[i] > max_len: no variant below claims the value; it gets PMC_E_ARG on the device (the
    // latency path's caller computed max_len from the lengths itself)
    if (!latency)
        hipLaunchKernelGGL(arg_check_kernel, dim3((unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 2048)),
                           dim3(256), 0, st, src_len, (uint64_t)n, (uint64_t)max_len, rc, dst_len);
    DeflateArgs a{src, src_off, src_len, dst, dst_off, dst_cap, dst_len, rc, n, 0, 0, 0, nullptr, nullptr,
                  ctx->dbg, -1};
    a.guard = (uint32_t *)ctx->guard.p;
#if defined(PMC_STAMPS) || defined(PMC_PHASE_STOP)
    if (const char *e = getenv("PMC_STOP_AFTER")) a.stop_after = atoi(e); // diagnostic builds only
#endif
    static const bool force_v1 = getenv("PMC_DEFLATE_V1") && atoi(getenv("PMC_DEFLATE_V1"));
    static const bool mono_env = getenv("PMC_DEFLATE_MONO") && atoi(getenv("PMC_DEFLATE_MONO"));
    static const int big_env = getenv("PMC_BIG_PASS") ? atoi(getenv("PMC_BIG_PASS")) : -1;
    static const uint64_t small_lim = deflate_small_limit(), big_lim = deflate_big_limit(), v1_lim = deflate_lds_limit();
    const uint64_t hbm_wb = deflate_wave_bytes(true, max_len);
    RouteIn in{};
    in.n = n;
    in.max_len = max_len;
    in.level = ctx->level;
    in.lane_order_ok = ctx->lane_order_ok;
    in.dict_len = ctx->dict_id ? ctx->dict_len : 0u;
    in.cus = (uint64_t)ctx->cus;
    in.latency = latency;
    in.small = small;
    in.force_v1 = force_v1;
    in.mono_env = mono_env;
    in.big_env = big_env;
    in.small_lim = small_lim;
    in.big_lim = big_lim;
    in.v1_lim = v1_lim;
    in.single_block_max = kSmallMax;
    in.hbm_wb = hbm_wb;
    const Route R = plan_route(in);
    const uint64_t hbm_waves = R.hbm_waves;
    if (R.rlist) {
        int r = ctx->rlist.ensure(4ull * ((uint64_t)n + 1));
        if (r) return r;
        HIP_TRY(hipMemsetAsync(ctx->rlist.p, 0, 4, st));
        a.rlist = (uint32_t *)ctx->rlist.p;
    }
    if (R.kind == Route::kSplit) {
        uint64_t need = 0;
        for (int k = 0; k < R.npass; k++)
            need = std::max(need, SplitLayout(R.pass[k].pcap, split_chunk_of(n, split_chunk_budget(), R.pass[k].pcap)).bytes());
        int r = ctx->split.ensure(need);
        if (r) return r;
        if (hbm_waves) {
            r = ctx->tokens.ensure(hbm_waves * kSlabSyms * sizeof(uint32_t));
            if (r) return r;
            r = ctx->dscratch.ensure(hbm_waves * hbm_wb);
            if (r) return r;
        }
        for (int k = 0; k < R.npass; k++) {
            r = run_split_pass(ctx, a, R.pass[k], R.dict_len, st);
            if (r) return r;
        }
        a.min_len = 0;
        a.xfl = 2; // (everything after the small pass is exact)
        a.mtime = 0;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            set_err("deflate split pipeline", e);
            return PMC_E_NO_DEVICE;
        }
    } else {
        const bool v1 = R.kind == Route::kV1;
        const DeflateKernel lds_kernel = mono_kernel(v1);
        const uint64_t lds_wb = v1 ? deflate_wave_bytes(false, R.cap) : deflate_small_wave_bytes(R.cap);
        Launch Ls = plan_lds(ctx, (const void *)lds_kernel, lds_wb, n);
        const uint64_t small_waves = (uint64_t)Ls.blocks * Ls.wpb;
        // size every per-wave buffer before the first launch (no reallocation under a kernel)
        int r = ctx->tokens.ensure(std::max(small_waves, hbm_waves) * kSlabSyms * sizeof(uint32_t));
        if (r) return r;
        r = ctx->fbscratch.ensure(small_waves * sizeof(Trees));
        if (r) return r;
        if (hbm_waves) {
            r = ctx->dscratch.ensure(hbm_waves * hbm_wb);
            if (r) return r;
        }
        a.tokens = (uint32_t *)ctx->tokens.p;
        a.lds_max_len = R.lds_cut;
        a.cap_len = R.cap;
        a.wave_bytes = lds_wb;
        a.scratch = (uint8_t *)ctx->fbscratch.p;
        klaunch(ctx, PMC_K_DEFLATE_MONO, st,
                [&] { hipLaunchKernelGGL(lds_kernel, dim3(Ls.blocks), dim3(64 * Ls.wpb), Ls.lds, st, a); });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            set_err("deflate_kernel<lds>", e);
            return PMC_E_NO_DEVICE;
        }
    }
    a.tokens = (uint32_t *)ctx->tokens.p;
    // ---- large values (> hbm_cut): segment-parallel parse, stitched, emitted per value ----
    if (R.lv) {
        const int r = large_values(ctx, a, R.hbm_cut, max_len, R.fast_all, st);
        if (r) return r;
    }
    // ---- HBM kernel (V1: values > lds_cut; else gated retries) ----
    if (hbm_waves) {
        a.cap_len = max_len;
        a.lds_max_len = R.gated ? max_len : R.hbm_cut;
        a.retry = 1; // (large-pass values of several blocks, and values a lane-order guard declined)
        a.gate = R.gated ? 1 : 0;
        a.wave_bytes = hbm_wb;
        a.scratch = (uint8_t *)ctx->dscratch.p;
        klaunch(ctx, PMC_K_DEFLATE_HBM, st, [&] {
            hipLaunchKernelGGL(deflate_kernel<true>, dim3((unsigned)hbm_waves), dim3(64), kCrcTabBytes, st, a);
        });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            set_err("deflate_kernel<hbm>", e);
            return PMC_E_NO_DEVICE;
        }
    }
    return PMC_OK;
}

// ---- prefix sums (the chunk pass, the ranged calls, pmc_host.hip's compacted chunks) --------------------------
namespace {
// Exclusive prefix sum of v[i] (0 where rc[i] != 0, if rc is given) into out[]; kScanBlock values per
// block, block totals to bsum[] (scan_blocks_kernel turns them into block bases, bsum[nb] = total).
constexpr uint32_t kScanBlock = 1024;
static_assert(kScanBlock == kIdxScanBlock, "the plans size scan_u32's block sums");
__global__ __launch_bounds__(kScanBlock) void scan_local_kernel(const uint32_t *v, const int32_t *rc, uint32_t n,
                                                                 uint64_t *out, uint64_t *bsum) {
    __shared__ uint64_t s[kScanBlock];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kScanBlock + t;
    const uint64_t x = i < n && !(rc && rc[i] != 0) ? v[i] : 0;
    s[t] = x;
    __syncthreads();
    for (uint32_t d = 1; d < kScanBlock; d <<= 1) {
        uint64_t y = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    if (i < n) out[i] = s[t] - x;
    if (t == kScanBlock - 1) bsum[blockIdx.x] = s[t];
}

__global__ __launch_bounds__(kScanBlock) void scan_blocks_kernel(uint64_t *bsum, uint32_t nb) {
    __shared__ uint64_t s[kScanBlock];
    __shared__ uint64_t carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += kScanBlock) {
        const uint64_t x = base + t < nb ? bsum[base + t] : 0;
        s[t] = x;
        __syncthreads();
        for (uint32_t d = 1; d < kScanBlock; d <<= 1) {
            uint64_t y = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += y;
            __syncthreads();
        }
        if (base + t < nb) bsum[base + t] = carry + s[t] - x;
        __syncthreads();
        if (t == kScanBlock - 1) carry += s[t];
        __syncthreads();
    }
    if (t == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(kScanBlock) void scan_add_kernel(uint64_t *out, uint32_t n, const uint64_t *bsum) {
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    if (i < n) out[i] += bsum[blockIdx.x];
}

int scan_u32(const uint32_t *v, const int32_t *rc, uint32_t n, uint64_t *out, uint64_t *bsum, hipStream_t st) {
    const uint32_t nb = (n + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(scan_local_kernel, dim3(nb), dim3(kScanBlock), 0, st, v, rc, n, out, bsum);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanBlock), 0, st, bsum, nb);
    hipLaunchKernelGGL(scan_add_kernel, dim3(nb), dim3(kScanBlock), 0, st, out, n, bsum);
    HIP_TRY(hipGetLastError());
    return PMC_OK;
}
} // namespace

// ---- a decompress call: plan_inflate (pmc_plan.hpp: which stages run, their grids and scratch, and why) ->
// order, record kernel, lane passes, chunk pass, CRC check, wave kernels --------------------------------------
// the A/B switches of the decompress path, read once per process
struct InflateEnv {
    bool wave_only, no_order, no_rec; // PMC_INFLATE_WAVE=1, PMC_INFLATE_ORDER=0, PMC_INFLATE_REC=0
};
static const InflateEnv &inflate_env() {
    auto value = [](const char *name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; };
    static const InflateEnv e{value("PMC_INFLATE_WAVE", 0) != 0, value("PMC_INFLATE_ORDER", 1) == 0,
                              value("PMC_INFLATE_REC", 1) == 0};
    return e;
}

static InflateIn inflate_in(pmc_ctx *ctx, uint32_t n, uint32_t max_len, bool latency, bool need_hbm) {
    // (asked once per context, under its decompress lock: a context is one device)
    if (!ctx->chunk_per_cu) {
        for (int k = 0; k < 2; k++) {
            const uint32_t rlds = rec_lds_bytes(k ? 1024 : kRecOutMax);
            ctx->rec_per_cu[k] = occupancy_blocks((const void *)rec_kernel(k != 0), 64, rlds, (int)(kLdsPerCu / rlds));
        }
        ctx->chunk_per_cu = occupancy_blocks((const void *)inflate_chunk_kernel, 64, kChunkLdsBytes);
    }
    const InflateEnv &env = inflate_env();
    InflateIn in{};
    in.n = n;
    in.max_len = max_len;
    in.cus = (uint64_t)ctx->cus;
    in.latency = latency;
    in.need_hbm = need_hbm;
    in.dict_len = ctx->dict_id ? ctx->dict_len : 0u;
    in.wave_only = env.wave_only;
    in.no_order = env.no_order;
    in.no_rec = env.no_rec;
    in.rec_per_cu_4k = (uint64_t)ctx->rec_per_cu[0];
    in.rec_per_cu_1k = (uint64_t)ctx->rec_per_cu[1];
    in.chunk_per_cu = (uint64_t)ctx->chunk_per_cu;
    in.rec_max = kRecMax;
    in.rec_out_max = kRecOutMax;
    in.scan_block = kIdxScanBlock;
    in.out_limit = kInflateLdsOut;
    return in;
}

// Each stage gets the InflateArgs of the call, `a`, and launches with it or with a copy that carries the
// fields only its own launches see.  A field a stage sets on `a` itself stays for the launches after it.

// The visit order: member indices by compressed length into ctx->order (bins | indices).
static int stage_order(pmc_ctx *ctx, const InflatePlan &P, const uint32_t *src_len, uint64_t n, const uint32_t **ord,
                       hipStream_t st) {
    uint32_t *bins = (uint32_t *)ctx->order.p, *o = bins + kOrderBins;
    HIP_TRY(hipMemsetAsync(bins, 0, kOrderBins * 4, st));
    klaunch(ctx, PMC_K_ORDER, st, [&] {
        hipLaunchKernelGGL(order_hist_kernel, dim3(P.ob), dim3(256), 0, st, src_len, n, bins);
        hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(1024), 0, st, bins);
        hipLaunchKernelGGL(order_scatter_kernel, dim3(P.ob), dim3(256), 0, st, src_len, n, bins, o);
    });
    *ord = o;
    return PMC_OK;
}

// The record kernel; the record rows it sets on `a` stay.  It appends the members it leaves to the lane passes
// to the list in ctx->bigl (count | members).
static int stage_record(pmc_ctx *ctx, const InflatePlan &P, InflateArgs &a, const uint32_t *ord, hipStream_t st) {
    a.rec_group = P.G;
    a.rec_max_out = P.rec_max_out;
    a.rec_work = (uint32_t *)ctx->recs.p;
    a.rec_scratch = (uint32_t *)((uint8_t *)ctx->recs.p + 256);
    a.rec_stride = P.rstride;
#if defined(PMC_STAMPS) || defined(PMC_PHASE_STOP)
    if (const char *e = getenv("PMC_STOP_AFTER")) a.stop_after = atoi(e); // 31 prepare, 32 phase A
#endif
    HIP_TRY(hipMemsetAsync(a.rec_work, 0, 4, st));
    InflateArgs k = a;
    k.order = ord;
    k.big_count = (uint32_t *)ctx->bigl.p;
    k.big_list = (uint32_t *)((uint8_t *)ctx->bigl.p + 256);
    HIP_TRY(hipMemsetAsync(k.big_count, 0, 4, st));
    klaunch(ctx, PMC_K_INFLATE_REC, st, [&] {
        hipLaunchKernelGGL(rec_kernel(P.out1k), dim3(P.rb), dim3(64), rec_lds_bytes(P.rec_max_out), st, k);
    });
    return PMC_OK;
}

// The lane passes: over the record kernel's list when it ran, else over every member.  multi_pass stays on `a`.
static void stage_lanes(pmc_ctx *ctx, const InflatePlan &P, InflateArgs &a, const uint32_t *ord, hipStream_t st) {
    a.multi_pass = P.multi_pass ? 1 : 0;
    InflateArgs k = a;
    k.order = ord;
    if (P.rec) {
        k.big_only = 1;
        k.big_count = (uint32_t *)ctx->bigl.p;
        k.big_list = (uint32_t *)((uint8_t *)ctx->bigl.p + 256);
    }
    klaunch(ctx, PMC_K_INFLATE_LANE, st, [&] {
        hipLaunchKernelGGL((inflate_lane_kernel<kLaneLitCap, false>), dim3(P.lb), dim3(64), kLaneLdsBytes, st, k);
        // members whose lit/len code did not fit its lists (a third of 30 KB JSON values): the wide
        // instance (it skips every other member at once)
        hipLaunchKernelGGL((inflate_lane_kernel<kLaneWideLit, false>), dim3(P.lb), dim3(64), kLaneWideLdsBytes, st, k);
        if (P.multi_pass)
            hipLaunchKernelGGL((inflate_lane_kernel<kLaneWideLit, true>), dim3(P.lb), dim3(64), kLaneMultiLdsBytes, st, k);
    });
}

// ---- indexed members (pmc_inflate_chunk.hip; include/pmc_codec.h "member index") --------------------------
// The chunk pass up to the CRC check: which members carry a valid index (InflatePlan::chunk_all), a prefix sum
// of their chunk counts, one lane per chunk, then rc / dst_len / crc_expect of the members whose chunks all
// decoded.  Enqueue only, no readback; the rows in ctx->idx are O(n).  The caller runs inflate_verify_kernel,
// then chunk_pass_count.
static int chunk_pass_decode(pmc_ctx *ctx, const InflatePlan &P, const InflateArgs &a, ChunkArgs &X, hipStream_t st) {
    uint8_t *p = (uint8_t *)ctx->idx.p;
    uint64_t *pre = (uint64_t *)(p + P.idx.pre), *bsum = (uint64_t *)(p + P.idx.bsum);
    X.cnt = (uint32_t *)(p + P.idx.cnt);
    X.fail = (uint32_t *)(p + P.idx.fail);
    X.pre = pre;
    X.total = (uint64_t *)(p + P.idx.total);
    X.counts = (uint64_t *)((uint8_t *)ctx->guard.p + 32);
    X.all = P.chunk_all ? 1 : 0;
    int r = PMC_OK;
    klaunch(ctx, PMC_K_ORDER, st, [&] {
        hipLaunchKernelGGL(inflate_chunk_scan_kernel, dim3(P.mb), dim3(256), 0, st, a, X);
        r = scan_u32(X.cnt, nullptr, (uint32_t)a.n, pre, bsum, st);
    });
    if (r) return r; // (scan_u32 has named the launch that failed)
    klaunch(ctx, PMC_K_INFLATE_LANE, st, [&] {
        hipLaunchKernelGGL(inflate_chunk_kernel, dim3(P.cb), dim3(64), kChunkLdsBytes, st, a, X);
        hipLaunchKernelGGL(inflate_chunk_finish_kernel, dim3(P.mb), dim3(256), 0, st, a, X);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_err("inflate_chunk_kernel", e);
        return PMC_E_NO_DEVICE;
    }
    return PMC_OK;
}
static void chunk_pass_count(pmc_ctx *ctx, const InflatePlan &P, const InflateArgs &a, const ChunkArgs &X, hipStream_t st) {
    klaunch(ctx, PMC_K_INFLATE_LANE, st,
            [&] { hipLaunchKernelGGL(inflate_chunk_count_kernel, dim3(P.mb), dim3(256), 0, st, a, X); });
}

// Launches a wave-per-member kernel (blocks of wpb waves) and checks the launch under `name`.
static int launch_wave(pmc_ctx *ctx, int kind, InflateKernel k, unsigned blocks, int wpb, size_t lds, const InflateArgs &a,
                       const char *name, hipStream_t st) {
    klaunch(ctx, kind, st, [&] { hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * wpb), lds, st, a); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(name, e);
        return PMC_E_NO_DEVICE;
    }
    return PMC_OK;
}
// An LDS wave pass with the image and input sizes in `a`; its wave_bytes follow them.
static int wave_lds(pmc_ctx *ctx, InflateKernel k, InflateArgs &a, const char *name, hipStream_t st) {
    a.wave_bytes = inflate_wave_bytes(false, a.dict_out, a.lds_max_in);
    const Launch L = plan_lds(ctx, (const void *)k, a.wave_bytes, a.n);
    return launch_wave(ctx, PMC_K_INFLATE_LDS, k, (unsigned)L.blocks, L.wpb, L.lds, a, name, st);
}

static int decompress_batch_body(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                 const uint32_t *src_len, uint32_t n, uint8_t *dst, const uint64_t *dst_off,
                                 const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc, uint32_t max_len,
                                 void *stream, bool latency = false, bool need_hbm = true) {
    if (!ctx) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    hipStream_t st = (hipStream_t)stream;
    const InflateIn in = inflate_in(ctx, n, max_len, latency, need_hbm);
    const InflatePlan P = plan_inflate(in);
    int r;
    if (P.verify && (r = ctx->crcx.ensure(P.crcx_bytes))) return r;
    if (P.order && (r = ctx->order.ensure(P.order_bytes))) return r;
    if (P.rec && ((r = ctx->recs.ensure(P.recs_bytes)) || (r = ctx->bigl.ensure(P.bigl_bytes)))) return r;
    if (P.chunk_pass && (r = ctx->idx.ensure(P.idx.bytes))) return r;
    // what every launch of the call sees
    InflateArgs a{};
    a.src = src;
    a.src_off = src_off;
    a.src_len = src_len;
    a.dst = dst;
    a.dst_off = dst_off;
    a.dst_cap = dst_cap;
    a.dst_len = dst_len;
    a.rc = rc;
    a.n = n;
    a.dbg = ctx->dbg ? ctx->dbg + 16 : nullptr;
    // (a context with a dictionary: the record and lane kernels leave its dictionary members to the LDS wave
    // kernel, which decodes them behind the dictionary)
    const uint32_t dD = in.dict_len;
    a.dict = dD ? (const uint8_t *)ctx->dict.p : nullptr;
    a.dict_len = dD;
    a.dict_id = dD ? ctx->dict_id : 0u;
    if (P.verify) a.crc_expect = (uint32_t *)ctx->crcx.p;
    // the stages before the wave kernels also see the visit order
    const uint32_t *ord = nullptr;
    auto ordered = [&] {
        InflateArgs k = a;
        k.order = ord;
        return k;
    };
    if (P.order && (r = stage_order(ctx, P, src_len, n, &ord, st))) return r;
    if (P.rec && (r = stage_record(ctx, P, a, ord, st))) return r;
    if (P.lane_route) stage_lanes(ctx, P, a, ord, st);
    // indexed members (FLG = FEXTRA: the lane passes declined them), one lane per chunk
    ChunkArgs X{};
    if (P.chunk_pass && (r = chunk_pass_decode(ctx, P, ordered(), X, st))) return r;
    if (P.verify) { // CRC-32 of every member the lane decoders and the chunk pass finished (rc 0)
        a.verify_group = P.VG;
        const InflateArgs k = ordered();
        klaunch(ctx, PMC_K_INFLATE_VERIFY, st,
                [&] { hipLaunchKernelGGL(inflate_verify_kernel, dim3(P.vb), dim3(512), 0, st, k); });
    }
    if (P.chunk_pass) chunk_pass_count(ctx, P, ordered(), X, st);
    // ---- wave-per-member kernels: every member, or those the stages above left kInflateRetry ----
    a.retry_only = P.retry_only ? 1 : 0;
    if (P.count_retried) a.retried = (uint32_t *)ctx->guard.p + 4; // (pmc_ctx_guard_counts counts[4])
    a.lds_max_out = P.out_cap;
    a.lds_max_in = P.lds_max_in;
    a.dict_out = P.dict_out;
    a.dict_pass = 0;
    a.dict_last = P.dict_second ? 0u : 1u;
    if ((r = wave_lds(ctx, wave_kernel(false, dD != 0), a, "inflate_kernel<lds>", st))) return r;
    if (P.dict_second) {
        InflateArgs a2 = a;
        a2.dict_pass = 1;
        a2.dict_last = 1;
        a2.first_img = P.second.first_img;
        a2.first_in = P.second.first_in;
        a2.lds_max_out = P.second.lds_max_out;
        a2.dict_out = P.second.dict_out;
        a2.lds_max_in = P.second.lds_max_in;
        if ((r = wave_lds(ctx, wave_kernel(false, true), a2, "inflate_dict_kernel<lds>", st))) return r;
    }
    // members whose output or input exceeds the LDS image (rare: large values, or garbage
    // input longer than its ISIZE suggests) -> HBM variant; always launched because input
    // lengths are device-resident (the kernel skips members the LDS kernel handled) -- unless a
    // host-memory caller, who knows the lengths, says no member needs it
    if (P.hbm) {
        a.wave_bytes = inflate_wave_bytes(true, 0, 0);
        return launch_wave(ctx, PMC_K_INFLATE_HBM, wave_kernel(true, dD != 0), P.hbm_blocks, 4, kCrcTabBytes + 4 * a.wave_bytes,
                           a, "inflate_kernel<hbm>", st);
    }
    return PMC_OK;
}

PMC_API int pmc_gzip_compress_batch(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                    const uint32_t *src_len, uint32_t n, uint8_t *dst, const uint64_t *dst_off,
                                    const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc, uint32_t max_len,
                                    void *stream) {
    if (!ctx) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[0]);
    int r = dir_enter(ctx, 0, st);
    if (r) return r;
    // a server-sized batch of small values (<= 1,024 of <= 4 KiB: the host calls' latency-path limits)
    // takes the one-kernel path here too (400 x 4 KiB: 2.15 -> ~1 ms, round 5)
    // (not at the fast level: compress_batch_body sends every batch through the split pipeline there)
    const bool small = n <= latency_batch() && max_len <= latency_max_len();
    r = compress_batch_body(ctx, src, src_off, src_len, n, dst, dst_off, dst_cap, dst_len, rc, max_len, stream, false,
                            small);
    const int r2 = dir_leave(ctx, 0, st);
    return r ? r : r2;
}

PMC_API int pmc_gzip_decompress_batch(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                      const uint32_t *src_len, uint32_t n, uint8_t *dst, const uint64_t *dst_off,
                                      const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc, uint32_t max_len,
                                      void *stream) {
    if (!ctx) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[1]);
    int r = dir_enter(ctx, 1, st);
    if (r) return r;
    // (a server-sized GET batch, or at most 4 members per CU: the wave-only route)
    const bool small = inflate_latency(n, max_len, (uint64_t)n * max_len, ctx->cus, latency_batch(), latency_max_len(),
                                       true, kInflateLdsOut);
    r = decompress_batch_body(ctx, src, src_off, src_len, n, dst, dst_off, dst_cap, dst_len, rc, max_len, stream, small,
                              true);
    const int r2 = dir_leave(ctx, 1, st);
    return r ? r : r2;
}

// ---- ranged reads (pmc_inflate_range.hip; include/pmc_codec.h "ranged reads") ------------------------------
// plan_range (pmc_plan.hpp) -> scan, prefix sum, one lane per covered chunk, finish.  Enqueue only, no readback.
static int range_batch_body(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                            const uint32_t *range_off, const uint32_t *range_len, uint32_t n, uint8_t *dst,
                            const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc,
                            hipStream_t st) {
    int r = PMC_OK;
    if (!ctx->range_per_cu)
        ctx->range_per_cu = occupancy_blocks((const void *)inflate_range_kernel<false>, 64, kChunkLdsBytes);
    const RangePlan P = plan_range(n, (uint64_t)ctx->cus, (uint64_t)ctx->range_per_cu, kIdxScanBlock);
    if ((r = ctx->rng.ensure(P.bytes))) return r;
    InflateArgs a{};
    a.src = src;
    a.src_off = src_off;
    a.src_len = src_len;
    a.dst = dst;
    a.dst_off = dst_off;
    a.dst_cap = dst_cap;
    a.dst_len = dst_len;
    a.rc = rc;
    a.n = n;
    uint8_t *p = (uint8_t *)ctx->rng.p;
    uint64_t *pre = (uint64_t *)(p + P.idx.pre), *bsum = (uint64_t *)(p + P.idx.bsum);
    RangeArgs R{};
    R.range_off = range_off;
    R.range_len = range_len;
    R.cnt = (uint32_t *)(p + P.idx.cnt);
    R.fail = (uint32_t *)(p + P.idx.fail);
    R.pre = pre;
    R.total = (uint64_t *)(p + P.idx.total);
    R.counts = (uint64_t *)((uint8_t *)ctx->guard.p + 64);
    R.vcounts = (uint64_t *)((uint8_t *)ctx->guard.p + 96);
    R.require = ctx->range_verify ? 1 : 0;
    R.ncrc = (uint32_t *)((uint8_t *)ctx->guard.p + 112);
    R.rows = p + P.rows_off;
    R.row_per_request = P.row_per_request ? 1 : 0;
    R.off = inflate_env().wave_only ? 1 : 0;
    klaunch(ctx, PMC_K_ORDER, st, [&] {
        hipLaunchKernelGGL(inflate_range_scan_kernel, dim3(P.mb), dim3(256), 0, st, a, R);
        r = scan_u32(R.cnt, nullptr, n, pre, bsum, st);
    });
    if (r) return r; // (scan_u32 has named the launch that failed)
    klaunch(ctx, PMC_K_INFLATE_LANE, st, [&] {
        hipLaunchKernelGGL(inflate_range_kernel<false>, dim3(P.cb), dim3(64), kChunkLdsBytes, st, a, R);
        hipLaunchKernelGGL(inflate_range_kernel<true>, dim3(P.cb), dim3(64), kRangeLdsBytes, st, a, R);
        hipLaunchKernelGGL(inflate_range_finish_kernel, dim3(P.mb), dim3(256), 0, st, a, R);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_err("inflate_range_kernel", e);
        return PMC_E_NO_DEVICE;
    }
    return PMC_OK;
}

PMC_API int pmc_gzip_decompress_range_batch(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                            const uint32_t *src_len, const uint32_t *range_off,
                                            const uint32_t *range_len, uint32_t n, uint8_t *dst, const uint64_t *dst_off,
                                            const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc, void *stream) {
    if (!ctx || (n && (!src || !src_off || !src_len || !range_off || !range_len || !dst || !dst_off || !dst_cap ||
                       !dst_len || !rc)))
        return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[1]);
    int r = dir_enter(ctx, 1, st);
    if (r) return r;
    // (the direction event is recorded on every path, as pmc_gzip_decompress_batch records it: a scan may be
    // enqueued on st when a later step fails)
    r = range_batch_body(ctx, src, src_off, src_len, range_off, range_len, n, dst, dst_off, dst_cap, dst_len, rc, st);
    const int r2 = dir_leave(ctx, 1, st);
    return r ? r : r2;
}

PMC_API int pmc_ctx_range_counts(pmc_ctx *ctx, uint64_t counts[3]) {
    if (!ctx || !counts) return PMC_E_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, (uint8_t *)ctx->guard.p + 64, 24, hipMemcpyDeviceToHost));
    return PMC_OK;
}

PMC_API int pmc_ctx_set_range_verify(pmc_ctx *ctx, int mode) {
    if (!ctx || (mode != 0 && mode != 1)) return PMC_E_ARG;
    ctx->range_verify = mode;
    return PMC_OK;
}

PMC_API int pmc_ctx_get_range_verify(pmc_ctx *ctx, int *mode) {
    if (!ctx || !mode) return PMC_E_ARG;
    *mode = ctx->range_verify;
    return PMC_OK;
}

PMC_API int pmc_ctx_range_verify_counts(pmc_ctx *ctx, uint64_t counts[2]) {
    if (!ctx || !counts) return PMC_E_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, (uint8_t *)ctx->guard.p + 96, 16, hipMemcpyDeviceToHost));
    return PMC_OK;
}

// ---- ranged and growing writes (pmc_deflate_patch.hip; include/pmc_codec.h "ranged writes") ----------------
// plan_patch (pmc_plan.hpp) -> scan, prefix sum, the total read back; then rounds of whole requests, each of at
// most kPatchRoundChunks touched chunks (PMC_PATCH_ROUND_CHUNKS lowers that, for tests): tables, edge decode,
// overlay, the fast parse, emit, finish, copy.  A round's kernels are only enqueued.
static uint64_t patch_round_chunks() {
    static const uint64_t v = getenv("PMC_PATCH_ROUND_CHUNKS")
                                  ? std::min<uint64_t>(std::max<uint64_t>(1, (uint64_t)atoll(getenv("PMC_PATCH_ROUND_CHUNKS"))),
                                                       kPatchRoundChunks)
                                  : kPatchRoundChunks;
    return v;
}

static int rewrite_batch_body(pmc_ctx *ctx, PatchArgs P, hipStream_t st) {
    int r = PMC_OK;
    const uint32_t n = P.n;
    if (!ctx->patch_per_cu) {
        HIP_TRY(hipFuncSetAttribute((const void *)patch_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)patch_decode_lds()));
        ctx->patch_per_cu = occupancy_blocks((const void *)patch_decode_kernel, 64, patch_decode_lds());
    }
    const PatchPlan Q = plan_patch(n, (uint64_t)ctx->cus, kIdxScanBlock);
    if ((r = ctx->pat.ensure(Q.bytes))) return r;
    uint8_t *q = (uint8_t *)ctx->pat.p;
    uint64_t *pre = (uint64_t *)(q + Q.pre), *bsum = (uint64_t *)(q + Q.bsum);
    P.cnt = (uint32_t *)(q + Q.cnt);
    P.ka = (uint32_t *)(q + Q.ka);
    P.fail = (uint32_t *)(q + Q.fail);
    P.pfail = (int32_t *)(q + Q.pfail);
    P.lv_val = (uint32_t *)(q + Q.lv_val);
    P.seg0 = (uint32_t *)(q + Q.seg0);
    P.rlen = (uint32_t *)(q + Q.rlen);
    P.roff = (uint64_t *)(q + Q.roff);
    P.pre = pre;
    P.counts = (uint64_t *)((uint8_t *)ctx->guard.p + 128);
    // (the fast parse needs the lane order the create-time probe checked; PMC_INFLATE_WAVE=1 turns the chunk
    // decoder off, as for ranged reads)
    P.off = !ctx->lane_order_ok || inflate_env().wave_only ? 1 : 0;
    klaunch(ctx, PMC_K_ORDER, st, [&] {
        hipLaunchKernelGGL(patch_scan_kernel, dim3(Q.mb), dim3(256), 0, st, P);
        r = scan_u32(P.cnt, nullptr, n, pre, bsum, st);
    });
    if (r) return r; // (scan_u32 has named the launch that failed)
    const uint32_t nb = (n + kIdxScanBlock - 1) / kIdxScanBlock;
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bsum + nb, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t budget = patch_round_chunks();
    std::vector<uint64_t> hpre;
    if (total > budget) { // several rounds: the host cuts at request boundaries
        hpre.resize((size_t)n + 1);
        HIP_TRY(hipMemcpy(hpre.data(), pre, 8 * (size_t)n, hipMemcpyDeviceToHost));
        hpre[n] = total;
    }
    const uint64_t fwb = lv_fast_wave_bytes();
    const Launch Lp = plan_lds(ctx, (const void *)lv_fast_parse_kernel, fwb, 1ull << 40, 0);
    for (uint32_t v0 = 0; v0 < n;) {
        uint32_t v1 = n;
        uint64_t i0 = 0, items = total;
        if (!hpre.empty()) { // requests while their chunks fit, and the first one always
            i0 = hpre[v0];
            v1 = v0 + 1;
            while (v1 < n && hpre[v1 + 1] - i0 <= budget) v1++;
            items = hpre[v1] - i0;
        }
        const PatchRound R = plan_patch_round(items, (uint64_t)ctx->cus);
        if ((r = ctx->patr.ensure(R.bytes))) return r;
        uint8_t *d = (uint8_t *)ctx->patr.p;
        P.v0 = v0;
        P.v1 = v1;
        P.i0 = i0;
        P.items = items;
        P.stage = d + R.stage;
        P.tok = (uint32_t *)(d + R.tok);
        P.seg_val = (uint32_t *)(d + R.seg_val);
        P.seg_tok0 = (uint64_t *)(d + R.seg_tok0);
        P.seg_tok = (uint32_t *)(d + R.seg_tok);
        P.slots = d + R.slots;
        P.span = (uint32_t *)(d + R.span);
        P.crc = (uint32_t *)(d + R.crc);
        P.slabs = d + R.slabs;
        const uint64_t nr = v1 - v0;
        if (items) {
            klaunch(ctx, PMC_K_ORDER, st, [&] {
                const uint64_t nt = std::max<uint64_t>(nr, items);
                hipLaunchKernelGGL(patch_tables_kernel, dim3((unsigned)std::min<uint64_t>((nt + 255) / 256, 4096)),
                                   dim3(256), 0, st, P);
            });
            klaunch(ctx, PMC_K_INFLATE_LANE, st, [&] {
                const uint64_t db = std::min<uint64_t>((2 * nr + 63) / 64, (uint64_t)ctx->cus * ctx->patch_per_cu);
                hipLaunchKernelGGL(patch_decode_kernel, dim3((unsigned)std::max<uint64_t>(1, db)), dim3(64),
                                   patch_decode_lds(), st, P);
            });
            // the fast parse over the regions: a request's touched chunks are its "value"
            DeflateArgs a{};
            a.src = P.stage;
            a.src_off = P.roff;
            a.src_len = P.rlen;
            a.n = n;
            a.cap_len = kFlCap;
            a.wave_bytes = fwb;
            a.guard = (uint32_t *)ctx->guard.p;
            LargeArgs L{};
            L.src = a.src;
            L.src_off = a.src_off;
            L.src_len = a.src_len;
            L.lv_val = P.lv_val;
            L.lv_seg0 = P.seg0;
            L.seg_val = P.seg_val;
            L.seg_tok0 = P.seg_tok0;
            L.nv = n;
            L.nseg = (uint32_t)(items * kPatchSegs);
            L.tok = P.tok;
            L.seg_tok = P.seg_tok;
            L.fail = P.pfail;
            L.xfl = 4;
            L.idx_chunk = kIdxChunk;
            L.idx_crc = 1;
            klaunch(ctx, PMC_K_DEFLATE_LARGE, st, [&] {
                hipLaunchKernelGGL(patch_overlay_kernel, dim3((unsigned)std::min<uint64_t>(items, 65535)), dim3(256), 0,
                                   st, P);
                const dim3 pg((unsigned)std::min<uint64_t>(Lp.blocks, (L.nseg + Lp.wpb - 1) / Lp.wpb));
                hipLaunchKernelGGL(lv_fast_parse_kernel, pg, dim3(64 * Lp.wpb), Lp.lds, st, a, L);
            });
            klaunch(ctx, PMC_K_DEFLATE_LARGE_EMIT, st, [&] {
                hipLaunchKernelGGL(patch_emit_kernel, dim3((unsigned)(R.waves / 4)), dim3(256), patch_emit_lds(4), st, P);
            });
        }
        klaunch(ctx, PMC_K_DEFLATE_LARGE_EMIT, st, [&] {
            const uint64_t fb = std::max<uint64_t>(1, std::min<uint64_t>((nr + 3) / 4, (uint64_t)ctx->cus * 8));
            hipLaunchKernelGGL(patch_finish_kernel, dim3((unsigned)fb), dim3(256), 0, st, P);
            // request blocks x chunk blocks: enough of the second to fill the device when the requests are few
            const uint64_t gx = std::min<uint64_t>(nr, 16384);
            const uint64_t gy = std::max<uint64_t>(1, std::min<uint64_t>(64, (uint64_t)ctx->cus * 8 / gx));
            hipLaunchKernelGGL(patch_copy_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, P);
        });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            set_err("ranged-write kernels", e);
            return PMC_E_NO_DEVICE;
        }
        v0 = v1;
    }
    return PMC_OK;
}

// the two entry points: the same call, with growth refused by the scan (grow 0) or served (grow 1)
static int rewrite_range_batch(pmc_ctx *ctx, int grow, const uint8_t *src, const uint64_t *src_off,
                               const uint32_t *src_len, const uint8_t *patch, const uint64_t *patch_off,
                               const uint32_t *patch_len, const uint32_t *range_off, uint32_t n, uint8_t *dst,
                               const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc,
                               void *stream) {
    if (!ctx || (n && (!src || !src_off || !src_len || !patch || !patch_off || !patch_len || !range_off || !dst ||
                       !dst_off || !dst_cap || !dst_len || !rc)))
        return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[0]);
    int r = dir_enter(ctx, 0, st);
    if (r) return r;
    PatchArgs P{};
    P.src = src;
    P.src_off = src_off;
    P.src_len = src_len;
    P.patch = patch;
    P.patch_off = patch_off;
    P.patch_len = patch_len;
    P.range_off = range_off;
    P.dst = dst;
    P.dst_off = dst_off;
    P.dst_cap = dst_cap;
    P.dst_len = dst_len;
    P.rc = rc;
    P.n = n;
    P.grow = grow;
    r = rewrite_batch_body(ctx, P, st);
    const int r2 = dir_leave(ctx, 0, st);
    return r ? r : r2;
}

PMC_API int pmc_gzip_rewrite_range_batch(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                         const uint32_t *src_len, const uint8_t *patch, const uint64_t *patch_off,
                                         const uint32_t *patch_len, const uint32_t *range_off, uint32_t n, uint8_t *dst,
                                         const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len,
                                         int32_t *rc, void *stream) {
    return rewrite_range_batch(ctx, 0, src, src_off, src_len, patch, patch_off, patch_len, range_off, n, dst, dst_off,
                               dst_cap, dst_len, rc, stream);
}

PMC_API int pmc_gzip_grow_range_batch(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                      const uint32_t *src_len, const uint8_t *patch, const uint64_t *patch_off,
                                      const uint32_t *patch_len, const uint32_t *range_off, uint32_t n, uint8_t *dst,
                                      const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc,
                                      void *stream) {
    return rewrite_range_batch(ctx, 1, src, src_off, src_len, patch, patch_off, patch_len, range_off, n, dst, dst_off,
                               dst_cap, dst_len, rc, stream);
}

PMC_API int pmc_ctx_rewrite_counts(pmc_ctx *ctx, uint64_t counts[5]) {
    if (!ctx || !counts) return PMC_E_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, (uint8_t *)ctx->guard.p + 128, 40, hipMemcpyDeviceToHost));
    return PMC_OK;
}

PMC_API int pmc_ctx_profile(pmc_ctx *ctx, int enable) {
    if (!ctx) return PMC_E_ARG;
    ctx->prof = enable != 0;
    return PMC_OK;
}

PMC_API int pmc_ctx_kernel_times(pmc_ctx *ctx, double *ms, uint32_t *launches, int nkinds) {
    if (!ctx || !ms || !launches || nkinds < 0) return PMC_E_ARG;
    int rc = PMC_OK;
    for (auto &r : ctx->krecs) {
        float t = 0;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) rc = PMC_E_NO_DEVICE;
        if (r.kind < nkinds) {
            ms[r.kind] += t;
            launches[r.kind] += 1;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    ctx->krecs.clear();
    return rc;
}

PMC_API int pmc_crc32_batch(pmc_ctx *ctx, const uint8_t *buf, const uint64_t *off, const uint32_t *len, uint32_t n,
                            uint32_t *crc, void *stream) {
    if (!ctx || (n && (!buf || !off || !len || !crc))) return PMC_E_ARG;
    if (!n) return PMC_OK;
    const unsigned b = (unsigned)std::min<uint64_t>(((uint64_t)n + 511) / 512, (uint64_t)ctx->cus * 4);
    hipLaunchKernelGGL(crc32_batch_kernel, dim3(b), dim3(512), 0, (hipStream_t)stream, buf, off, len, (uint64_t)n, crc);
    return hipGetLastError() == hipSuccess ? PMC_OK : PMC_E_NO_DEVICE;
}

PMC_API int pmc_gzip_isize_batch(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                 const uint32_t *src_len, uint32_t n, uint32_t *isize, void *stream) {
    if (!ctx) return PMC_E_ARG;
    if (!n) return PMC_OK;
    hipLaunchKernelGGL(isize_kernel, dim3(std::min<uint32_t>((n + 255) / 256, 4096)), dim3(256), 0,
                       (hipStream_t)stream, src, src_off, src_len, n, isize);
    return hipGetLastError() == hipSuccess ? PMC_OK : PMC_E_NO_DEVICE;
}

// ---- helpers -------------------------------------------------------------------------
static dim3 grid_for(uint64_t items, int per_thread = 1) {
    uint64_t b = (items / per_thread + 255) / 256;
    return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, 1u << 16)));
}

PMC_API int pmc_gen_values(const uint8_t *corpus, uint32_t corpus_len, uint64_t seed, int kind, uint64_t first,
                           const uint64_t *index, uint32_t n, uint32_t vlen, uint8_t *dst, void *stream) {
    if (!n || !vlen || (kind == 0 && vlen > corpus_len)) return PMC_E_ARG;
    hipLaunchKernelGGL(gen_values_kernel, grid_for((uint64_t)n * ((vlen + 7) / 8)), dim3(256), 0,
                       (hipStream_t)stream, corpus, corpus_len, seed, kind, first, index, n, vlen, dst);
    return hipGetLastError() == hipSuccess ? PMC_OK : PMC_E_NO_DEVICE;
}

PMC_API int pmc_fill_layout(uint64_t *off, uint32_t *len, uint32_t *cap, uint32_t n, uint64_t stride, uint32_t vlen,
                            uint32_t capv, void *stream) {
    if (!n) return PMC_OK;
    hipLaunchKernelGGL(fill_layout_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, off, len, cap, n, stride,
                       vlen, capv);
    return hipGetLastError() == hipSuccess ? PMC_OK : PMC_E_NO_DEVICE;
}

PMC_API int pmc_compare_values(const uint8_t *a, const uint64_t *a_off, const uint8_t *b, const uint64_t *b_off,
                               const uint32_t *len, const uint32_t *len_b, uint32_t n, uint32_t *mismatches,
                               void *stream) {
    if (!n) return PMC_OK;
    hipLaunchKernelGGL(compare_values_kernel, dim3(std::min<uint32_t>((n + 3) / 4, 8192)), dim3(256), 0,
                       (hipStream_t)stream, a, a_off, b, b_off, len, len_b, n, mismatches);
    return hipGetLastError() == hipSuccess ? PMC_OK : PMC_E_NO_DEVICE;
}

PMC_API int pmc_route_keys(uint64_t first, uint32_t n, uint32_t num_shards, uint32_t n_gpus, uint8_t *gpu,
                           void *stream) {
    if (!n || !num_shards || !n_gpus) return PMC_E_ARG;
    hipLaunchKernelGGL(route_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, first, n, num_shards, n_gpus,
                       gpu);
    return hipGetLastError() == hipSuccess ? PMC_OK : PMC_E_NO_DEVICE;
}

// Diagnostics: device buffer of 32 uint64 that PMC_STAMPS builds add per-phase cycles into.
PMC_API int pmc_debug_stamps(pmc_ctx *ctx, uint64_t *dev_buf) {
    if (!ctx) return PMC_E_ARG;
    ctx->dbg = dev_buf;
    return PMC_OK;
}

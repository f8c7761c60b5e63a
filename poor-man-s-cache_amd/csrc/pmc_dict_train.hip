// pmc_dict_train.hip -- dictionary training (include/pmc_codec.h "dictionary training"; the normative statement is
// tests/dict_train_model.py): count, then per epoch score and select, then assemble.  A fixed sequence of launches
// on the caller's stream: nothing is read back, and no block waits for another.  Every reduction is an integer one
// under a total order (score, then lowest sample, then lowest start), so the bytes do not depend on scheduling.
// Compiled into the unity TU after pmc_host.hip (uses pmc_ctx, DevBuf, dir_enter / dir_leave and HostCall).
namespace pmc {

struct TrainSlot { // a block's, then an epoch's, best candidate; score 0 stands for none
    uint64_t score;
    uint32_t i, q;
};
static_assert(sizeof(TrainSlot) == kTrainSlotBytes, "plan_dict_train's slot");

struct TrainArgs {
    const uint8_t *src;
    const uint64_t *src_off;
    const uint32_t *src_len;
    uint32_t n;
    uint32_t *freq;   // 2^F slots
    uint32_t *nsel;   // segments selected so far
    TrainSlot *slots; // one per block of an epoch's score launch
    uint8_t *rows;    // row m: the 64 bytes of selection m
    uint8_t *dict;
    uint32_t *dict_len;
};

// starts scored per pass over a sample, and the positions hashed for them: W - 1 in front (for dist) and W - 1
// behind (the last start's window)
constexpr uint32_t kTrainTile = 256, kTrainTilePos = kTrainTile + 2 * (kTrainWin - 1);

// The 8 bytes at p, little endian, from aligned dword loads: only dwords that hold one of the 8 bytes are read, so
// no load leaves the 4-byte-aligned span around the sample.
__device__ __forceinline__ uint64_t train_load8(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t s = (uint32_t)(a & 3) * 8;
    const uint32_t *w = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t w0 = w[0], w1 = w[1];
    if (s == 0) return w0 | ((uint64_t)w1 << 32);
    const uint32_t w2 = w[2];
    const uint32_t lo = (w0 >> s) | (w1 << (32 - s)), hi = (w1 >> s) | (w2 << (32 - s));
    return lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ uint32_t train_hash(uint64_t w) { return (uint32_t)((w * kTrainMult) >> (64 - kTrainBits)); }
__device__ __forceinline__ uint32_t train_len(const TrainArgs &a, uint32_t i) { return min(a.src_len[i], kDictSpan); }

__device__ __forceinline__ bool train_better(uint64_t s, uint32_t i, uint32_t q, const TrainSlot &b) {
    return s > b.score || (s == b.score && (i < b.i || (i == b.i && q < b.q)));
}
// the wave's best in every lane
__device__ __forceinline__ TrainSlot train_wave_best(TrainSlot b) {
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t s = __shfl_xor((unsigned long long)b.score, off);
        const uint32_t i = __shfl_xor(b.i, off), q = __shfl_xor(b.q, off);
        if (train_better(s, i, q, b)) b = TrainSlot{s, i, q};
    }
    return b;
}

// COUNT: one wave per sample, lanes over positions.
__global__ __launch_bounds__(64) void dict_train_count_kernel(TrainArgs a) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const uint32_t len = train_len(a, i);
        const uint8_t *v = a.src + a.src_off[i];
        for (uint32_t p = lane; p + kTrainKmer <= len; p += 64) atomicAdd(&a.freq[train_hash(train_load8(v + p))], 1u);
    }
}

// SCORE of one epoch's samples [lo, hi): one wave per sample, a tile of starts at a time.  Per position of the
// tile: its hash, the table's count and prev = p - dist (the nearest equal hash at most W - 1 back, -1 for none) in
// LDS; then one lane per start sums the counts of the positions whose prev lies before the start.
__global__ __launch_bounds__(64) void dict_train_score_kernel(TrainArgs a, uint32_t lo, uint32_t hi) {
    __shared__ uint32_t sh[kTrainTilePos], sf[kTrainTilePos];
    __shared__ int32_t sprev[kTrainTilePos];
    const uint32_t lane = threadIdx.x;
    TrainSlot best{0, ~0u, ~0u};
    for (uint32_t i = lo + blockIdx.x; i < hi; i += gridDim.x) {
        const uint32_t len = train_len(a, i);
        if (len < kTrainSeg) continue; // (the whole wave: i and len are uniform)
        const uint8_t *v = a.src + a.src_off[i];
        const uint32_t nq = len - kTrainSeg + 1;
        for (uint32_t q0 = 0; q0 < nq; q0 += kTrainTile) {
            const uint32_t tq = min(kTrainTile, nq - q0);
            const uint32_t p0 = q0 >= kTrainWin - 1 ? q0 - (kTrainWin - 1) : 0;
            const uint32_t p1 = q0 + tq + kTrainWin - 1; // <= len - 7: every position has its 8 bytes
            for (uint32_t t = lane; p0 + t < p1; t += 64) {
                const uint32_t h = train_hash(train_load8(v + p0 + t));
                sh[t] = h;
                sf[t] = a.freq[h];
            }
            __syncthreads();
            for (uint32_t p = q0 + lane; p < p1; p += 64) {
                const uint32_t t = p - p0, h = sh[t];
                int32_t prev = -1;
                for (uint32_t d = kTrainWin - 1; d >= 1; d--) // (downwards: the smallest d is written last)
                    if (d <= t && sh[t - d] == h) prev = (int32_t)(p - d);
                sprev[t] = prev;
            }
            __syncthreads();
            for (uint32_t q = q0 + lane; q < q0 + tq; q += 64) {
                uint64_t s = 0;
                for (uint32_t j = 0; j < kTrainWin; j++) {
                    const uint32_t t = q + j - p0;
                    s += sprev[t] < (int32_t)q ? sf[t] : 0u;
                }
                // a lane meets its candidates in rising (i, q): strictly greater keeps the lowest
                if (s > best.score) best = TrainSlot{s, i, q};
            }
            __syncthreads();
        }
    }
    best = train_wave_best(best);
    if (lane == 0) a.slots[blockIdx.x] = best;
}

// SELECT, one wave: the epoch's best of the block slots; its 57 table slots zeroed, its bytes to row nsel.
__global__ __launch_bounds__(64) void dict_train_select_kernel(TrainArgs a, uint32_t nslots) {
    const uint32_t lane = threadIdx.x;
    TrainSlot best{0, ~0u, ~0u};
    for (uint32_t k = lane; k < nslots; k += 64) {
        const TrainSlot s = a.slots[k];
        if (train_better(s.score, s.i, s.q, best)) best = s;
    }
    best = train_wave_best(best);
    if (best.score == 0) return;
    const uint32_t m = *a.nsel;
    const uint8_t *seg = a.src + a.src_off[best.i] + best.q;
    if (lane < kTrainWin) a.freq[train_hash(train_load8(seg + lane))] = 0;
    a.rows[(uint64_t)m * kTrainSeg + lane] = seg[lane];
    __syncthreads(); // every lane has read nsel
    if (lane == 0) *a.nsel = m + 1;
}

// ASSEMBLY: the rows in reverse order of selection, and the length.
__global__ __launch_bounds__(256) void dict_train_final_kernel(TrainArgs a) {
    const uint32_t m = *a.nsel;
    for (uint32_t t = threadIdx.x; t < m * kTrainSeg; t += 256)
        a.dict[(uint64_t)(m - 1 - t / kTrainSeg) * kTrainSeg + t % kTrainSeg] = a.rows[t];
    if (threadIdx.x == 0) *a.dict_len = m * kTrainSeg;
}

} // namespace pmc

namespace {

bool dict_train_bad_args(pmc_ctx *ctx, const void *src, const void *src_off, const void *src_len, uint32_t n,
                         uint32_t dict_size, const void *dict, const void *dict_len) {
    return !ctx || !dict_train_args_ok(n, dict_size) || !src || !src_off || !src_len || !dict || !dict_len;
}

// (the caller holds dir_mu[0]; the launches are left out of the per-kind timing)
int dict_train_body(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len, uint32_t n,
                    uint32_t dict_size, uint8_t *dict, uint32_t *dict_len, hipStream_t st) {
    const DictTrainPlan P = plan_dict_train(n, dict_size, (uint64_t)ctx->cus);
    int r = ctx->train.ensure(P.bytes);
    if (r) return r;
    uint8_t *p = (uint8_t *)ctx->train.p;
    TrainArgs a{src, src_off, src_len, n, (uint32_t *)(p + P.table), (uint32_t *)(p + P.nsel),
                (TrainSlot *)(p + P.slots), p + P.rows, dict, dict_len};
    hipError_t e = hipMemsetAsync(p, 0, P.slots, st); // the table and the count of selections
    if (e != hipSuccess) {
        set_err("dict_train: hipMemsetAsync", e);
        return PMC_E_NO_DEVICE;
    }
    hipLaunchKernelGGL(dict_train_count_kernel, dim3(P.count_blocks), dim3(64), 0, st, a);
    for (uint32_t ep = 0; ep < P.E; ep++) {
        const uint32_t nb = P.blocks(ep);
        if (!nb) continue; // an empty epoch selects nothing
        hipLaunchKernelGGL(dict_train_score_kernel, dim3(nb), dim3(64), 0, st, a, P.lo(ep), P.hi(ep));
        hipLaunchKernelGGL(dict_train_select_kernel, dim3(1), dim3(64), 0, st, a, nb);
    }
    hipLaunchKernelGGL(dict_train_final_kernel, dim3(1), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err("dict_train kernels", e);
        return PMC_E_NO_DEVICE;
    }
    return PMC_OK;
}

} // namespace

PMC_API int pmc_dict_train_batch(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                                 uint32_t n, uint32_t dict_size, uint8_t *dict, uint32_t *dict_len, void *stream) {
    if (dict_train_bad_args(ctx, src, src_off, src_len, n, dict_size, dict, dict_len)) return PMC_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[0]);
    int r = dir_enter(ctx, 0, st);
    if (r) return r;
    r = dict_train_body(ctx, src, src_off, src_len, n, dict_size, dict, dict_len, st);
    const int r2 = dir_leave(ctx, 0, st);
    return r ? r : r2;
}

// Host samples: packed (each truncated to the span it counts for) behind their offsets and lengths in the
// context's staging buffer, trained on the context's stream, the result copied back.
PMC_API int pmc_dict_train_host(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                                uint32_t n, uint32_t dict_size, uint8_t *dict, uint32_t *dict_len) {
    if (dict_train_bad_args(ctx, src, src_off, src_len, n, dict_size, dict, dict_len)) return PMC_E_ARG;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += std::min(src_len[i], kDictSpan);
    if (total > kTrainHostBytes) return PMC_E_ARG;
    HostCall guard(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    // u64 offsets | u32 lengths | u32 dict_len | the dictionary | the bytes (each region 16-byte aligned)
    const uint64_t o_len = 8ull * n, o_dl = (o_len + 4ull * n + 15) & ~15ull, o_dict = o_dl + 16;
    const uint64_t o_src = o_dict + PMC_DICT_MAX, bytes = o_src + total + 16;
    std::vector<uint8_t> h(bytes);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = std::min(src_len[i], kDictSpan);
        memcpy(h.data() + 8ull * i, &at, 8);
        memcpy(h.data() + o_len + 4ull * i, &len, 4);
        memcpy(h.data() + o_src + at, src + src_off[i], len);
        at += len;
    }
    int r = ctx->staging.ensure(bytes);
    if (r) return r;
    uint8_t *d = (uint8_t *)ctx->staging.p;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, st));
    r = pmc_dict_train_batch(ctx, d + o_src, (const uint64_t *)d, (const uint32_t *)(d + o_len), n, dict_size,
                             d + o_dict, (uint32_t *)(d + o_dl), st);
    if (r) {
        (void)hipStreamSynchronize(st); // launches already queued read the staging
        return r;
    }
    std::vector<uint8_t> back(16 + PMC_DICT_MAX);
    HIP_TRY(hipMemcpyAsync(back.data(), d + o_dl, back.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t got = 0;
    memcpy(&got, back.data(), 4);
    if (got > dict_size) return PMC_E_NO_DEVICE; // (cannot happen: at most E selections)
    memcpy(dict, back.data() + 16, got);
    *dict_len = got;
    return PMC_OK;
}

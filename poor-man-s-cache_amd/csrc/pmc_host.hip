// pmc_host.hip -- the host-memory entries of the C-ABI (include/pmc_codec.h): pmc_gzip_*_batch_host, the
// single-value pmc_gzip_compress / pmc_gzip_decompress and pmc_gzip_*_batch_pinned.
//
// Host-resident batches: pinned staging, H2D -> kernels -> D2H.  What a call stages where, which route it takes
// and what a pinned call's chunks cover is pmc_plan.hpp's (HostStage, plan_host_batch, plan_pinned_chunk,
// PinnedSlot); here are the buffers, copies, launches and events.  Compiled into the unity TU after
// pmc_capi.hip (uses pmc_ctx, DevBuf, HostBuf, the batch bodies and scan_u32).
#include <chrono>
#include <condition_variable>
#include <functional>
#include <thread>

#include <unistd.h>

namespace {
enum Dir { kCompress, kDecompress };

// A host-API call holds its context's lock (the staging buffers, pinned pipe and default context
// are shared by every thread that calls the drop-in) and leaves the caller's current device as
// it found it.
struct HostCall {
    std::lock_guard<std::mutex> lock;
    int prev = -1;
    explicit HostCall(pmc_ctx *ctx) : lock(ctx->host_mu) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~HostCall() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Per-value copies between the caller's buffers and the staging area: one job per value, spread over a
// small pool of persistent host threads once a call moves enough bytes that one core's memcpy (~10 GB/s)
// would show beside the kernels (a 4,096 x 4 KiB batch is 16 MiB in and 17 MiB of slots out): one part per
// MiB, at most 8 parts (PMC_HOST_THREADS overrides).  Threads spawned per call cost more than they saved
// at 16 parts (unpack 0.43 -> 0.7 ms), so the pool's workers live for the process and wait on a condition.
class CopyPool {
  public:
    static CopyPool &get() {
        static CopyPool *p = new CopyPool(); // (never destroyed: workers may outlive static destructors)
        return *p;
    }
    unsigned parts() const { return nthreads + 1; }
    // runs part(k) for k = 0 .. t - 1 (t <= parts()), part 0 on the calling thread
    template <class F>
    void run(unsigned t, F part) {
        // Inline on the calling thread when: one part; a process forked after the pool started (the child
        // has no workers); or the pool is busy with another context's copies (a server's SET and
        // GET contexts copy at the same time: the second caller does its own copies instead of waiting).
        std::unique_lock<std::mutex> one(run_mu, std::defer_lock);
        if (t <= 1 || getpid() != owner || !one.try_lock()) {
            for (unsigned k = 0; k < t; k++) part(k);
            return;
        }
        std::unique_lock<std::mutex> lk(mu);
        fn = [&part](unsigned k) { part(k); };
        want = t - 1;
        taken = 0;
        left = t - 1;
        gen++;
        cv.notify_all();
        lk.unlock();
        part(0u);
        lk.lock();
        done.wait(lk, [&] { return left == 0; });
        fn = nullptr;
    }

  private:
    CopyPool() : owner(getpid()) {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const unsigned cap = getenv("PMC_HOST_THREADS") ? (unsigned)std::max(1, atoi(getenv("PMC_HOST_THREADS")))
                                                        : std::min(8u, hw);
        nthreads = cap - 1;
        for (unsigned k = 0; k < nthreads; k++) std::thread([this] { loop(); }).detach();
    }
    void loop() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return gen != seen && taken < want; });
            seen = gen;
            const unsigned k = ++taken; // parts 1 .. want
            auto f = fn;
            lk.unlock();
            f(k);
            lk.lock();
            if (--left == 0) done.notify_one();
        }
    }
    const pid_t owner; // the process whose threads these workers are
    std::mutex mu, run_mu;
    std::condition_variable cv, done;
    std::function<void(unsigned)> fn;
    unsigned nthreads = 0, want = 0, taken = 0, left = 0;
    uint64_t gen = 0;
};

template <class F>
void par_values(uint32_t n, uint64_t bytes, F job) {
    CopyPool &P = CopyPool::get();
    const unsigned t = (unsigned)std::min<uint64_t>({(uint64_t)P.parts(), (uint64_t)n, std::max<uint64_t>(1, bytes >> 20)});
    P.run(t, [&](unsigned k) {
        const uint32_t a = (uint32_t)((uint64_t)n * k / t), b = (uint32_t)((uint64_t)n * (k + 1) / t);
        for (uint32_t i = a; i < b; i++) job(i);
    });
}

double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the caller's arrays of a host-memory batch call (include/pmc_codec.h; dst_off null: packed slots)
struct HostArgs {
    const uint8_t *src;
    const uint64_t *src_off;
    const uint32_t *src_len;
    uint32_t n;
    uint8_t *dst;
    const uint64_t *dst_off;
    const uint32_t *dst_cap;
    uint32_t *dst_len;
    int32_t *rc;
};

int host_batch_locked(pmc_ctx *ctx, Dir dir, const HostArgs &A, bool force_pipeline);

// The staging of a call of `bytes` bytes, host side *hp and device side *dp.  The latency path's kernel reads
// its inputs from, and writes its outputs to, coherent host memory in place: no H2D / D2H copies (each a
// runtime copy kernel of its own) around its one launch.
int host_buffers(pmc_ctx *ctx, bool zero_copy, uint64_t bytes, uint8_t **hp, uint8_t **dp) {
    int r;
    if (zero_copy) {
        ctx->zc.flags = hipHostMallocCoherent;
        const void *old = ctx->zc.p;
        r = ctx->zc.ensure(bytes);
        if (r) return r;
        if (ctx->zc.p != old) ctx->zc_dev = nullptr; // (a new buffer: its device address is looked up below)
        if (!ctx->zc_dev) {
            void *d = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&d, ctx->zc.p, 0));
            ctx->zc_dev = d;
        }
        *hp = (uint8_t *)ctx->zc.p;
        *dp = (uint8_t *)ctx->zc_dev;
    } else {
        r = ctx->pinned.ensure(bytes);
        if (r) return r;
        r = ctx->staging.ensure(bytes);
        if (r) return r;
        *hp = (uint8_t *)ctx->pinned.p;
        *dp = (uint8_t *)ctx->staging.p;
    }
    return PMC_OK;
}

// Step 1: the lengths and capacities into the staging's arrays, the source bytes packed behind them.
void host_fill(const HostStage &L, const HostArgs &A) {
    L.fill(A.src_len, A.dst_cap);
    par_values(A.n, L.in_bytes, [&](uint32_t i) { memcpy(L.src.h + L.soff.h[i], A.src + A.src_off[i], A.src_len[i]); });
}

// Step 2: the batch's kernels over the device side of the staging.
int host_enqueue(pmc_ctx *ctx, Dir dir, const HostBatchPlan &P, const HostStage &L, uint32_t n, hipStream_t st) {
    const int d = dir == kCompress ? 0 : 1;
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[d]);
    int e = dir_enter(ctx, d, st);
    if (e) return e;
    e = dir == kCompress ? compress_batch_body(ctx, L.src.d, L.soff.d, L.slen.d, n, L.dst.d, L.doff.d, L.dcap.d, L.dlen.d,
                                               L.rc.d, (uint32_t)P.max_len, st, P.latency)
                         : decompress_batch_body(ctx, L.src.d, L.soff.d, L.slen.d, n, L.dst.d, L.doff.d, L.dcap.d, L.dlen.d,
                                                 L.rc.d, (uint32_t)P.max_len, st, P.latency, P.need_hbm);
    const int e2 = dir_leave(ctx, d, st);
    return e ? e : e2;
}

// Step 3, a latency-path compress: that path launches no retry pass, so the values its kernel declined (a
// lane-order guard fired) are redone, alone, by a pipeline call (its gated HBM pass), straight into the
// caller's buffers.  redone[i] marks them (empty: there were none).
int host_redo(pmc_ctx *ctx, Dir dir, const HostStage &L, const HostArgs &A, std::vector<uint8_t> &redone) {
    std::vector<uint32_t> redo;
    for (uint32_t i = 0; i < A.n; i++)
        if (L.rc.h[i] == kDeflateRetry) redo.push_back(i);
    if (redo.empty()) return PMC_OK;
    redone.assign(A.n, 0);
    ctx->latency_redone++;
    const uint32_t m = (uint32_t)redo.size();
    std::vector<uint64_t> r_soff(m), r_doff(m);
    std::vector<uint32_t> r_slen(m), r_cap(m), r_dlen(m);
    std::vector<int32_t> r_rc(m);
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = redo[k];
        r_soff[k] = A.src_off[i];
        r_slen[k] = A.src_len[i];
        r_cap[k] = A.dst_cap[i];
        r_doff[k] = A.dst_off ? A.dst_off[i] : L.doff.h[i];
        redone[i] = 1;
    }
    const HostArgs R{A.src, r_soff.data(), r_slen.data(), m, A.dst, r_doff.data(), r_cap.data(), r_dlen.data(), r_rc.data()};
    const int r = host_batch_locked(ctx, dir, R, true);
    if (r) return r;
    for (uint32_t k = 0; k < m; k++) {
        L.rc.h[redo[k]] = r_rc[k];
        L.dlen.h[redo[k]] = r_dlen[k];
    }
    return PMC_OK;
}

// Step 4: verdicts and lengths to the caller, each successful output from its staging slot to its place in
// dst (redone values are in place already).  Returns the output bytes moved.
uint64_t host_unpack(const HostStage &L, const HostArgs &A, const std::vector<uint8_t> &redone) {
    auto skip = [&](uint32_t i) { return L.rc.h[i] != 0 || (!redone.empty() && redone[i]); };
    uint64_t moved = 0;
    for (uint32_t i = 0; i < A.n; i++) {
        A.rc[i] = L.rc.h[i];
        A.dst_len[i] = L.dlen.h[i];
        if (!skip(i)) moved += L.dlen.h[i];
    }
    par_values(A.n, moved, [&](uint32_t i) {
        if (skip(i)) return;
        const uint64_t to = A.dst_off ? A.dst_off[i] : L.doff.h[i];
        memcpy(A.dst + to, L.dst.h + L.doff.h[i], L.dlen.h[i]);
    });
    return moved;
}

// (the caller holds ctx->host_mu; force_pipeline: the throughput route whatever the batch's size)
int host_batch_locked(pmc_ctx *ctx, Dir dir, const HostArgs &A, bool force_pipeline) {
    if (A.n == 0) return PMC_OK;
    static const bool trace = getenv("PMC_HOST_TRACE") && atoi(getenv("PMC_HOST_TRACE"));
    double t[8] = {};
    if (trace) t[0] = now_us();
    HIP_TRY(hipSetDevice(ctx->device));
    const HostBatchPlan P = plan_host_batch({dir == kCompress, A.n, A.src_len, A.dst_cap, (uint64_t)ctx->cus,
                                             level_is_fast(ctx->level), ctx->lane_order_ok, latency_batch(),
                                             latency_max_len(), kInflateLdsOut, force_pipeline});
    ctx->path_calls[P.path]++;
    const bool zc = P.latency;
    uint8_t *hp, *dp;
    int r = host_buffers(ctx, zc, HostStage(A.n, P.in_bytes, P.out_bytes).bytes(), &hp, &dp);
    if (r) return r;
    const HostStage L(A.n, P.in_bytes, P.out_bytes, hp, dp);

    host_fill(L, A);
    if (trace) t[1] = now_us();

    hipStream_t st = ctx->stream;
    if (!zc) HIP_TRY(hipMemcpyAsync(dp, hp, L.down, hipMemcpyHostToDevice, st));
    r = host_enqueue(ctx, dir, P, L, A.n, st);
    if (r) {
        // kernels already queued may still read or write the staging (in zero-copy mode the host
        // buffers themselves), which the next call refills: let them drain before returning
        (void)hipStreamSynchronize(st);
        return r;
    }
    if (trace) t[2] = now_us();
    if (!zc) HIP_TRY(hipMemcpyAsync(L.dlen.h, L.dlen.d, L.up, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    std::vector<uint8_t> redone;
    if (zc && dir == kCompress && (r = host_redo(ctx, dir, L, A, redone))) return r;
    if (trace) t[3] = now_us();

    const uint64_t moved = host_unpack(L, A, redone);
    if (trace) {
        t[4] = now_us();
        fprintf(stderr,
                "pmc_host_trace %s n=%u in=%llu out=%llu path=%s stage_us=%.1f enqueue_us=%.1f wait_us=%.1f "
                "unpack_us=%.1f total_us=%.1f\n",
                dir == kCompress ? "compress" : "decompress", A.n, (unsigned long long)P.in_bytes,
                (unsigned long long)moved, P.latency ? "latency" : "pipeline", t[1] - t[0], t[2] - t[1], t[3] - t[2],
                t[4] - t[3], t[4] - t[0]);
    }
    return PMC_OK;
}

int host_batch(pmc_ctx *ctx, Dir dir, const HostArgs &A) {
    if (!ctx) return PMC_E_ARG;
    if (A.n == 0) return PMC_OK;
    HostCall guard(ctx);
    return host_batch_locked(ctx, dir, A, false);
}

// Rebases one chunk's offsets onto its device copy: src_off -= sb, dst_off -= db (dst_off may be null).
__global__ void rebase_kernel(uint64_t *soff, uint64_t *doff, uint32_t n, uint64_t sb, uint64_t db) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        soff[i] -= sb;
        if (doff) doff[i] -= db;
    }
}

// One wave per member: slot bytes dst[doff[i] ..+ len[i]) -> packed[poff[i] ..) (rc[i] != 0: none).
__global__ __launch_bounds__(256) void compact_kernel(const uint8_t *dst, const uint64_t *doff, const uint32_t *len,
                                                      const int32_t *rc, const uint64_t *poff, uint32_t n,
                                                      uint8_t *packed) {
    const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        if (rc[i] != 0) continue;
        const uint8_t *a = dst + doff[i];
        uint8_t *b = packed + poff[i];
        for (uint32_t k = lane; k < len[i]; k += 64) b[k] = a[k];
    }
}

int pipe_init(pmc_ctx *ctx) {
    auto &P = ctx->pipe;
    if (P.h2d) return PMC_OK;
    HIP_TRY(hipStreamCreateWithFlags(&P.h2d, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&P.d2h, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        HIP_TRY(hipEventCreateWithFlags(&P.in[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&P.out[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&P.done[k], hipEventDisableTiming));
    }
    return P.total.ensure(64);
}

// Pinned host batch, chunked and software-pipelined over three streams (s = c & 1):
//   h2d:    offsets/lengths/caps of chunk c, then its source byte range  -> event in[s]
//   stream: rebase offsets, the codec kernels                            -> event out[s]
//   d2h:    dst_len, rc, then the chunk's destination bytes              -> event done[s]
// and chunk c + 2 reuses slot s after done[s].  Chunk c's source bytes are the range
// [min src_off, max src_off + src_len) of its values (packed layouts copy exactly their bytes).
// Destinations, three ways:
//   tiled slots (dst_off given, and the chunk's slots tile one range in index order:
//     dst_off[i + 1] == dst_off[i] + dst_cap[i]): the range is copied back whole, straight into dst;
//   any other slot layout (gaps, permuted or interleaved slots): the device compacts the chunk's
//     outputs, they land in a pinned bounce buffer and the host copies each output to its dst_off,
//     so no byte outside [dst_off[i], dst_off[i] + dst_len[i]) of a successful value is written;
//   packed mode (dst_off null): the compacted bytes are appended to dst.
// A compacted chunk's device slots are laid out by a scan of dst_cap, its results compacted by a
// scan of dst_len (rc != 0 -> 0 bytes); the host waits for chunk c's byte total (on the compute
// stream, after its kernels) only once chunk c + 1's kernels are enqueued, so the device never idles.
int pinned_batch_run(pmc_ctx *ctx, Dir dir, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                     uint32_t n, uint8_t *dst, const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len,
                     int32_t *rc, uint32_t max_len, uint32_t chunk) {
    if (!ctx || !src || !src_off || !src_len || !dst || !dst_cap || !dst_len || !rc) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    int r = pipe_init(ctx);
    if (r) return r;
    auto &P = ctx->pipe;
    const bool packed = dst_off == nullptr;
    const PinnedChunks C = pinned_chunk_of(n, chunk);
    chunk = C.chunk;
    const uint32_t nchunks = C.nchunks;
    volatile uint64_t *h_total = (volatile uint64_t *)P.total.p;  // chunk totals, slot s at [s]
    uint8_t *d_pk[2] = {nullptr, nullptr};
    uint64_t out_pos = 0;
    // slot mode, compacted chunk: its outputs wait in bounce[s] until done[s], then go to dst_off
    struct Pend {
        bool on = false;
        uint32_t a = 0, m = 0;
    } pend[2];
    auto scatter = [&](uint32_t s) -> int {
        if (!pend[s].on) return PMC_OK;
        HIP_TRY(hipEventSynchronize(P.done[s]));
        const uint8_t *b = (const uint8_t *)P.bounce[s].p;
        uint64_t p = 0;
        for (uint32_t i = pend[s].a; i < pend[s].a + pend[s].m; i++)
            if (rc[i] == 0) {
                memcpy(dst + dst_off[i], b + p, dst_len[i]);
                p += dst_len[i];
            }
        pend[s].on = false;
        return PMC_OK;
    };
    // compacted chunk c's bytes go back once its total is known (called after chunk c + 1 is enqueued)
    auto finish = [&](uint32_t c) -> int {
        const uint32_t s = c & 1;
        HIP_TRY(hipEventSynchronize(P.out[s]));
        const uint64_t tot = h_total[s];
        uint8_t *to = dst + out_pos;
        if (!packed) {
            int e = scatter(s);  // chunk c - 2's outputs leave bounce[s] first
            if (e) return e;
            if ((e = P.bounce[s].ensure(tot + 64))) return e;
            to = (uint8_t *)P.bounce[s].p;
            pend[s].on = true;
            pend[s].a = c * chunk;
            pend[s].m = std::min<uint32_t>(chunk, n - c * chunk);
        }
        HIP_TRY(hipStreamWaitEvent(P.d2h, P.out[s], 0));
        if (tot) HIP_TRY(hipMemcpyAsync(to, d_pk[s], tot, hipMemcpyDeviceToHost, P.d2h));
        HIP_TRY(hipEventRecord(P.done[s], P.d2h));
        if (packed) out_pos += tot;
        return PMC_OK;
    };
    int64_t unfinished = -1;  // a compacted chunk whose D2H is not enqueued yet
    for (uint32_t c = 0; c < nchunks; c++) {
        const uint32_t a = c * chunk, m = std::min<uint32_t>(chunk, n - a), s = c & 1;
        const PinnedChunk K = plan_pinned_chunk(src_off, src_len, dst_off, dst_cap, a, m);
        const uint64_t need = PinnedSlot(m, K).need;
        if (need > P.slot[s].cap) {
            // the slot's previous chunk must have drained before it is reallocated
            if (P.busy[s]) HIP_TRY(hipEventSynchronize(P.done[s]));
            r = P.slot[s].ensure(need + need / 8);
            if (r) return r;
            P.busy[s] = false;
        }
        const PinnedSlot L(m, K, P.slot[s].p);
        d_pk[s] = L.packed.d;
        if (P.busy[s]) HIP_TRY(hipStreamWaitEvent(P.h2d, P.done[s], 0));
        HIP_TRY(hipMemcpyAsync(L.soff.d, src_off + a, m * 8ull, hipMemcpyHostToDevice, P.h2d));
        if (!K.compact) HIP_TRY(hipMemcpyAsync(L.doff.d, dst_off + a, m * 8ull, hipMemcpyHostToDevice, P.h2d));
        HIP_TRY(hipMemcpyAsync(L.slen.d, src_len + a, m * 4ull, hipMemcpyHostToDevice, P.h2d));
        HIP_TRY(hipMemcpyAsync(L.dcap.d, dst_cap + a, m * 4ull, hipMemcpyHostToDevice, P.h2d));
        HIP_TRY(hipMemcpyAsync(L.src.d, src + K.sb, K.se - K.sb, hipMemcpyHostToDevice, P.h2d));
        HIP_TRY(hipEventRecord(P.in[s], P.h2d));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, P.in[s], 0));
        hipLaunchKernelGGL(rebase_kernel, dim3(std::min<uint32_t>((m + 255) / 256, 1024)), dim3(256), 0, ctx->stream,
                           L.soff.d, K.compact ? nullptr : L.doff.d, m, K.sb, K.db);
        HIP_TRY(hipGetLastError());
        if (K.compact && (r = scan_u32(L.dcap.d, nullptr, m, L.doff.d, L.bsum.d, ctx->stream))) return r;
        r = dir == kCompress
                ? pmc_gzip_compress_batch(ctx, L.src.d, L.soff.d, L.slen.d, m, L.dst.d, L.doff.d, L.dcap.d, L.dlen.d,
                                          L.rc.d, max_len, ctx->stream)
                : pmc_gzip_decompress_batch(ctx, L.src.d, L.soff.d, L.slen.d, m, L.dst.d, L.doff.d, L.dcap.d, L.dlen.d,
                                            L.rc.d, max_len, ctx->stream);
        if (r) return r;
        if (K.compact) {
            if ((r = scan_u32(L.dlen.d, L.rc.d, m, L.poff.d, L.bsum.d, ctx->stream))) return r;
            hipLaunchKernelGGL(compact_kernel, dim3(std::min<uint32_t>((m + 3) / 4, 8192)), dim3(256), 0,
                               ctx->stream, L.dst.d, L.doff.d, L.dlen.d, L.rc.d, L.poff.d, m, L.packed.d);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(dst_len + a, L.dlen.d, m * 4ull, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipMemcpyAsync(rc + a, L.rc.d, m * 4ull, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipMemcpyAsync((void *)(h_total + s), L.bsum.d + K.nb, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipEventRecord(P.out[s], ctx->stream));
        } else {
            HIP_TRY(hipEventRecord(P.out[s], ctx->stream));
            HIP_TRY(hipStreamWaitEvent(P.d2h, P.out[s], 0));
            HIP_TRY(hipMemcpyAsync(dst_len + a, L.dlen.d, m * 4ull, hipMemcpyDeviceToHost, P.d2h));
            HIP_TRY(hipMemcpyAsync(rc + a, L.rc.d, m * 4ull, hipMemcpyDeviceToHost, P.d2h));
            HIP_TRY(hipMemcpyAsync(dst + K.db, L.dst.d, K.de - K.db, hipMemcpyDeviceToHost, P.d2h));
            HIP_TRY(hipEventRecord(P.done[s], P.d2h));
        }
        P.busy[s] = true;
        if (unfinished >= 0 && (r = finish((uint32_t)unfinished))) return r;
        unfinished = K.compact ? (int64_t)c : -1;
    }
    if (unfinished >= 0 && (r = finish((uint32_t)unfinished))) return r;
    // slot mode: the last compacted chunks' outputs to their dst_off, in chunk order
    for (uint32_t k = 0; k < 2; k++) {
        const uint32_t s = nchunks >= 2 ? (nchunks - 2 + k) & 1 : k;
        if ((r = scatter(s))) return r;
    }
    HIP_TRY(hipStreamSynchronize(P.d2h));
    P.busy[0] = P.busy[1] = false;
    return PMC_OK;
}

// On an error part of the batch may still be in flight on the three streams, reading and writing the
// caller's buffers: drain them before returning, so the caller may free those buffers at once.
int pinned_batch(pmc_ctx *ctx, Dir dir, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                 uint32_t n, uint8_t *dst, const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len,
                 int32_t *rc, uint32_t max_len, uint32_t chunk) {
    if (!ctx) return PMC_E_ARG;
    HostCall guard(ctx);
    const int r = pinned_batch_run(ctx, dir, src, src_off, src_len, n, dst, dst_off, dst_cap, dst_len, rc, max_len,
                                   chunk);
    if (r && ctx && ctx->pipe.h2d) {
        (void)hipStreamSynchronize(ctx->pipe.h2d);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->pipe.d2h);
        ctx->pipe.busy[0] = ctx->pipe.busy[1] = false;
    }
    return r;
}

// One value through host_batch (ctx null: the default context).  A compress call's capacity must be
// pmc_gzip_bound(in_len) at least.
int single_value(pmc_ctx *ctx, Dir dir, const void *in, size_t in_len, void *out, size_t out_cap, size_t *out_len) {
    *out_len = 0;
    if (!in || in_len == 0) return PMC_INVALID_INPUT;
    if (!ctx) ctx = pmc_default_ctx();
    if (!ctx) return PMC_E_NO_DEVICE;
    if (dir == kCompress && (in_len > 0xffffffffull || out_cap < pmc_gzip_bound(in_len))) return PMC_E_CAPACITY;
    uint64_t so = 0;
    uint32_t sl = (uint32_t)in_len, cap = (uint32_t)std::min<size_t>(out_cap, 0xffffffffull), dl = 0;
    int32_t rc = 0;
    int r = host_batch(ctx, dir, {(const uint8_t *)in, &so, &sl, 1, (uint8_t *)out, &so, &cap, &dl, &rc});
    if (r) return r;
    *out_len = dl;
    return rc;
}

} // namespace

PMC_API int pmc_gzip_compress_batch_host(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                         const uint32_t *src_len, uint32_t n, uint8_t *dst, const uint64_t *dst_off,
                                         const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc) {
    return host_batch(ctx, kCompress, {src, src_off, src_len, n, dst, dst_off, dst_cap, dst_len, rc});
}

PMC_API int pmc_gzip_decompress_batch_host(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                           const uint32_t *src_len, uint32_t n, uint8_t *dst,
                                           const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len,
                                           int32_t *rc) {
    return host_batch(ctx, kDecompress, {src, src_off, src_len, n, dst, dst_off, dst_cap, dst_len, rc});
}

PMC_API int pmc_gzip_compress_batch_pinned(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                           const uint32_t *src_len, uint32_t n, uint8_t *dst,
                                           const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len,
                                           int32_t *rc, uint32_t max_len, uint32_t chunk) {
    return pinned_batch(ctx, kCompress, src, src_off, src_len, n, dst, dst_off, dst_cap, dst_len, rc, max_len,
                        chunk);
}

PMC_API int pmc_gzip_decompress_batch_pinned(pmc_ctx *ctx, const uint8_t *src, const uint64_t *src_off,
                                             const uint32_t *src_len, uint32_t n, uint8_t *dst,
                                             const uint64_t *dst_off, const uint32_t *dst_cap, uint32_t *dst_len,
                                             int32_t *rc, uint32_t max_len, uint32_t chunk) {
    return pinned_batch(ctx, kDecompress, src, src_off, src_len, n, dst, dst_off, dst_cap, dst_len, rc, max_len,
                        chunk);
}

PMC_API int pmc_gzip_compress(pmc_ctx *ctx, const void *in, size_t in_len, void *out, size_t out_cap,
                              size_t *out_len) {
    return single_value(ctx, kCompress, in, in_len, out, out_cap, out_len);
}

PMC_API int pmc_gzip_decompress(pmc_ctx *ctx, const void *in, size_t in_len, void *out, size_t out_cap,
                                size_t *out_len) {
    return single_value(ctx, kDecompress, in, in_len, out, out_cap, out_len);
}

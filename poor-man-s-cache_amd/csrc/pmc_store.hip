// pmc_store.hip -- device-resident compressed value store (include/pmc_codec.h).
//
// The reference keeps every compressed value in host memory: Entry.value holds the gzip member
// that insertEntry got from GzipCompressor::Compress (/root/reference/src/kvs/kvs.cpp:183-187,
// kvs.hpp:38-44), a >= 16 KiB new[] buffer per value (gzip_compressor.cpp:21-33), and every GET
// decompresses it into another new[] buffer (kvs.cpp:233) that the response then copies again
// (protocol.cpp:466-497).  Here the members live in one HBM heap:
//   * a SET batch crosses PCIe once as raw values and is compressed straight into its extents;
//   * a GET batch is decompressed on the device into the packed response image of the batch,
//     which crosses PCIe once into a pinned buffer; the wire framing (custom protocol's 0x1F or a
//     RESP bulk string header/trailer) is written around each value in that buffer, so the value
//     bytes are never copied on the host (f3).
// The heap allocator is host-side: extents of the member's compressed length rounded to 16 B (to 1/8
// of a power of two above 8 KiB), per-size free lists, bump allocation otherwise.  A put compresses
// into gzip_bound slots of its device staging, learns the lengths, allocates, then compacts.
// Everything here that is arithmetic -- the allocator, the staging layouts, the framing, the fallback
// rounds -- is pmc_store_plan.hpp's.  Compiled into the unity TU after pmc_capi.hip and pmc_host.hip (uses pmc_ctx,
// DevBuf, HostBuf, the scan/compact kernels).

#include "pmc_store_plan.hpp"

// A put (compress, on the context's stream) and a get (decompress, on the store's own stream) may
// run at the same time from two threads: each direction has its own lock and staging buffers; the
// allocator has a third lock.  Extents a get reads are never ones a concurrent put writes (a put
// only writes extents it allocates, and callers free extents only after their gets returned).
struct pmc_store {
    pmc_ctx *ctx = nullptr;
    std::mutex put_mu, get_mu, alloc_mu;
    hipStream_t gst = nullptr;  // get / read_members stream
    DevBuf heap;
    StoreHeap alloc;      // which bytes of `heap` are whose (alloc_mu held)
    DevBuf pdev, gdev;    // device side of a put / a get: arrays + value bytes / response image
    HostBuf phost, ghost; // pinned host side of a put / the arrays of a get
    HostBuf hresp;        // pinned response image of the last get (resp[] points here)
    DevBuf rdev;          // get_range: a fallback round's arrays + the whole values it decodes
    HostBuf rhost;        // the arrays' pinned host side
};

namespace {

struct StoreCall {  // one direction's lock + the caller's device restored afterwards
    std::lock_guard<std::mutex> lock;
    int prev = -1;
    StoreCall(pmc_store *s, std::mutex &mu) : lock(mu) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(s->ctx->device);
    }
    ~StoreCall() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// a HIP call's verdict, a failure recorded under the entry point's name
struct HipOk {
    const char *who;
    bool operator()(hipError_t e) const {
        if (e != hipSuccess) set_err(who, e);
        return e == hipSuccess;
    }
};

// compact_kernel over m items (device arrays): len[k] bytes from src + from[k] to dst + to[k] where rc[k] is 0
void launch_compact(hipStream_t st, uint32_t m, const uint8_t *src, const uint64_t *from, const uint32_t *len,
                    const int32_t *rc, const uint64_t *to, uint8_t *dst) {
    hipLaunchKernelGGL(compact_kernel, dim3(std::min<uint32_t>((m + 3) / 4, 8192)), dim3(256), 0, st, src, from, len, rc,
                       to, m, dst);
}

// a decode's verdict for a value of `want` bytes: its rc, and PMC_Z_DATA_ERROR where it decoded to another length
inline int32_t read_verdict(int32_t rc, uint32_t got, uint32_t want) {
    return rc != PMC_OK ? rc : got != want ? PMC_Z_DATA_ERROR : PMC_OK;
}

// The step a put and a ranged set end with.  The members of the call's m values lie in their slots (d_slots +
// doff[k], dlen[k] bytes, verdict rc[k]; lengths and verdicts are on the host).  Every value of rc 0 gets an
// extent by its member's length: at(k) is where the extent is written, raw(k) the value's raw length; a full heap
// makes its rc PMC_Z_MEM_ERROR, which the compact pass skips.  Then the extents' offsets (noff) and the verdicts
// go up -- with up_dlen the lengths too -- and the members are compacted into the heap.  False where that failed:
// the new extents hold nothing, so they are released again and their values' rc becomes PMC_E_NO_DEVICE.
template <class ExtAt, class RawOf>
bool store_commit(pmc_store *s, HipOk ok, hipStream_t st, uint32_t m, const uint8_t *d_slots,
                  const StageArr<uint64_t> &doff, const StageArr<uint32_t> &dlen, const StageArr<int32_t> &rc,
                  const StageArr<uint64_t> &noff, bool up_dlen, ExtAt at, RawOf raw) {
    {
        std::lock_guard<std::mutex> a(s->alloc_mu);
        for (uint32_t k = 0; k < m; k++) {
            noff.h[k] = 0;
            if (rc.h[k] != PMC_OK) continue;
            const uint32_t size = StoreHeap::extent_size(dlen.h[k]);
            uint64_t off = 0;
            if (!s->alloc.alloc(size, &off)) {
                rc.h[k] = PMC_Z_MEM_ERROR;
                continue;
            }
            at(k) = pmc_extent{off, size, dlen.h[k], raw(k), 1};
            noff.h[k] = off;
        }
    }
    bool moved = ok(hipMemcpyAsync(noff.d, noff.h, m * 8ull, hipMemcpyHostToDevice, st)) &&
                 ok(hipMemcpyAsync(rc.d, rc.h, m * 4ull, hipMemcpyHostToDevice, st)) &&
                 (!up_dlen || ok(hipMemcpyAsync(dlen.d, dlen.h, m * 4ull, hipMemcpyHostToDevice, st)));
    if (moved) {
        launch_compact(st, m, d_slots, doff.d, dlen.d, rc.d, noff.d, (uint8_t *)s->heap.p);
        moved = ok(hipGetLastError()) && ok(hipStreamSynchronize(st));
    }
    if (!moved) {
        std::lock_guard<std::mutex> a(s->alloc_mu);
        for (uint32_t k = 0; k < m; k++)
            if (rc.h[k] == PMC_OK) {
                s->alloc.release(at(k));
                rc.h[k] = PMC_E_NO_DEVICE;
            }
    }
    return moved;
}

} // namespace

PMC_API int pmc_store_create(pmc_ctx *ctx, uint64_t heap_bytes, pmc_store **out) {
    if (!out) return PMC_E_ARG;
    *out = nullptr;
    if (!ctx) return PMC_E_ARG;
    if (heap_bytes == 0) heap_bytes = 1ull << 30;
    HIP_TRY(hipSetDevice(ctx->device));
    pmc_store *s = new pmc_store;
    s->ctx = ctx;
    if (int r = s->heap.ensure(heap_bytes)) {
        delete s;
        return r;
    }
    if (hipStreamCreateWithFlags(&s->gst, hipStreamNonBlocking) != hipSuccess) {
        s->heap.release();
        delete s;
        return PMC_E_NO_DEVICE;
    }
    s->alloc.heap_bytes = heap_bytes;
    *out = s;
    return PMC_OK;
}

PMC_API void pmc_store_destroy(pmc_store *s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> g(s->get_mu);
        StoreCall call(s, s->put_mu);
        (void)hipStreamSynchronize(s->ctx->stream);
        (void)hipStreamSynchronize(s->gst);
        s->heap.release();
        s->pdev.release();
        s->gdev.release();
        s->phost.release();
        s->ghost.release();
        s->hresp.release();
        s->rdev.release();
        s->rhost.release();
        (void)hipStreamDestroy(s->gst);
    }
    delete s;
}

PMC_API int pmc_store_put_batch(pmc_store *s, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                                uint32_t n, pmc_extent *ext, int32_t *rc) {
    if (!s || (n && (!src || !src_off || !src_len || !ext || !rc))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    StoreCall call(s, s->put_mu);
    pmc_ctx *ctx = s->ctx;
    // values sent to the codec: the non-empty ones.  They are compressed into gzip_bound slots of the
    // put's device staging first; extents are allocated only once the compressed lengths are known,
    // so the heap holds ~C bytes per value, not the uncompressed bound (kvs.hpp:38-44 keeps C bytes).
    std::vector<uint32_t> pick;
    pick.reserve(n);
    uint64_t bytes = 0, slots = 0, max_len = 1;
    for (uint32_t i = 0; i < n; i++) {
        ext[i] = pmc_extent{0, 0, 0, 0, 0};
        if (src_len[i] == 0) {
            rc[i] = PMC_INVALID_INPUT;
            continue;
        }
        rc[i] = PMC_OK;
        pick.push_back(i);
        bytes += src_len[i];
        slots += round16(gzip_bound(src_len[i]));
        max_len = std::max<uint64_t>(max_len, src_len[i]);
    }
    const uint32_t m = (uint32_t)pick.size();
    if (m == 0) return PMC_OK;
    auto fail_all = [&](int code) {  // nothing was allocated yet
        for (uint32_t k = 0; k < m; k++) rc[pick[k]] = code;
        return code;
    };
    // staging: PutStage's arrays | value bytes | member slots (device only)
    const uint64_t meta = PutStage(m).meta, vb = al256(bytes + 16);
    int r = s->phost.ensure(meta + vb);
    if (!r) r = s->pdev.ensure(meta + vb + slots + 64);
    if (r) return fail_all(r);
    uint8_t *hp = (uint8_t *)s->phost.p, *dp = (uint8_t *)s->pdev.p;
    const PutStage L(m, hp, dp);
    uint8_t *h_src = hp + meta, *d_slots = dp + meta + vb;
    uint64_t so = 0, doff = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        L.soff.h[k] = so;
        L.slen.h[k] = src_len[i];
        memcpy(h_src + so, src + src_off[i], src_len[i]);
        so += src_len[i];
        L.doff.h[k] = doff;
        L.dcap.h[k] = (uint32_t)gzip_bound(src_len[i]);
        doff += round16(gzip_bound(src_len[i]));
    }
    hipStream_t st = ctx->stream;
    const HipOk ok{"pmc_store_put_batch"};
    // 1. values in, members into the staging slots, lengths back
    if (!ok(hipMemcpyAsync(dp, hp, meta + bytes, hipMemcpyHostToDevice, st))) return fail_all(PMC_E_NO_DEVICE);
    r = pmc_gzip_compress_batch(ctx, dp + meta, L.soff.d, L.slen.d, m, d_slots, L.doff.d, L.dcap.d, L.dlen.d, L.rc.d,
                                (uint32_t)max_len, st);
    if (r) return fail_all(r);
    if (!ok(hipMemcpyAsync(L.dlen_rc.h, L.dlen_rc.d, L.dlen_rc.bytes, hipMemcpyDeviceToHost, st)) ||
        !ok(hipStreamSynchronize(st)))
        return fail_all(PMC_E_NO_DEVICE);
    // 2. extents by compressed length, the members from the slots into them.  A failed compact fails every
    // value sent to the codec, those whose compress had failed too.
    const bool moved = store_commit(
        s, ok, st, m, d_slots, L.doff, L.dlen, L.rc, L.poff, false, [&](uint32_t k) -> pmc_extent & { return ext[pick[k]]; },
        [&](uint32_t k) { return src_len[pick[k]]; });
    for (uint32_t k = 0; k < m; k++) rc[pick[k]] = moved ? L.rc.h[k] : PMC_E_NO_DEVICE;
    return moved ? PMC_OK : PMC_E_NO_DEVICE;
}

// frame_of(i): extent i's PMC_FRAME_* (checked by the callers)
template <class FrameOf>
static int store_get(pmc_store *s, const pmc_extent *ext, uint32_t n, FrameOf frame_of, const uint8_t **resp,
                     uint32_t *resp_len, int32_t *rc) {
    if (n == 0) return PMC_OK;
    StoreCall call(s, s->get_mu);
    pmc_ctx *ctx = s->ctx;
    std::vector<uint32_t> pick;
    std::vector<uint64_t> pos(n, 0);
    std::vector<uint8_t> hlen(n, 0);
    uint64_t total = 0, max_raw = 1;
    for (uint32_t i = 0; i < n; i++) {
        const int frame = frame_of(i);
        resp[i] = nullptr;
        resp_len[i] = 0;
        if (!(ext[i].flags & 1) || ext[i].len == 0) {
            rc[i] = PMC_E_ARG;
            continue;
        }
        hlen[i] = (uint8_t)frame_head(frame, ext[i].raw_len);
        pos[i] = total;
        total += hlen[i] + (uint64_t)ext[i].raw_len + frame_tail(frame);
        max_raw = std::max<uint64_t>(max_raw, ext[i].raw_len);
        rc[i] = PMC_OK;
        pick.push_back(i);
    }
    const uint32_t m = (uint32_t)pick.size();
    if (m == 0) return PMC_OK;
    // device staging: GetStage's arrays | response image
    const uint64_t meta = GetStage(m).meta;
    int r = s->ghost.ensure(meta);
    if (!r) r = s->gdev.ensure(meta + total + 64);
    if (!r) r = s->hresp.ensure(total + 64);
    if (r) return r;
    uint8_t *hp = (uint8_t *)s->ghost.p, *dp = (uint8_t *)s->gdev.p;
    const GetStage L(m, hp, dp);
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        L.soff.h[k] = ext[i].off;
        L.slen.h[k] = ext[i].len;
        L.doff.h[k] = pos[i] + hlen[i];
        L.dcap.h[k] = ext[i].raw_len;
    }
    hipStream_t st = s->gst;
    uint8_t *d_img = dp + meta, *img = (uint8_t *)s->hresp.p;
    HIP_TRY(hipMemcpyAsync(dp, hp, meta, hipMemcpyHostToDevice, st));
    r = pmc_gzip_decompress_batch(ctx, (const uint8_t *)s->heap.p, L.soff.d, L.slen.d, m, d_img, L.doff.d, L.dcap.d,
                                  L.dlen.d, L.rc.d, (uint32_t)max_raw, st);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(L.dlen_rc.h, L.dlen_rc.d, L.dlen_rc.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(img, d_img, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        if ((rc[i] = read_verdict(L.rc.h[k], L.dlen.h[k], ext[i].raw_len)) != PMC_OK) continue;
        const int frame = frame_of(i);
        frame_write(img + pos[i], frame, ext[i].raw_len);
        resp[i] = img + pos[i];
        resp_len[i] = hlen[i] + ext[i].raw_len + frame_tail(frame);
    }
    return PMC_OK;
}

PMC_API int pmc_store_get_batch(pmc_store *s, const pmc_extent *ext, uint32_t n, int frame, const uint8_t **resp,
                                uint32_t *resp_len, int32_t *rc) {
    if (!s || (n && (!ext || !resp || !resp_len || !rc)) || frame < PMC_FRAME_RAW || frame > PMC_FRAME_RESP)
        return PMC_E_ARG;
    return store_get(s, ext, n, [frame](uint32_t) { return frame; }, resp, resp_len, rc);
}

PMC_API int pmc_store_get_batch_frames(pmc_store *s, const pmc_extent *ext, uint32_t n, const uint8_t *frames,
                                       const uint8_t **resp, uint32_t *resp_len, int32_t *rc) {
    if (!s || (n && (!ext || !frames || !resp || !resp_len || !rc))) return PMC_E_ARG;
    for (uint32_t i = 0; i < n; i++)
        if (frames[i] > PMC_FRAME_RESP) return PMC_E_ARG;
    return store_get(s, ext, n, [frames](uint32_t i) { return (int)frames[i]; }, resp, resp_len, rc);
}

// Ranged get (include/pmc_codec.h pmc_store_get_range_batch): the ranged call over the heap for the extents
// that may carry an index, then whole reads, in rounds of bounded scratch, of those it declined and of the
// small ones; one D2H of the response image.
PMC_API int pmc_store_get_range_batch(pmc_store *s, const pmc_extent *ext, const uint32_t *range_off,
                                      const uint32_t *range_len, uint32_t n, int frame, const uint8_t **resp,
                                      uint32_t *resp_len, int32_t *rc) {
    if (!s || (n && (!ext || !range_off || !range_len || !resp || !resp_len || !rc)) || frame < PMC_FRAME_RAW ||
        frame > PMC_FRAME_RESP)
        return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    StoreCall call(s, s->get_mu);
    pmc_ctx *ctx = s->ctx;
    // live extents: their clamped ranges and their places in the response image
    std::vector<uint32_t> live, ranged, whole;
    std::vector<uint64_t> pos(n, 0);
    std::vector<uint32_t> ro(n, 0), rl(n, 0);
    std::vector<uint8_t> hlen(n, 0);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        resp[i] = nullptr;
        resp_len[i] = 0;
        if (!(ext[i].flags & 1) || ext[i].len == 0) {
            rc[i] = PMC_E_ARG;
            continue;
        }
        const RangeOf r = range_of(ext[i].raw_len, kRangeLog2Max, range_off[i], range_len[i]);
        ro[i] = r.o;
        rl[i] = r.L;
        hlen[i] = (uint8_t)frame_head(frame, r.L);
        pos[i] = total;
        total += hlen[i] + (uint64_t)r.L + frame_tail(frame);
        rc[i] = PMC_OK;
        live.push_back(i);
        // (an empty range needs no device work; a value of <= 4096 bytes cannot carry an index)
        if (r.L) (ext[i].raw_len > (1u << kIdxLog2Min) ? ranged : whole).push_back(i);
    }
    if (live.empty()) return PMC_OK;
    // device staging: RangeGetStage's arrays | response image
    const uint32_t m = (uint32_t)ranged.size();
    const uint64_t meta = RangeGetStage(m).meta;
    int r = s->ghost.ensure(meta + 64);
    if (!r) r = s->gdev.ensure(meta + total + 64);
    if (!r) r = s->hresp.ensure(total + 64);
    if (r) return r;
    hipStream_t st = s->gst;
    uint8_t *d_img = (uint8_t *)s->gdev.p + meta, *img = (uint8_t *)s->hresp.p;
    if (m) {
        uint8_t *hp = (uint8_t *)s->ghost.p, *dp = (uint8_t *)s->gdev.p;
        const RangeGetStage L(m, hp, dp);
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = ranged[k];
            L.soff.h[k] = ext[i].off;
            L.slen.h[k] = ext[i].len;
            L.roff.h[k] = ro[i];
            L.rlen.h[k] = rl[i];
            L.doff.h[k] = pos[i] + hlen[i];
            L.dcap.h[k] = rl[i];
        }
        HIP_TRY(hipMemcpyAsync(dp, hp, meta, hipMemcpyHostToDevice, st));
        r = pmc_gzip_decompress_range_batch(ctx, (const uint8_t *)s->heap.p, L.soff.d, L.slen.d, L.roff.d, L.rlen.d, m,
                                            d_img, L.doff.d, L.dcap.d, L.dlen.d, L.rc.d, st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(L.dlen_rc.h, L.dlen_rc.d, L.dlen_rc.bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = ranged[k];
            if (L.rc.h[k] == PMC_E_NO_INDEX) whole.push_back(i);
            else rc[i] = read_verdict(L.rc.h[k], L.dlen.h[k], rl[i]);
        }
    }
    // the whole reads, in rounds over `whole`: the small extents in batch order, then the declined ones
    std::vector<uint32_t> raw(whole.size());
    for (size_t w = 0; w < whole.size(); w++) raw[w] = ext[whole[w]].raw_len;
    for (size_t w0 = 0; w0 < whole.size();) {
        const FallbackRound R = cut_round(raw.data(), raw.size(), w0, kRangeFallbackBudget);
        const uint32_t q = (uint32_t)(R.end - w0);
        // round staging: RangeGetRound's arrays | values
        const uint64_t rmeta = RangeGetRound(q).meta;
        r = s->rhost.ensure(rmeta);
        if (!r) r = s->rdev.ensure(rmeta + R.bytes + 64);
        if (r) return r;
        uint8_t *hp = (uint8_t *)s->rhost.p, *dp = (uint8_t *)s->rdev.p;
        const RangeGetRound L(q, hp, dp);
        uint64_t at = 0;
        for (uint32_t k = 0; k < q; k++) {
            const uint32_t i = whole[w0 + k];
            L.soff.h[k] = ext[i].off;
            L.slen.h[k] = ext[i].len;
            L.doff.h[k] = at;
            L.dcap.h[k] = ext[i].raw_len;
            L.cut.h[k] = at + ro[i];
            L.clen.h[k] = rl[i];
            L.poff.h[k] = pos[i] + hlen[i];
            at += round16(ext[i].raw_len);
        }
        uint8_t *d_vals = dp + rmeta;
        HIP_TRY(hipMemcpyAsync(dp, hp, rmeta, hipMemcpyHostToDevice, st));
        r = pmc_gzip_decompress_batch(ctx, (const uint8_t *)s->heap.p, L.soff.d, L.slen.d, q, d_vals, L.doff.d, L.dcap.d,
                                      L.dlen.d, L.rc.d, (uint32_t)R.max_raw, st);
        if (r) return r;
        // the slices of the values that decoded (rc 0) into their places in the image
        launch_compact(st, q, d_vals, L.cut.d, L.clen.d, L.rc.d, L.poff.d, d_img);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(L.dlen_rc.h, L.dlen_rc.d, L.dlen_rc.bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < q; k++) {
            const uint32_t i = whole[w0 + k];
            rc[i] = read_verdict(L.rc.h[k], L.dlen.h[k], ext[i].raw_len);
        }
        w0 = R.end;
    }
    if (total) {
        HIP_TRY(hipMemcpyAsync(img, d_img, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (uint32_t i : live) {
        if (rc[i] != PMC_OK) continue;
        frame_write(img + pos[i], frame, rl[i]);
        resp[i] = img + pos[i];
        resp_len[i] = hlen[i] + rl[i] + frame_tail(frame);
    }
    return PMC_OK;
}

// Ranged set (include/pmc_codec.h pmc_store_set_range_batch) and, with `grow`, growing set
// (pmc_store_grow_range_batch): the rewrite or the grow call over the heap for the extents that may carry an index;
// whole read into a value of the new length, overlay and compress, in rounds of bounded scratch, for those it
// declined and the small ones; then new extents by member length, the members compacted in, and the old extents
// released.  nraw: a value's length after the write (grown_len; without `grow` what it was).
static int store_write_range(pmc_store *s, bool grow, const char *who, pmc_extent *ext, const uint8_t *src,
                             const uint64_t *src_off, const uint32_t *src_len, const uint32_t *range_off, uint32_t n,
                             int32_t *rc) {
    std::lock_guard<std::mutex> get_lock(s->get_mu);
    StoreCall call(s, s->put_mu);
    pmc_ctx *ctx = s->ctx;
    // live, in-bounds, distinct extents; an empty patch changes nothing
    std::unordered_map<uint64_t, uint32_t> seen;
    std::vector<uint32_t> nraw(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const bool live = (ext[i].flags & 1) && ext[i].len;
        const uint64_t end = (uint64_t)range_off[i] + src_len[i];
        const uint64_t after = src_len[i] ? grown_len(ext[i].raw_len, range_off[i], src_len[i]) : ext[i].raw_len;
        const bool fits = grow ? src_len[i] == 0 || after <= kStoreGrowMax : end <= ext[i].raw_len;
        rc[i] = live && fits ? PMC_OK : PMC_E_ARG;
        nraw[i] = (uint32_t)after; // (<= 2^32 - 1 where fits)
        if (live) seen[ext[i].off]++;
    }
    std::vector<uint32_t> pick, full; // pick: chunk-path requests first, then the small ones
    for (uint32_t i = 0; i < n; i++) {
        if ((ext[i].flags & 1) && ext[i].len && seen[ext[i].off] > 1) rc[i] = PMC_E_ARG;
        if (rc[i] == PMC_OK && src_len[i] && ext[i].raw_len > kIdxChunk) pick.push_back(i);
    }
    const uint32_t mc = (uint32_t)pick.size();
    for (uint32_t i = 0; i < n; i++)
        if (rc[i] == PMC_OK && src_len[i] && ext[i].raw_len <= kIdxChunk) pick.push_back(i);
    const uint32_t m = (uint32_t)pick.size();
    if (m == 0) return PMC_OK;
    auto fail_all = [&](int code) { // nothing was allocated or released yet
        for (uint32_t k = 0; k < m; k++) rc[pick[k]] = code;
        return code;
    };
    // put staging: RangeSetStage's arrays | patches | member slots (device only)
    const uint64_t meta = RangeSetStage(m).meta;
    uint64_t pbytes = 0, slots = 0;
    for (uint32_t k = 0; k < m; k++) {
        pbytes += src_len[pick[k]];
        slots += round16(gzip_bound(nraw[pick[k]]));
    }
    const uint64_t pb = al256(pbytes + 16);
    int r = s->phost.ensure(meta + pb);
    if (!r) r = s->pdev.ensure(meta + pb + slots + 64);
    if (r) return fail_all(r);
    uint8_t *hp = (uint8_t *)s->phost.p, *dp = (uint8_t *)s->pdev.p;
    const RangeSetStage L(m, hp, dp);
    uint8_t *h_patch = hp + meta, *d_patch = dp + meta, *d_slots = dp + meta + pb;
    uint64_t po = 0, doff = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        L.soff.h[k] = ext[i].off;
        L.slen.h[k] = ext[i].len;
        L.poff.h[k] = po;
        L.plen.h[k] = src_len[i];
        L.roff.h[k] = range_off[i];
        memcpy(h_patch + po, src + src_off[i], src_len[i]);
        po += src_len[i];
        L.doff.h[k] = doff;
        L.dcap.h[k] = (uint32_t)gzip_bound(nraw[i]);
        doff += round16(gzip_bound(nraw[i]));
        L.dlen.h[k] = 0;
        L.rc.h[k] = k < mc ? PMC_OK : PMC_E_NO_INDEX; // (the small ones take the full path)
    }
    hipStream_t st = ctx->stream;
    const HipOk ok{who};
    if (!ok(hipMemcpyAsync(dp, hp, meta + pbytes, hipMemcpyHostToDevice, st))) return fail_all(PMC_E_NO_DEVICE);
    // 1. the chunk path
    if (mc) {
        r = (grow ? pmc_gzip_grow_range_batch : pmc_gzip_rewrite_range_batch)(
            ctx, (const uint8_t *)s->heap.p, L.soff.d, L.slen.d, d_patch, L.poff.d, L.plen.d, L.roff.d, mc, d_slots,
            L.doff.d, L.dcap.d, L.dlen.d, L.rc.d, st);
        if (r) return fail_all(r);
        if (!ok(hipMemcpyAsync(L.dlen.h, L.dlen.d, mc * 4ull, hipMemcpyDeviceToHost, st)) ||
            !ok(hipMemcpyAsync(L.rc.h, L.rc.d, mc * 4ull, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st)))
            return fail_all(PMC_E_NO_DEVICE);
    }
    std::vector<uint32_t> raw;
    for (uint32_t k = 0; k < m; k++)
        if (L.rc.h[k] == PMC_E_NO_INDEX) {
            full.push_back(k);
            raw.push_back(nraw[pick[k]]);
        }
    // 2. the full path, in rounds over `full`
    for (size_t w0 = 0; w0 < full.size();) {
        const FallbackRound R = cut_round(raw.data(), raw.size(), w0, kRangeFallbackBudget);
        const uint32_t q = (uint32_t)(R.end - w0);
        // round staging: RangeWriteRound's arrays | values of the new lengths
        const uint64_t rmeta = RangeWriteRound(q).meta;
        r = s->rhost.ensure(rmeta);
        if (!r) r = s->rdev.ensure(rmeta + R.bytes + 64);
        if (r) return fail_all(r);
        uint8_t *rh = (uint8_t *)s->rhost.p, *rd = (uint8_t *)s->rdev.p;
        const RangeWriteRound G(q, rh, rd);
        uint64_t at = 0;
        for (uint32_t j = 0; j < q; j++) {
            const uint32_t k = full[w0 + j], i = pick[k];
            G.soff.h[j] = ext[i].off;
            G.slen.h[j] = ext[i].len;
            G.voff.h[j] = at;
            G.vcap.h[j] = ext[i].raw_len;
            G.nlen.h[j] = nraw[i];
            G.cut.h[j] = at + range_off[i];
            G.poff.h[j] = L.poff.h[k];
            G.plen.h[j] = src_len[i];
            G.doff.h[j] = L.doff.h[k];
            G.dcap.h[j] = L.dcap.h[k];
            at += round16(nraw[i]);
        }
        uint8_t *d_vals = rd + rmeta;
        if (!ok(hipMemcpyAsync(rd, rh, rmeta, hipMemcpyHostToDevice, st))) return fail_all(PMC_E_NO_DEVICE);
        // (a growing set: the bytes between a value's old end and its patch are zero)
        if (grow && !ok(hipMemsetAsync(d_vals, 0, R.bytes, st))) return fail_all(PMC_E_NO_DEVICE);
        r = pmc_gzip_decompress_batch(ctx, (const uint8_t *)s->heap.p, G.soff.d, G.slen.d, q, d_vals, G.voff.d, G.vcap.d,
                                      G.vlen.d, G.vrc.d, (uint32_t)R.max_raw, st);
        if (r) return fail_all(r);
        // the patches over the values that decoded (rc 0), then the values compressed into their slots
        launch_compact(st, q, d_patch, G.poff.d, G.plen.d, G.vrc.d, G.cut.d, d_vals);
        if (!ok(hipGetLastError())) return fail_all(PMC_E_NO_DEVICE);
        r = pmc_gzip_compress_batch(ctx, d_vals, G.voff.d, G.nlen.d, q, d_slots, G.doff.d, G.dcap.d, G.dlen.d, G.rc.d,
                                    (uint32_t)R.max_raw, st);
        if (r) return fail_all(r);
        if (!ok(hipMemcpyAsync(G.vlen_vrc.h, G.vlen_vrc.d, G.vlen_vrc.bytes, hipMemcpyDeviceToHost, st)) ||
            !ok(hipMemcpyAsync(G.dlen_rc.h, G.dlen_rc.d, G.dlen_rc.bytes, hipMemcpyDeviceToHost, st)) ||
            !ok(hipStreamSynchronize(st)))
            return fail_all(PMC_E_NO_DEVICE);
        for (uint32_t j = 0; j < q; j++) {
            const uint32_t k = full[w0 + j], i = pick[k];
            const int32_t v = read_verdict(G.vrc.h[j], G.vlen.h[j], ext[i].raw_len);
            L.rc.h[k] = v != PMC_OK ? v : G.rc.h[j];
            L.dlen.h[k] = G.dlen.h[j];
        }
        w0 = R.end;
    }
    // 3. new extents by member length, the members from the slots into them; only then are the old ones released
    // (a value that got no new extent, or whose new extent was lost to a failed compact, keeps its old one)
    std::vector<pmc_extent> fresh(m, pmc_extent{0, 0, 0, 0, 0});
    const bool moved = store_commit(
        s, ok, st, m, d_slots, L.doff, L.dlen, L.rc, L.noff, true, [&](uint32_t k) -> pmc_extent & { return fresh[k]; },
        [&](uint32_t k) { return nraw[pick[k]]; });
    std::lock_guard<std::mutex> a(s->alloc_mu);
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        if (L.rc.h[k] != PMC_OK) {
            rc[i] = L.rc.h[k];
            continue;
        }
        s->alloc.release(ext[i]);
        ext[i] = fresh[k];
    }
    return moved ? PMC_OK : PMC_E_NO_DEVICE;
}

PMC_API int pmc_store_set_range_batch(pmc_store *s, pmc_extent *ext, const uint8_t *src, const uint64_t *src_off,
                                      const uint32_t *src_len, const uint32_t *range_off, uint32_t n, int32_t *rc) {
    if (!s || (n && (!ext || !src || !src_off || !src_len || !range_off || !rc))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    return store_write_range(s, false, "pmc_store_set_range_batch", ext, src, src_off, src_len, range_off, n, rc);
}

PMC_API int pmc_store_grow_range_batch(pmc_store *s, pmc_extent *ext, const uint8_t *src, const uint64_t *src_off,
                                       const uint32_t *src_len, const uint32_t *range_off, uint32_t n, int32_t *rc) {
    if (!s || (n && (!ext || !src || !src_off || !src_len || !range_off || !rc))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    return store_write_range(s, true, "pmc_store_grow_range_batch", ext, src, src_off, src_len, range_off, n, rc);
}

PMC_API int pmc_store_append_batch(pmc_store *s, pmc_extent *ext, const uint8_t *src, const uint64_t *src_off,
                                   const uint32_t *src_len, uint32_t n, int32_t *rc) {
    if (!s || (n && (!ext || !src || !src_off || !src_len || !rc))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    std::vector<uint32_t> at(n);
    for (uint32_t i = 0; i < n; i++) at[i] = ext[i].raw_len;
    return store_write_range(s, true, "pmc_store_append_batch", ext, src, src_off, src_len, at.data(), n, rc);
}

PMC_API int pmc_store_read_members(pmc_store *s, const pmc_extent *ext, uint32_t n, uint8_t *dst,
                                   const uint64_t *dst_off) {
    if (!s || (n && (!ext || !dst || !dst_off))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    StoreCall call(s, s->get_mu);
    for (uint32_t i = 0; i < n; i++)
        if (!(ext[i].flags & 1)) return PMC_E_ARG;
    // gather the members on the device (compact_kernel), then one D2H.  staging: MembersStage's arrays | members
    const uint64_t meta = MembersStage(n).meta;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += ext[i].len;
    int r = s->ghost.ensure(meta + total + 64);
    if (!r) r = s->gdev.ensure(meta + total + 64);
    if (r) return r;
    uint8_t *hp = (uint8_t *)s->ghost.p, *dp = (uint8_t *)s->gdev.p;
    const MembersStage L(n, hp, dp);
    uint64_t p = 0;
    for (uint32_t i = 0; i < n; i++) {
        L.soff.h[i] = ext[i].off;
        L.poff.h[i] = p;
        L.len.h[i] = ext[i].len;
        L.rc.h[i] = 0;
        p += ext[i].len;
    }
    hipStream_t st = s->gst;
    HIP_TRY(hipMemcpyAsync(dp, hp, meta, hipMemcpyHostToDevice, st));
    launch_compact(st, n, (const uint8_t *)s->heap.p, L.soff.d, L.len.d, L.rc.d, L.poff.d, dp + meta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hp + meta, dp + meta, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; i++) memcpy(dst + dst_off[i], hp + meta + L.poff.h[i], ext[i].len);
    return PMC_OK;
}

PMC_API int pmc_store_free(pmc_store *s, pmc_extent *ext, uint32_t n) {
    if (!s || (n && !ext)) return PMC_E_ARG;
    std::lock_guard<std::mutex> lock(s->alloc_mu);
    for (uint32_t i = 0; i < n; i++) s->alloc.release(ext[i]);
    return PMC_OK;
}

PMC_API uint8_t *pmc_store_data(pmc_store *s) { return s ? (uint8_t *)s->heap.p : nullptr; }

PMC_API int pmc_store_stats(pmc_store *s, uint64_t *used, uint64_t *reserved, uint64_t *heap) {
    if (!s) return PMC_E_ARG;
    std::lock_guard<std::mutex> lock(s->alloc_mu);
    if (used) *used = s->alloc.used;
    if (reserved) *reserved = s->alloc.bump;
    if (heap) *heap = s->alloc.heap_bytes;
    return PMC_OK;
}

// ---- fixed-slot device slab (include/pmc_codec.h pmc_slab_*) ------------------------------------
// The device-resident form of the store for callers whose keys, values and bookkeeping already live
// on the device (bench.py --mix, BASELINE configs[2]): slot s holds at most one gzip member at
// data + s * stride (stride = gzip_bound(max_value_len) rounded to 16 B) and its length in lens[s]
// (0 = empty).  set / get are enqueue-only batch calls on the caller's stream; the slot layouts are
// built on the device, so a batch never waits for the host.
struct pmc_slab {
    pmc_ctx *ctx = nullptr;
    uint32_t slots = 0, max_len = 0, cap = 0;
    uint64_t stride = 0;
    DevBuf data, lens;
    DevBuf set_scratch, get_scratch; // per direction: offsets / caps / lengths of a batch
};

namespace {
__global__ void slab_set_layout_kernel(const uint32_t *slot, uint32_t n, uint64_t stride, uint32_t cap, uint64_t *doff,
                                       uint32_t *dcap) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        doff[i] = (uint64_t)slot[i] * stride;
        dcap[i] = cap;
    }
}
__global__ void slab_commit_kernel(const uint32_t *slot, uint32_t n, const uint32_t *dlen, const int32_t *rc,
                                   uint32_t *lens) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        lens[slot[i]] = rc[i] == 0 ? dlen[i] : 0u;
}
__global__ void slab_get_layout_kernel(const uint32_t *slot, uint32_t n, uint64_t stride, const uint32_t *lens,
                                       uint64_t *soff, uint32_t *slen) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        soff[i] = (uint64_t)slot[i] * stride;
        slen[i] = lens[slot[i]];
    }
}
inline dim3 slab_grid(uint32_t n) { return dim3((unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 4096)); }
} // namespace

PMC_API int pmc_slab_create(pmc_ctx *ctx, uint32_t slots, uint32_t max_value_len, pmc_slab **out) {
    if (!out) return PMC_E_ARG;
    *out = nullptr;
    if (!ctx || !slots || !max_value_len) return PMC_E_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    pmc_slab *s = new pmc_slab;
    s->ctx = ctx;
    s->slots = slots;
    s->max_len = max_value_len;
    s->cap = (uint32_t)gzip_bound(max_value_len);
    s->stride = ((uint64_t)s->cap + 15) & ~(uint64_t)15;
    int r = s->data.ensure(s->stride * slots + 16);
    if (!r) r = s->lens.ensure((uint64_t)slots * 4);
    if (!r && hipMemset(s->lens.p, 0, (uint64_t)slots * 4) != hipSuccess) r = PMC_E_NO_DEVICE;
    if (r) {
        s->data.release();
        s->lens.release();
        delete s;
        return r;
    }
    *out = s;
    return PMC_OK;
}

PMC_API void pmc_slab_destroy(pmc_slab *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipDeviceSynchronize();
    s->data.release();
    s->lens.release();
    s->set_scratch.release();
    s->get_scratch.release();
    delete s;
}

PMC_API uint8_t *pmc_slab_data(pmc_slab *s) { return s ? (uint8_t *)s->data.p : nullptr; }
PMC_API uint32_t *pmc_slab_lengths(pmc_slab *s) { return s ? (uint32_t *)s->lens.p : nullptr; }
PMC_API uint64_t pmc_slab_stride(pmc_slab *s) { return s ? s->stride : 0; }

PMC_API int pmc_slab_set(pmc_slab *s, const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                         const uint32_t *slot, uint32_t n, int32_t *rc, void *stream) {
    if (!s || (n && (!src || !src_off || !src_len || !slot || !rc))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    pmc_ctx *ctx = s->ctx;
    hipStream_t st = (hipStream_t)stream;
    // the set scratch follows the compress direction's ordering (dir_enter / dir_leave)
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[0]);
    int r = dir_enter(ctx, 0, st);
    if (r) return r;
    const uint64_t a8 = ((uint64_t)n * 8 + 255) & ~(uint64_t)255, a4 = ((uint64_t)n * 4 + 255) & ~(uint64_t)255;
    if ((r = s->set_scratch.ensure(a8 + 2 * a4))) return r;
    uint64_t *doff = (uint64_t *)s->set_scratch.p;
    uint32_t *dcap = (uint32_t *)((uint8_t *)doff + a8), *dlen = (uint32_t *)((uint8_t *)dcap + a4);
    hipLaunchKernelGGL(slab_set_layout_kernel, slab_grid(n), dim3(256), 0, st, slot, n, s->stride, s->cap, doff, dcap);
    HIP_TRY(hipGetLastError());
    r = pmc_gzip_compress_batch(ctx, src, src_off, src_len, n, (uint8_t *)s->data.p, doff, dcap, dlen, rc, s->max_len,
                                stream);
    if (r) return r;
    hipLaunchKernelGGL(slab_commit_kernel, slab_grid(n), dim3(256), 0, st, slot, n, (const uint32_t *)dlen,
                       (const int32_t *)rc, (uint32_t *)s->lens.p);
    HIP_TRY(hipGetLastError());
    return dir_leave(ctx, 0, st);
}

PMC_API int pmc_slab_get(pmc_slab *s, const uint32_t *slot, uint32_t n, uint8_t *dst, const uint64_t *dst_off,
                         const uint32_t *dst_cap, uint32_t *dst_len, int32_t *rc, void *stream) {
    if (!s || (n && (!slot || !dst || !dst_off || !dst_cap || !dst_len || !rc))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    pmc_ctx *ctx = s->ctx;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::recursive_mutex> dir_lock(ctx->dir_mu[1]);
    int r = dir_enter(ctx, 1, st);
    if (r) return r;
    const uint64_t a8 = ((uint64_t)n * 8 + 255) & ~(uint64_t)255;
    if ((r = s->get_scratch.ensure(a8 + (uint64_t)n * 4 + 256))) return r;
    uint64_t *soff = (uint64_t *)s->get_scratch.p;
    uint32_t *slen = (uint32_t *)((uint8_t *)soff + a8);
    hipLaunchKernelGGL(slab_get_layout_kernel, slab_grid(n), dim3(256), 0, st, slot, n, s->stride,
                       (const uint32_t *)s->lens.p, soff, slen);
    HIP_TRY(hipGetLastError());
    r = pmc_gzip_decompress_batch(ctx, (const uint8_t *)s->data.p, soff, slen, n, dst, dst_off, dst_cap, dst_len, rc,
                                  s->max_len, stream);
    if (r) return r;
    return dir_leave(ctx, 1, st);
}

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
// into gzip_bound slots of its device staging, learns the lengths, allocates, then compacts.  Compiled into the unity TU after
// pmc_capi.hip (uses pmc_ctx, DevBuf, HostBuf, the scan/compact kernels).

#include <unordered_map>

// A put (compress, on the context's stream) and a get (decompress, on the store's own stream) may
// run at the same time from two threads: each direction has its own lock and staging buffers; the
// allocator has a third lock.  Extents a get reads are never ones a concurrent put writes (a put
// only writes extents it allocates, and callers free extents only after their gets returned).
struct pmc_store {
    pmc_ctx *ctx = nullptr;
    std::mutex put_mu, get_mu, alloc_mu;
    hipStream_t gst = nullptr;  // get / read_members stream
    DevBuf heap;
    uint64_t heap_bytes = 0, bump = 0, used = 0;
    std::unordered_map<uint32_t, std::vector<uint64_t>> free_lists;  // extent size -> offsets
    DevBuf pdev, gdev;    // device side of a put / a get: arrays + value bytes / response image
    HostBuf phost, ghost; // pinned host side of a put / the arrays of a get
    HostBuf hresp;        // pinned response image of the last get (resp[] points here)
    DevBuf rdev;          // get_range: a fallback round's arrays + the whole values it decodes
    HostBuf rhost;        // the arrays' pinned host side
};

namespace {

// bytes reserved for a member of `len` bytes: 16-byte granules, and above 8 KiB steps of 1/8 of
// the power of two below (bounded waste, few distinct free-list sizes)
uint32_t extent_size(uint64_t len) {
    uint64_t c = (len + 15) & ~(uint64_t)15;
    if (c > 8192) {
        uint64_t p = 1;
        while (p * 2 <= c) p *= 2;
        const uint64_t step = p / 8;
        c = (c + step - 1) / step * step;
    }
    return (uint32_t)c;
}

bool store_alloc(pmc_store *s, uint32_t size, uint64_t *off) {  // alloc_mu held
    auto it = s->free_lists.find(size);
    if (it != s->free_lists.end() && !it->second.empty()) {
        *off = it->second.back();
        it->second.pop_back();
    } else {
        if (s->bump + size > s->heap_bytes) return false;
        *off = s->bump;
        s->bump += size;
    }
    s->used += size;
    return true;
}

void store_release(pmc_store *s, pmc_extent &e) {  // alloc_mu held
    if (!(e.flags & 1)) return;
    s->free_lists[e.cap].push_back(e.off);
    s->used -= e.cap;
    e.flags = 0;
}

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

inline uint64_t al256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

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
    s->heap_bytes = heap_bytes;
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
        slots += (gzip_bound(src_len[i]) + 15) & ~(uint64_t)15;
        max_len = std::max<uint64_t>(max_len, src_len[i]);
    }
    const uint32_t m = (uint32_t)pick.size();
    if (m == 0) return PMC_OK;
    auto fail_all = [&](int code) {  // nothing was allocated yet
        for (uint32_t k = 0; k < m; k++) rc[pick[k]] = code;
        return code;
    };
    // staging: soff | doff | poff (u64) | slen | dcap | dlen | rc (u32) | value bytes | member slots
    const uint64_t meta = al256(m * 8ull) * 3 + al256(m * 4ull) * 4;
    const uint64_t vb = al256(bytes + 16);
    int r = s->phost.ensure(meta + vb);
    if (!r) r = s->pdev.ensure(meta + vb + slots + 64);
    if (r) return fail_all(r);
    uint8_t *hp = (uint8_t *)s->phost.p, *dp = (uint8_t *)s->pdev.p;
    uint64_t *h_soff = (uint64_t *)hp, *h_doff = (uint64_t *)(hp + al256(m * 8ull));
    uint64_t *h_poff = (uint64_t *)(hp + al256(m * 8ull) * 2);
    uint32_t *h_slen = (uint32_t *)(hp + al256(m * 8ull) * 3);
    uint32_t *h_dcap = (uint32_t *)((uint8_t *)h_slen + al256(m * 4ull));
    uint32_t *h_dlen = (uint32_t *)((uint8_t *)h_dcap + al256(m * 4ull));
    int32_t *h_rc = (int32_t *)((uint8_t *)h_dlen + al256(m * 4ull));
    uint8_t *h_src = hp + meta;
    uint8_t *d_slots = dp + meta + vb;
    const uint64_t d_base = (uint64_t)(dp - hp);  // device address = host address + d_base
    auto dev = [&](void *h) { return (uint8_t *)h + d_base; };
    uint64_t so = 0, doff = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        h_soff[k] = so;
        h_slen[k] = src_len[i];
        memcpy(h_src + so, src + src_off[i], src_len[i]);
        so += src_len[i];
        h_doff[k] = doff;
        h_dcap[k] = (uint32_t)gzip_bound(src_len[i]);
        doff += (gzip_bound(src_len[i]) + 15) & ~(uint64_t)15;
    }
    hipStream_t st = ctx->stream;
    auto ok = [](hipError_t e) {
        if (e != hipSuccess) set_err("pmc_store_put_batch", e);
        return e == hipSuccess;
    };
    // 1. values in, members into the staging slots, lengths back
    if (!ok(hipMemcpyAsync(dp, hp, meta + bytes, hipMemcpyHostToDevice, st))) return fail_all(PMC_E_NO_DEVICE);
    r = pmc_gzip_compress_batch(ctx, dev(h_src), (uint64_t *)dev(h_soff), (uint32_t *)dev(h_slen), m, d_slots,
                                (uint64_t *)dev(h_doff), (uint32_t *)dev(h_dcap), (uint32_t *)dev(h_dlen),
                                (int32_t *)dev(h_rc), (uint32_t)max_len, st);
    if (r) return fail_all(r);
    if (!ok(hipMemcpyAsync(h_dlen, dev(h_dlen), al256(m * 4ull) * 2, hipMemcpyDeviceToHost, st)) ||
        !ok(hipStreamSynchronize(st)))
        return fail_all(PMC_E_NO_DEVICE);
    // 2. extents by compressed length
    {
        std::lock_guard<std::mutex> a(s->alloc_mu);
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = pick[k];
            if (h_rc[k] != PMC_OK) {
                rc[i] = h_rc[k];
                continue;
            }
            const uint32_t size = extent_size(h_dlen[k]);
            uint64_t off = 0;
            if (!store_alloc(s, size, &off)) {
                rc[i] = h_rc[k] = PMC_Z_MEM_ERROR;  // the compact pass skips it
                continue;
            }
            ext[i] = pmc_extent{off, size, h_dlen[k], src_len[i], 1};
            h_poff[k] = off;
        }
    }
    // 3. members from the slots into their extents (one H2D of the extent offsets and verdicts)
    bool moved = ok(hipMemcpyAsync(dev(h_poff), h_poff, m * 8ull, hipMemcpyHostToDevice, st)) &&
                 ok(hipMemcpyAsync(dev(h_rc), h_rc, m * 4ull, hipMemcpyHostToDevice, st));
    if (moved) {
        hipLaunchKernelGGL(compact_kernel, dim3(std::min<uint32_t>((m + 3) / 4, 8192)), dim3(256), 0, st,
                           (const uint8_t *)d_slots, (const uint64_t *)dev(h_doff), (const uint32_t *)dev(h_dlen),
                           (const int32_t *)dev(h_rc), (const uint64_t *)dev(h_poff), m, (uint8_t *)s->heap.p);
        moved = ok(hipGetLastError()) && ok(hipStreamSynchronize(st));
    }
    if (!moved) {  // the extents hold nothing: release them and fail their values
        std::lock_guard<std::mutex> a(s->alloc_mu);
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = pick[k];
            if (ext[i].flags & 1) store_release(s, ext[i]);
            rc[i] = PMC_E_NO_DEVICE;
        }
        return PMC_E_NO_DEVICE;
    }
    return PMC_OK;
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
    auto digits = [](uint32_t v) {
        uint32_t d = 1;
        while (v >= 10) {
            v /= 10;
            d++;
        }
        return d;
    };
    auto tail = [](int frame) -> uint32_t { return frame == PMC_FRAME_RESP ? 2 : frame == PMC_FRAME_CUSTOM ? 1 : 0; };
    for (uint32_t i = 0; i < n; i++) {
        const int frame = frame_of(i);
        resp[i] = nullptr;
        resp_len[i] = 0;
        if (!(ext[i].flags & 1) || ext[i].len == 0) {
            rc[i] = PMC_E_ARG;
            continue;
        }
        hlen[i] = (uint8_t)(frame == PMC_FRAME_RESP ? 1 + digits(ext[i].raw_len) + 2 : 0);
        pos[i] = total;
        total += hlen[i] + (uint64_t)ext[i].raw_len + tail(frame);
        max_raw = std::max<uint64_t>(max_raw, ext[i].raw_len);
        rc[i] = PMC_OK;
        pick.push_back(i);
    }
    const uint32_t m = (uint32_t)pick.size();
    if (m == 0) return PMC_OK;
    // device staging: soff | doff (u64) | slen | dcap | dlen | rc (u32) | response image
    const uint64_t meta = al256(m * 8ull) * 2 + al256(m * 4ull) * 4;
    int r = s->ghost.ensure(meta);
    if (!r) r = s->gdev.ensure(meta + total + 64);
    if (!r) r = s->hresp.ensure(total + 64);
    if (r) return r;
    uint8_t *hp = (uint8_t *)s->ghost.p, *dp = (uint8_t *)s->gdev.p;
    uint64_t *h_soff = (uint64_t *)hp, *h_doff = (uint64_t *)(hp + al256(m * 8ull));
    uint32_t *h_slen = (uint32_t *)(hp + al256(m * 8ull) * 2);
    uint32_t *h_dcap = (uint32_t *)((uint8_t *)h_slen + al256(m * 4ull));
    uint32_t *h_dlen = (uint32_t *)((uint8_t *)h_dcap + al256(m * 4ull));
    int32_t *h_rc = (int32_t *)((uint8_t *)h_dlen + al256(m * 4ull));
    const uint64_t d_base = (uint64_t)(dp - hp);
    auto dev = [&](void *h) { return (uint8_t *)h + d_base; };
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        h_soff[k] = ext[i].off;
        h_slen[k] = ext[i].len;
        h_doff[k] = pos[i] + hlen[i];
        h_dcap[k] = ext[i].raw_len;
    }
    hipStream_t st = s->gst;
    uint8_t *d_img = dp + meta, *img = (uint8_t *)s->hresp.p;
    HIP_TRY(hipMemcpyAsync(dp, hp, meta, hipMemcpyHostToDevice, st));
    r = pmc_gzip_decompress_batch(ctx, (const uint8_t *)s->heap.p, (uint64_t *)dev(h_soff), (uint32_t *)dev(h_slen),
                                  m, d_img, (uint64_t *)dev(h_doff), (uint32_t *)dev(h_dcap), (uint32_t *)dev(h_dlen),
                                  (int32_t *)dev(h_rc), (uint32_t)max_raw, st);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(h_dlen, dev(h_dlen), al256(m * 4ull) * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(img, d_img, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        if (h_rc[k] != PMC_OK || h_dlen[k] != ext[i].raw_len) {
            rc[i] = h_rc[k] != PMC_OK ? h_rc[k] : PMC_Z_DATA_ERROR;
            continue;
        }
        const int frame = frame_of(i);
        uint8_t *p = img + pos[i];
        if (frame == PMC_FRAME_RESP) {  // "$<len>\r\n" value "\r\n"  (protocol.cpp:466-497)
            const int nd = hlen[i] - 3;
            p[0] = '$';
            uint32_t v = ext[i].raw_len;
            for (int d = nd; d >= 1; d--) {
                p[d] = (uint8_t)('0' + v % 10);
                v /= 10;
            }
            p[nd + 1] = '\r';
            p[nd + 2] = '\n';
            p[hlen[i] + ext[i].raw_len] = '\r';
            p[hlen[i] + ext[i].raw_len + 1] = '\n';
        } else if (frame == PMC_FRAME_CUSTOM) {  // value + MSG_SEPARATOR (protocol.hpp:17)
            p[ext[i].raw_len] = 0x1F;
        }
        resp[i] = p;
        resp_len[i] = hlen[i] + ext[i].raw_len + tail(frame);
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
    auto digits = [](uint32_t v) {
        uint32_t d = 1;
        while (v >= 10) {
            v /= 10;
            d++;
        }
        return d;
    };
    const uint32_t tail = frame == PMC_FRAME_RESP ? 2 : frame == PMC_FRAME_CUSTOM ? 1 : 0;
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
        hlen[i] = (uint8_t)(frame == PMC_FRAME_RESP ? 1 + digits(r.L) + 2 : 0);
        pos[i] = total;
        total += hlen[i] + (uint64_t)r.L + tail;
        rc[i] = PMC_OK;
        live.push_back(i);
        // (an empty range needs no device work; a value of <= 4096 bytes cannot carry an index)
        if (r.L) (ext[i].raw_len > (1u << kIdxLog2Min) ? ranged : whole).push_back(i);
    }
    if (live.empty()) return PMC_OK;
    // device staging: soff | doff (u64) | slen | roff | rlen | dcap | dlen | rc (u32) | response image
    const uint32_t m = (uint32_t)ranged.size();
    const uint64_t a8 = al256(m * 8ull), a4 = al256(m * 4ull), meta = a8 * 2 + a4 * 6;
    int r = s->ghost.ensure(meta + 64);
    if (!r) r = s->gdev.ensure(meta + total + 64);
    if (!r) r = s->hresp.ensure(total + 64);
    if (r) return r;
    hipStream_t st = s->gst;
    uint8_t *d_img = (uint8_t *)s->gdev.p + meta, *img = (uint8_t *)s->hresp.p;
    if (m) {
        uint8_t *hp = (uint8_t *)s->ghost.p, *dp = (uint8_t *)s->gdev.p;
        uint64_t *h_soff = (uint64_t *)hp, *h_doff = (uint64_t *)(hp + a8);
        uint32_t *h_slen = (uint32_t *)(hp + a8 * 2), *h_roff = (uint32_t *)(hp + a8 * 2 + a4);
        uint32_t *h_rlen = (uint32_t *)(hp + a8 * 2 + a4 * 2), *h_dcap = (uint32_t *)(hp + a8 * 2 + a4 * 3);
        uint32_t *h_dlen = (uint32_t *)(hp + a8 * 2 + a4 * 4);
        int32_t *h_rc = (int32_t *)(hp + a8 * 2 + a4 * 5);
        const uint64_t d_base = (uint64_t)(dp - hp);
        auto dev = [&](void *h) { return (uint8_t *)h + d_base; };
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = ranged[k];
            h_soff[k] = ext[i].off;
            h_slen[k] = ext[i].len;
            h_roff[k] = ro[i];
            h_rlen[k] = rl[i];
            h_doff[k] = pos[i] + hlen[i];
            h_dcap[k] = rl[i];
        }
        HIP_TRY(hipMemcpyAsync(dp, hp, meta, hipMemcpyHostToDevice, st));
        r = pmc_gzip_decompress_range_batch(ctx, (const uint8_t *)s->heap.p, (uint64_t *)dev(h_soff), (uint32_t *)dev(h_slen),
                                            (uint32_t *)dev(h_roff), (uint32_t *)dev(h_rlen), m, d_img,
                                            (uint64_t *)dev(h_doff), (uint32_t *)dev(h_dcap), (uint32_t *)dev(h_dlen),
                                            (int32_t *)dev(h_rc), st);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(h_dlen, dev(h_dlen), a4 * 2, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = ranged[k];
            if (h_rc[k] == PMC_E_NO_INDEX) whole.push_back(i);
            else if (h_rc[k] != PMC_OK || h_dlen[k] != rl[i]) rc[i] = h_rc[k] != PMC_OK ? h_rc[k] : PMC_Z_DATA_ERROR;
        }
    }
    // the whole reads: extents while their values fit the budget, and the first one always
    for (size_t w0 = 0; w0 < whole.size();) {
        size_t w1 = w0;
        uint64_t bytes = 0, max_raw = 1;
        while (w1 < whole.size()) {
            const uint64_t need = ((uint64_t)ext[whole[w1]].raw_len + 15) & ~(uint64_t)15;
            if (w1 > w0 && bytes + need > kRangeFallbackBudget) break;
            bytes += need;
            max_raw = std::max<uint64_t>(max_raw, ext[whole[w1]].raw_len);
            w1++;
        }
        const uint32_t q = (uint32_t)(w1 - w0);
        // round staging: soff | doff | cut (slice source) | poff (u64) | slen | dcap | dlen | rc | clen (u32) | values
        const uint64_t b8 = al256(q * 8ull), b4 = al256(q * 4ull), rmeta = b8 * 4 + b4 * 5;
        r = s->rhost.ensure(rmeta);
        if (!r) r = s->rdev.ensure(rmeta + bytes + 64);
        if (r) return r;
        uint8_t *hp = (uint8_t *)s->rhost.p, *dp = (uint8_t *)s->rdev.p;
        uint64_t *h_soff = (uint64_t *)hp, *h_doff = (uint64_t *)(hp + b8), *h_cut = (uint64_t *)(hp + b8 * 2);
        uint64_t *h_poff = (uint64_t *)(hp + b8 * 3);
        uint32_t *h_slen = (uint32_t *)(hp + b8 * 4), *h_dcap = (uint32_t *)(hp + b8 * 4 + b4);
        uint32_t *h_dlen = (uint32_t *)(hp + b8 * 4 + b4 * 2);
        int32_t *h_rc = (int32_t *)(hp + b8 * 4 + b4 * 3);
        uint32_t *h_clen = (uint32_t *)(hp + b8 * 4 + b4 * 4);
        const uint64_t d_base = (uint64_t)(dp - hp);
        auto dev = [&](void *h) { return (uint8_t *)h + d_base; };
        uint64_t at = 0;
        for (uint32_t k = 0; k < q; k++) {
            const uint32_t i = whole[w0 + k];
            h_soff[k] = ext[i].off;
            h_slen[k] = ext[i].len;
            h_doff[k] = at;
            h_dcap[k] = ext[i].raw_len;
            h_cut[k] = at + ro[i];
            h_clen[k] = rl[i];
            h_poff[k] = pos[i] + hlen[i];
            at += ((uint64_t)ext[i].raw_len + 15) & ~(uint64_t)15;
        }
        uint8_t *d_vals = dp + rmeta;
        HIP_TRY(hipMemcpyAsync(dp, hp, rmeta, hipMemcpyHostToDevice, st));
        r = pmc_gzip_decompress_batch(ctx, (const uint8_t *)s->heap.p, (uint64_t *)dev(h_soff), (uint32_t *)dev(h_slen), q,
                                      d_vals, (uint64_t *)dev(h_doff), (uint32_t *)dev(h_dcap), (uint32_t *)dev(h_dlen),
                                      (int32_t *)dev(h_rc), (uint32_t)max_raw, st);
        if (r) return r;
        // the slices of the values that decoded (rc 0) into their places in the image
        hipLaunchKernelGGL(compact_kernel, dim3(std::min<uint32_t>((q + 3) / 4, 8192)), dim3(256), 0, st,
                           (const uint8_t *)d_vals, (const uint64_t *)dev(h_cut), (const uint32_t *)dev(h_clen),
                           (const int32_t *)dev(h_rc), (const uint64_t *)dev(h_poff), q, d_img);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_dlen, dev(h_dlen), b4 * 2, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < q; k++) {
            const uint32_t i = whole[w0 + k];
            if (h_rc[k] != PMC_OK || h_dlen[k] != ext[i].raw_len) rc[i] = h_rc[k] != PMC_OK ? h_rc[k] : PMC_Z_DATA_ERROR;
        }
        w0 = w1;
    }
    if (total) {
        HIP_TRY(hipMemcpyAsync(img, d_img, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (uint32_t i : live) {
        if (rc[i] != PMC_OK) continue;
        uint8_t *p = img + pos[i];
        if (frame == PMC_FRAME_RESP) { // "$<len>\r\n" range bytes "\r\n"
            const int nd = hlen[i] - 3;
            p[0] = '$';
            uint32_t v = rl[i];
            for (int d = nd; d >= 1; d--) {
                p[d] = (uint8_t)('0' + v % 10);
                v /= 10;
            }
            p[nd + 1] = '\r';
            p[nd + 2] = '\n';
            p[hlen[i] + rl[i]] = '\r';
            p[hlen[i] + rl[i] + 1] = '\n';
        } else if (frame == PMC_FRAME_CUSTOM) {
            p[rl[i]] = 0x1F;
        }
        resp[i] = p;
        resp_len[i] = hlen[i] + rl[i] + tail;
    }
    return PMC_OK;
}

// Ranged set (include/pmc_codec.h pmc_store_set_range_batch): the rewrite call over the heap for the extents
// that may carry an index; whole read, overlay and compress, in rounds of bounded scratch, for those it declined
// and the small ones; then new extents by member length, the members compacted in, and the old extents released.
PMC_API int pmc_store_set_range_batch(pmc_store *s, pmc_extent *ext, const uint8_t *src, const uint64_t *src_off,
                                      const uint32_t *src_len, const uint32_t *range_off, uint32_t n, int32_t *rc) {
    if (!s || (n && (!ext || !src || !src_off || !src_len || !range_off || !rc))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    std::lock_guard<std::mutex> get_lock(s->get_mu);
    StoreCall call(s, s->put_mu);
    pmc_ctx *ctx = s->ctx;
    // live, in-bounds, distinct extents; an empty patch changes nothing
    std::unordered_map<uint64_t, uint32_t> seen;
    for (uint32_t i = 0; i < n; i++) {
        const bool live = (ext[i].flags & 1) && ext[i].len;
        rc[i] = live && (uint64_t)range_off[i] + src_len[i] <= ext[i].raw_len ? PMC_OK : PMC_E_ARG;
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
    // put staging: soff | poff | doff | noff (u64) | slen | plen | roff | dcap | dlen | rc (u32) | patches | slots
    const uint64_t a8 = al256(m * 8ull), a4 = al256(m * 4ull), meta = a8 * 4 + a4 * 6;
    uint64_t pbytes = 0, slots = 0;
    for (uint32_t k = 0; k < m; k++) {
        pbytes += src_len[pick[k]];
        slots += (gzip_bound(ext[pick[k]].raw_len) + 15) & ~(uint64_t)15;
    }
    const uint64_t pb = al256(pbytes + 16);
    int r = s->phost.ensure(meta + pb);
    if (!r) r = s->pdev.ensure(meta + pb + slots + 64);
    if (r) return fail_all(r);
    uint8_t *hp = (uint8_t *)s->phost.p, *dp = (uint8_t *)s->pdev.p;
    uint64_t *h_soff = (uint64_t *)hp, *h_poff = (uint64_t *)(hp + a8), *h_doff = (uint64_t *)(hp + a8 * 2);
    uint64_t *h_noff = (uint64_t *)(hp + a8 * 3);
    uint32_t *h_slen = (uint32_t *)(hp + a8 * 4), *h_plen = (uint32_t *)(hp + a8 * 4 + a4);
    uint32_t *h_roff = (uint32_t *)(hp + a8 * 4 + a4 * 2), *h_dcap = (uint32_t *)(hp + a8 * 4 + a4 * 3);
    uint32_t *h_dlen = (uint32_t *)(hp + a8 * 4 + a4 * 4);
    int32_t *h_rc = (int32_t *)(hp + a8 * 4 + a4 * 5);
    uint8_t *h_patch = hp + meta, *d_patch = dp + meta, *d_slots = dp + meta + pb;
    const uint64_t d_base = (uint64_t)(dp - hp);
    auto dev = [&](void *h) { return (uint8_t *)h + d_base; };
    uint64_t po = 0, doff = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        h_soff[k] = ext[i].off;
        h_slen[k] = ext[i].len;
        h_poff[k] = po;
        h_plen[k] = src_len[i];
        h_roff[k] = range_off[i];
        memcpy(h_patch + po, src + src_off[i], src_len[i]);
        po += src_len[i];
        h_doff[k] = doff;
        h_dcap[k] = (uint32_t)gzip_bound(ext[i].raw_len);
        doff += (gzip_bound(ext[i].raw_len) + 15) & ~(uint64_t)15;
        h_dlen[k] = 0;
        h_rc[k] = k < mc ? PMC_OK : PMC_E_NO_INDEX; // (the small ones take the full path)
    }
    hipStream_t st = ctx->stream;
    auto ok = [](hipError_t e) {
        if (e != hipSuccess) set_err("pmc_store_set_range_batch", e);
        return e == hipSuccess;
    };
    if (!ok(hipMemcpyAsync(dp, hp, meta + pbytes, hipMemcpyHostToDevice, st))) return fail_all(PMC_E_NO_DEVICE);
    // 1. the chunk path
    if (mc) {
        r = pmc_gzip_rewrite_range_batch(ctx, (const uint8_t *)s->heap.p, (uint64_t *)dev(h_soff), (uint32_t *)dev(h_slen),
                                         d_patch, (uint64_t *)dev(h_poff), (uint32_t *)dev(h_plen),
                                         (uint32_t *)dev(h_roff), mc, d_slots, (uint64_t *)dev(h_doff),
                                         (uint32_t *)dev(h_dcap), (uint32_t *)dev(h_dlen), (int32_t *)dev(h_rc), st);
        if (r) return fail_all(r);
        if (!ok(hipMemcpyAsync(h_dlen, dev(h_dlen), mc * 4ull, hipMemcpyDeviceToHost, st)) ||
            !ok(hipMemcpyAsync(h_rc, dev(h_rc), mc * 4ull, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st)))
            return fail_all(PMC_E_NO_DEVICE);
    }
    for (uint32_t k = 0; k < m; k++)
        if (h_rc[k] == PMC_E_NO_INDEX) full.push_back(k);
    // 2. the full path: extents while their values fit the budget, and the first one always
    for (size_t w0 = 0; w0 < full.size();) {
        size_t w1 = w0;
        uint64_t bytes = 0, max_raw = 1;
        while (w1 < full.size()) {
            const uint64_t need = ((uint64_t)ext[pick[full[w1]]].raw_len + 15) & ~(uint64_t)15;
            if (w1 > w0 && bytes + need > kRangeFallbackBudget) break;
            bytes += need;
            max_raw = std::max<uint64_t>(max_raw, ext[pick[full[w1]]].raw_len);
            w1++;
        }
        const uint32_t q = (uint32_t)(w1 - w0);
        // round staging: soff | voff | cut | poff | doff (u64) | slen | vcap | vlen | vrc | plen | dcap | dlen | rc (u32) |
        // values
        const uint64_t b8 = al256(q * 8ull), b4 = al256(q * 4ull), rmeta = b8 * 5 + b4 * 8;
        r = s->rhost.ensure(rmeta);
        if (!r) r = s->rdev.ensure(rmeta + bytes + 64);
        if (r) return fail_all(r);
        uint8_t *rh = (uint8_t *)s->rhost.p, *rd = (uint8_t *)s->rdev.p;
        uint64_t *g_soff = (uint64_t *)rh, *g_voff = (uint64_t *)(rh + b8), *g_cut = (uint64_t *)(rh + b8 * 2);
        uint64_t *g_poff = (uint64_t *)(rh + b8 * 3), *g_doff = (uint64_t *)(rh + b8 * 4);
        uint32_t *g_slen = (uint32_t *)(rh + b8 * 5), *g_vcap = (uint32_t *)(rh + b8 * 5 + b4);
        uint32_t *g_vlen = (uint32_t *)(rh + b8 * 5 + b4 * 2);
        int32_t *g_vrc = (int32_t *)(rh + b8 * 5 + b4 * 3);
        uint32_t *g_plen = (uint32_t *)(rh + b8 * 5 + b4 * 4), *g_dcap = (uint32_t *)(rh + b8 * 5 + b4 * 5);
        uint32_t *g_dlen = (uint32_t *)(rh + b8 * 5 + b4 * 6);
        int32_t *g_rc = (int32_t *)(rh + b8 * 5 + b4 * 7);
        const uint64_t r_base = (uint64_t)(rd - rh);
        auto rdev = [&](void *h) { return (uint8_t *)h + r_base; };
        uint64_t at = 0;
        for (uint32_t j = 0; j < q; j++) {
            const uint32_t k = full[w0 + j], i = pick[k];
            g_soff[j] = ext[i].off;
            g_slen[j] = ext[i].len;
            g_voff[j] = at;
            g_vcap[j] = ext[i].raw_len;
            g_cut[j] = at + range_off[i];
            g_poff[j] = h_poff[k];
            g_plen[j] = src_len[i];
            g_doff[j] = h_doff[k];
            g_dcap[j] = h_dcap[k];
            at += ((uint64_t)ext[i].raw_len + 15) & ~(uint64_t)15;
        }
        uint8_t *d_vals = rd + rmeta;
        if (!ok(hipMemcpyAsync(rd, rh, rmeta, hipMemcpyHostToDevice, st))) return fail_all(PMC_E_NO_DEVICE);
        r = pmc_gzip_decompress_batch(ctx, (const uint8_t *)s->heap.p, (uint64_t *)rdev(g_soff), (uint32_t *)rdev(g_slen), q,
                                      d_vals, (uint64_t *)rdev(g_voff), (uint32_t *)rdev(g_vcap), (uint32_t *)rdev(g_vlen),
                                      (int32_t *)rdev(g_vrc), (uint32_t)max_raw, st);
        if (r) return fail_all(r);
        // the patches over the values that decoded (rc 0), then the values compressed into their slots
        hipLaunchKernelGGL(compact_kernel, dim3(std::min<uint32_t>((q + 3) / 4, 8192)), dim3(256), 0, st,
                           (const uint8_t *)d_patch, (const uint64_t *)rdev(g_poff), (const uint32_t *)rdev(g_plen),
                           (const int32_t *)rdev(g_vrc), (const uint64_t *)rdev(g_cut), q, d_vals);
        if (!ok(hipGetLastError())) return fail_all(PMC_E_NO_DEVICE);
        r = pmc_gzip_compress_batch(ctx, d_vals, (uint64_t *)rdev(g_voff), (uint32_t *)rdev(g_vcap), q, d_slots,
                                    (uint64_t *)rdev(g_doff), (uint32_t *)rdev(g_dcap), (uint32_t *)rdev(g_dlen),
                                    (int32_t *)rdev(g_rc), (uint32_t)max_raw, st);
        if (r) return fail_all(r);
        if (!ok(hipMemcpyAsync(g_vlen, rdev(g_vlen), b4 * 2, hipMemcpyDeviceToHost, st)) ||
            !ok(hipMemcpyAsync(g_dlen, rdev(g_dlen), b4 * 2, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st)))
            return fail_all(PMC_E_NO_DEVICE);
        for (uint32_t j = 0; j < q; j++) {
            const uint32_t k = full[w0 + j], i = pick[k];
            if (g_vrc[j] != PMC_OK || g_vlen[j] != ext[i].raw_len) h_rc[k] = g_vrc[j] != PMC_OK ? g_vrc[j] : PMC_Z_DATA_ERROR;
            else h_rc[k] = g_rc[j];
            h_dlen[k] = g_dlen[j];
        }
        w0 = w1;
    }
    // 3. new extents by member length (the old ones stay until the members are in)
    std::vector<pmc_extent> fresh(m, pmc_extent{0, 0, 0, 0, 0});
    {
        std::lock_guard<std::mutex> a(s->alloc_mu);
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = pick[k];
            h_noff[k] = 0;
            if (h_rc[k] != PMC_OK) {
                rc[i] = h_rc[k];
                continue;
            }
            const uint32_t size = extent_size(h_dlen[k]);
            uint64_t off = 0;
            if (!store_alloc(s, size, &off)) {
                rc[i] = h_rc[k] = PMC_Z_MEM_ERROR; // the compact pass skips it
                continue;
            }
            fresh[k] = pmc_extent{off, size, h_dlen[k], ext[i].raw_len, 1};
            h_noff[k] = off;
        }
    }
    // 4. members from the slots into the new extents
    bool moved = ok(hipMemcpyAsync(dev(h_noff), h_noff, m * 8ull, hipMemcpyHostToDevice, st)) &&
                 ok(hipMemcpyAsync(dev(h_rc), h_rc, m * 4ull, hipMemcpyHostToDevice, st)) &&
                 ok(hipMemcpyAsync(dev(h_dlen), h_dlen, m * 4ull, hipMemcpyHostToDevice, st));
    if (moved) {
        hipLaunchKernelGGL(compact_kernel, dim3(std::min<uint32_t>((m + 3) / 4, 8192)), dim3(256), 0, st,
                           (const uint8_t *)d_slots, (const uint64_t *)dev(h_doff), (const uint32_t *)dev(h_dlen),
                           (const int32_t *)dev(h_rc), (const uint64_t *)dev(h_noff), m, (uint8_t *)s->heap.p);
        moved = ok(hipGetLastError()) && ok(hipStreamSynchronize(st));
    }
    std::lock_guard<std::mutex> a(s->alloc_mu);
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = pick[k];
        if (!(fresh[k].flags & 1)) continue;
        if (!moved) { // the new extents hold nothing: the old ones stay
            store_release(s, fresh[k]);
            rc[i] = PMC_E_NO_DEVICE;
            continue;
        }
        store_release(s, ext[i]);
        ext[i] = fresh[k];
    }
    return moved ? PMC_OK : PMC_E_NO_DEVICE;
}

PMC_API int pmc_store_read_members(pmc_store *s, const pmc_extent *ext, uint32_t n, uint8_t *dst,
                                   const uint64_t *dst_off) {
    if (!s || (n && (!ext || !dst || !dst_off))) return PMC_E_ARG;
    if (n == 0) return PMC_OK;
    StoreCall call(s, s->get_mu);
    for (uint32_t i = 0; i < n; i++)
        if (!(ext[i].flags & 1)) return PMC_E_ARG;
    // gather the members on the device (compact_kernel), then one D2H
    const uint64_t meta = al256(n * 8ull) * 2 + al256(n * 4ull) * 2;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += ext[i].len;
    int r = s->ghost.ensure(meta + total + 64);
    if (!r) r = s->gdev.ensure(meta + total + 64);
    if (r) return r;
    uint8_t *hp = (uint8_t *)s->ghost.p, *dp = (uint8_t *)s->gdev.p;
    uint64_t *h_soff = (uint64_t *)hp, *h_poff = (uint64_t *)(hp + al256(n * 8ull));
    uint32_t *h_len = (uint32_t *)(hp + al256(n * 8ull) * 2);
    int32_t *h_rc = (int32_t *)((uint8_t *)h_len + al256(n * 4ull));
    const uint64_t d_base = (uint64_t)(dp - hp);
    auto dev = [&](void *h) { return (uint8_t *)h + d_base; };
    uint64_t p = 0;
    for (uint32_t i = 0; i < n; i++) {
        h_soff[i] = ext[i].off;
        h_poff[i] = p;
        h_len[i] = ext[i].len;
        h_rc[i] = 0;
        p += ext[i].len;
    }
    hipStream_t st = s->gst;
    HIP_TRY(hipMemcpyAsync(dp, hp, meta, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(compact_kernel, dim3(std::min<uint32_t>((n + 3) / 4, 8192)), dim3(256), 0, st,
                       (const uint8_t *)s->heap.p, (const uint64_t *)dev(h_soff), (const uint32_t *)dev(h_len),
                       (const int32_t *)dev(h_rc), (const uint64_t *)dev(h_poff), n, dp + meta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hp + meta, dp + meta, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; i++) memcpy(dst + dst_off[i], hp + meta + h_poff[i], ext[i].len);
    return PMC_OK;
}

PMC_API int pmc_store_free(pmc_store *s, pmc_extent *ext, uint32_t n) {
    if (!s || (n && !ext)) return PMC_E_ARG;
    std::lock_guard<std::mutex> lock(s->alloc_mu);
    for (uint32_t i = 0; i < n; i++) store_release(s, ext[i]);
    return PMC_OK;
}

PMC_API uint8_t *pmc_store_data(pmc_store *s) { return s ? (uint8_t *)s->heap.p : nullptr; }

PMC_API int pmc_store_stats(pmc_store *s, uint64_t *used, uint64_t *reserved, uint64_t *heap) {
    if (!s) return PMC_E_ARG;
    std::lock_guard<std::mutex> lock(s->alloc_mu);
    if (used) *used = s->used;
    if (reserved) *reserved = s->bump;
    if (heap) *heap = s->heap_bytes;
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

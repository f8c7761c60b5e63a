// pmc_store_plan.hpp -- the host-side arithmetic of the device store and the group calls: the heap allocator
// (StoreHeap), where the arrays of every call's staging lie (the named layouts over pmc_plan.hpp's StageCarver), the wire
// framing of a response (frame_head / frame_tail / frame_write) and how the values a ranged call read whole are
// cut into rounds (cut_round).  Plain C++17 with no HIP in it: pmc_store.hip and pmc_group.hip turn these into
// copies and launches, and tests/host/store_check.cpp prints them for tests/test_host_store.py, which needs
// no GPU.
#pragma once
#include <unordered_map>

#include "pmc_plan.hpp"

namespace pmc {

inline uint64_t round16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// ---- the heap allocator ------------------------------------------------------------------------------------
// Extents of the member's length rounded up (extent_size), a free list per exact size, last in first out,
// bump allocation otherwise.  No lock of its own: pmc_store's alloc_mu is held around every call.
struct StoreHeap {
    uint64_t heap_bytes = 0, bump = 0, used = 0;
    std::unordered_map<uint32_t, std::vector<uint64_t>> free_lists; // extent size -> offsets

    // bytes reserved for a member of `len` bytes: 16-byte granules, and above 8 KiB steps of 1/8 of
    // the power of two below (bounded waste, few distinct free-list sizes)
    static uint32_t extent_size(uint64_t len) {
        uint64_t c = round16(len);
        if (c > 8192) {
            uint64_t p = 1;
            while (p * 2 <= c) p *= 2;
            const uint64_t step = p / 8;
            c = (c + step - 1) / step * step;
        }
        return (uint32_t)c;
    }
    // an extent of `size` bytes: the newest entry of its size's list, else the bump; false (and nothing
    // changed) where neither can serve
    bool alloc(uint32_t size, uint64_t *off) {
        auto it = free_lists.find(size);
        if (it != free_lists.end() && !it->second.empty()) {
            *off = it->second.back();
            it->second.pop_back();
        } else {
            if (bump + size > heap_bytes) return false;
            *off = bump;
            bump += size;
        }
        used += size;
        return true;
    }
    void release(pmc_extent &e) { // (an extent that is not live: nothing)
        if (!(e.flags & 1)) return;
        free_lists[e.cap].push_back(e.off);
        used -= e.cap;
        e.flags = 0;
    }
};

// ---- staging layouts ---------------------------------------------------------------------------------------
// The store's layouts over pmc_plan.hpp's StageCarver, one per call site (members are initialised in declaration
// order: that order is the layout).
struct PutStage { // pmc_store_put_batch: ... | value bytes | member slots
    PMC_STAGE(PutStage);
    StageArr<uint64_t> soff = c.u64(), doff = c.u64(), poff = c.u64();
    StageArr<uint32_t> slen = c.u32(), dcap = c.u32(), dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    StageSpan dlen_rc = c.span(dlen, rc);
    uint64_t meta = c.meta;
};
struct GetStage { // store_get: ... | response image; group_share: ... | values | outputs
    PMC_STAGE(GetStage);
    StageArr<uint64_t> soff = c.u64(), doff = c.u64();
    StageArr<uint32_t> slen = c.u32(), dcap = c.u32(), dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    StageSpan dlen_rc = c.span(dlen, rc);
    uint64_t meta = c.meta;
};
struct RangeGetStage { // pmc_store_get_range_batch, the ranged call: ... | response image
    PMC_STAGE(RangeGetStage);
    StageArr<uint64_t> soff = c.u64(), doff = c.u64();
    StageArr<uint32_t> slen = c.u32(), roff = c.u32(), rlen = c.u32(), dcap = c.u32(), dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    StageSpan dlen_rc = c.span(dlen, rc);
    uint64_t meta = c.meta;
};
struct RangeGetRound { // its fallback round (cut: the slice's source, poff: its place in the image): ... | values
    PMC_STAGE(RangeGetRound);
    StageArr<uint64_t> soff = c.u64(), doff = c.u64(), cut = c.u64(), poff = c.u64();
    StageArr<uint32_t> slen = c.u32(), dcap = c.u32(), dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    StageArr<uint32_t> clen = c.u32();
    StageSpan dlen_rc = c.span(dlen, rc);
    uint64_t meta = c.meta;
};
struct RangeSetStage { // pmc_store_set_range_batch (noff: the new extents): ... | patches | member slots
    PMC_STAGE(RangeSetStage);
    StageArr<uint64_t> soff = c.u64(), poff = c.u64(), doff = c.u64(), noff = c.u64();
    StageArr<uint32_t> slen = c.u32(), plen = c.u32(), roff = c.u32(), dcap = c.u32(), dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    uint64_t meta = c.meta;
};
struct RangeSetRound { // its fallback round (v*: the whole values it decodes): ... | values
    PMC_STAGE(RangeSetRound);
    StageArr<uint64_t> soff = c.u64(), voff = c.u64(), cut = c.u64(), poff = c.u64(), doff = c.u64();
    StageArr<uint32_t> slen = c.u32(), vcap = c.u32(), vlen = c.u32();
    StageArr<int32_t> vrc = c.i32();
    StageArr<uint32_t> plen = c.u32(), dcap = c.u32(), dlen = c.u32();
    StageArr<int32_t> rc = c.i32();
    StageSpan vlen_vrc = c.span(vlen, vrc), dlen_rc = c.span(dlen, rc);
    uint64_t meta = c.meta;
};
// the round as the ranged and growing sets use it: behind RangeSetRound's arrays the values' new lengths (vcap:
// what the old member decodes to; nlen: what is compressed -- the same where the value does not grow)
struct RangeWriteRound : RangeSetRound {
    explicit RangeWriteRound(uint64_t m, void *host = nullptr, void *dev = nullptr) : RangeSetRound(m, host, dev) {}
    StageArr<uint32_t> nlen = c.u32();
    uint64_t meta = c.meta;
};
struct MembersStage { // pmc_store_read_members: ... | members
    PMC_STAGE(MembersStage);
    StageArr<uint64_t> soff = c.u64(), poff = c.u64();
    StageArr<uint32_t> len = c.u32();
    StageArr<int32_t> rc = c.i32();
    uint64_t meta = c.meta;
};
#undef PMC_STAGE

// ---- wire framing ------------------------------------------------------------------------------------------
// A response of L value bytes in frame PMC_FRAME_*: frame_head bytes, the value, frame_tail bytes.
// RESP: "$<L>\r\n" value "\r\n" (the reference's protocol.cpp:466-497); custom: value + MSG_SEPARATOR 0x1F
// (protocol.hpp:17); raw: the value alone.
inline uint32_t frame_head(int frame, uint32_t L) {
    if (frame != PMC_FRAME_RESP) return 0;
    uint32_t d = 1;
    for (uint32_t v = L; v >= 10; v /= 10) d++;
    return 1 + d + 2;
}
inline uint32_t frame_tail(int frame) { return frame == PMC_FRAME_RESP ? 2 : frame == PMC_FRAME_CUSTOM ? 1 : 0; }
// Writes head and tail around the L value bytes at p + frame_head (which it leaves alone).
inline void frame_write(uint8_t *p, int frame, uint32_t L) {
    if (frame == PMC_FRAME_RESP) {
        const uint32_t head = frame_head(frame, L);
        p[0] = '$';
        uint32_t v = L;
        for (uint32_t d = head - 3; d >= 1; d--) {
            p[d] = (uint8_t)('0' + v % 10);
            v /= 10;
        }
        p[head - 2] = '\r';
        p[head - 1] = '\n';
        p[head + (uint64_t)L] = '\r';
        p[head + (uint64_t)L + 1] = '\n';
    } else if (frame == PMC_FRAME_CUSTOM) {
        p[L] = 0x1F;
    }
}

// ---- growing sets ------------------------------------------------------------------------------------------
// A value of raw_len bytes after a write of len bytes at off (len > 0): max(raw_len, off + len) bytes.  The store
// takes no value longer than the server's MAX_REQUEST_SIZE, Redis's own limit for APPEND and SETRANGE.
constexpr uint64_t kStoreGrowMax = 536870912;
inline uint64_t grown_len(uint32_t raw_len, uint32_t off, uint32_t len) {
    return std::max<uint64_t>(raw_len, (uint64_t)off + len);
}

// ---- fallback rounds ---------------------------------------------------------------------------------------
// The round that starts at raw_len[start] (start < n): values while their 16-byte-rounded lengths fit the
// budget, and the first one always.  The budget counts the values' bytes only, not the round's arrays.
struct FallbackRound {
    size_t end;      // the next round's start
    uint64_t bytes;  // the values' rounded lengths
    uint64_t max_raw;
};
inline FallbackRound cut_round(const uint32_t *raw_len, size_t n, size_t start, uint64_t budget) {
    FallbackRound r{start, 0, 1};
    while (r.end < n) {
        const uint64_t need = round16(raw_len[r.end]);
        if (r.end > start && r.bytes + need > budget) break;
        r.bytes += need;
        r.max_raw = std::max<uint64_t>(r.max_raw, raw_len[r.end]);
        r.end++;
    }
    return r;
}

} // namespace pmc

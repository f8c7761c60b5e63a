// store_check.cpp -- the host arithmetic of the device store (csrc/pmc_store_plan.hpp: StoreHeap, the staging
// layouts, the framer, cut_round), for tests/test_host_store.py.  Plain C++ with no HIP in it; the test builds it
// with the address and undefined-behaviour sanitizers and runs it directly.
//
//   store_check layout <m> ...           one JSON object per m: every layout's offsets, meta and spans
//   store_check frame <frame> <L> ...    one JSON object per L: head and tail as written around L value bytes
//   store_check cut <budget> <len> ...   the rounds over the lengths (budget 0: kRangeFallbackBudget)
//   store_check heap <heap_bytes>        ops on stdin, "a <member_len>" / "r <off>": one JSON object per op
#include <sys/mman.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../poor-man-s-cache_amd/csrc/pmc_store_plan.hpp"

using namespace pmc;

namespace {

// never dereferenced: the bases a bound layout's pointers are checked against
uint8_t *const kHost = (uint8_t *)0x100000, *const kDev = (uint8_t *)0x7f0000000000;
bool g_bound_ok = true;

// one array of a layout: its offset printed, and the same array of the layout bound to the bases checked
template <class T>
void arr(const char *name, const StageArr<T> &a, const StageArr<T> &b) {
    g_bound_ok = g_bound_ok && a.off == b.off && (uint8_t *)b.h == kHost + a.off && (uint8_t *)b.d == kDev + a.off;
    printf(", \"%s\": %" PRIu64, name, a.off);
}
void span(const char *name, const StageSpan &s, const StageSpan &b, uint64_t off) {
    g_bound_ok = g_bound_ok && (uint8_t *)b.h == kHost + off && (uint8_t *)b.d == kDev + off && b.bytes == s.bytes;
    printf(", \"%s\": %" PRIu64, name, s.bytes);
}
// L: the layout as the call sites size it (no bases); B: the same layout bound to the bases
#define OPEN(Type, name)                         \
    const Type L(m), B(m, kHost, kDev);          \
    g_bound_ok = g_bound_ok && L.meta == B.meta; \
    printf(", \"" name "\": {\"meta\": %" PRIu64, L.meta)
#define ARR(x) arr(#x, L.x, B.x)
#define SPAN(x, first) span(#x, L.x, B.x, L.first.off)
#define CLOSE() printf("}")

void layouts(uint64_t m) {
    printf("{\"m\": %" PRIu64, m);
    {
        OPEN(PutStage, "put");
        ARR(soff), ARR(doff), ARR(poff), ARR(slen), ARR(dcap), ARR(dlen), ARR(rc), SPAN(dlen_rc, dlen), CLOSE();
    }
    {
        OPEN(GetStage, "get");
        ARR(soff), ARR(doff), ARR(slen), ARR(dcap), ARR(dlen), ARR(rc), SPAN(dlen_rc, dlen), CLOSE();
    }
    {
        OPEN(RangeGetStage, "range_get");
        ARR(soff), ARR(doff), ARR(slen), ARR(roff), ARR(rlen), ARR(dcap), ARR(dlen), ARR(rc), SPAN(dlen_rc, dlen), CLOSE();
    }
    {
        OPEN(RangeGetRound, "range_get_round");
        ARR(soff), ARR(doff), ARR(cut), ARR(poff), ARR(slen), ARR(dcap), ARR(dlen), ARR(rc), ARR(clen), SPAN(dlen_rc, dlen),
            CLOSE();
    }
    {
        OPEN(RangeSetStage, "range_set");
        ARR(soff), ARR(poff), ARR(doff), ARR(noff), ARR(slen), ARR(plen), ARR(roff), ARR(dcap), ARR(dlen), ARR(rc), CLOSE();
    }
    {
        OPEN(RangeSetRound, "range_set_round");
        ARR(soff), ARR(voff), ARR(cut), ARR(poff), ARR(doff), ARR(slen), ARR(vcap), ARR(vlen), ARR(vrc), ARR(plen), ARR(dcap),
            ARR(dlen), ARR(rc), SPAN(vlen_vrc, vlen), SPAN(dlen_rc, dlen), CLOSE();
    }
    {
        OPEN(MembersStage, "members");
        ARR(soff), ARR(poff), ARR(len), ARR(rc), CLOSE();
    }
    printf(", \"bound_ok\": %d}\n", g_bound_ok ? 1 : 0);
}

std::string hex(const uint8_t *p, size_t n) {
    std::string s;
    char b[3];
    for (size_t i = 0; i < n; i++) {
        snprintf(b, sizeof b, "%02x", p[i]);
        s += b;
    }
    return s;
}

// frame_write around L value bytes that lie 64 bytes into a mapping of canary bytes.  The first and the last
// 8 KiB of the mapping are checked byte by byte; what lies between (value bytes only: head and tail are within
// 16 bytes of the value's ends) is made unwritable, so a write there ends the program.
int frame_case(int frame, uint32_t L) {
    const uint32_t head = frame_head(frame, L), tail = frame_tail(frame);
    const uint64_t kEdge = 8192, kGuard = 64, kCanary = 0xA5;
    const uint64_t used = kGuard + head + (uint64_t)L + tail + kGuard, map = (used + 4095) & ~(uint64_t)4095;
    uint8_t *buf = (uint8_t *)mmap(nullptr, map, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (buf == MAP_FAILED) return 3;
    const uint64_t lo_end = std::min(map, kEdge), hi_at = std::max(lo_end, map - std::min(map, kEdge));
    memset(buf, (int)kCanary, lo_end);
    memset(buf + hi_at, (int)kCanary, map - hi_at);
    if (hi_at > lo_end && mprotect(buf + lo_end, hi_at - lo_end, PROT_NONE) != 0) return 3;
    uint8_t *p = buf + kGuard;
    frame_write(p, frame, L);
    const uint64_t t0 = kGuard + head + (uint64_t)L; // the tail's offset in the mapping
    uint64_t touched = 0;
    auto scan = [&](uint64_t a, uint64_t b) {
        for (uint64_t o = a; o < b; o++) {
            const bool ours = (o >= kGuard && o < kGuard + head) || (o >= t0 && o < t0 + tail);
            if (!ours && buf[o] != kCanary) touched++;
        }
    };
    scan(0, lo_end);
    scan(hi_at, map);
    printf("{\"frame\": %d, \"L\": %u, \"head\": %u, \"tail\": %u, \"head_hex\": \"%s\", \"tail_hex\": \"%s\", "
           "\"touched_outside\": %" PRIu64 "}\n",
           frame, L, head, tail, hex(p, head).c_str(), hex(buf + t0, tail).c_str(), touched);
    munmap(buf, map);
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "layout")) {
        for (int k = 2; k < argc; k++) layouts(strtoull(argv[k], nullptr, 10));
        return 0;
    }
    if (!strcmp(argv[1], "frame")) {
        if (argc < 4) return 2;
        const int frame = atoi(argv[2]);
        for (int k = 3; k < argc; k++)
            if (int r = frame_case(frame, (uint32_t)strtoull(argv[k], nullptr, 10))) return r;
        return 0;
    }
    if (!strcmp(argv[1], "cut")) {
        if (argc < 3) return 2;
        uint64_t budget = strtoull(argv[2], nullptr, 10);
        if (budget == 0) budget = kRangeFallbackBudget;
        std::vector<uint32_t> len;
        for (int k = 3; k < argc; k++) len.push_back((uint32_t)strtoull(argv[k], nullptr, 10));
        printf("{\"budget\": %" PRIu64 ", \"rounds\": [", budget);
        for (size_t w0 = 0; w0 < len.size();) {
            const FallbackRound R = cut_round(len.data(), len.size(), w0, budget);
            if (R.end <= w0) return 3; // a round takes its first value always
            printf("%s{\"start\": %zu, \"end\": %zu, \"bytes\": %" PRIu64 ", \"max_raw\": %" PRIu64 "}", w0 ? ", " : "", w0,
                   R.end, R.bytes, R.max_raw);
            w0 = R.end;
        }
        printf("]}\n");
        return 0;
    }
    if (!strcmp(argv[1], "heap")) {
        if (argc != 3) return 2;
        StoreHeap heap;
        heap.heap_bytes = strtoull(argv[2], nullptr, 10);
        std::map<uint64_t, pmc_extent> live;
        char op;
        uint64_t v;
        while (scanf(" %c %" SCNu64, &op, &v) == 2) {
            if (op == 'a') {
                const uint32_t cap = StoreHeap::extent_size(v);
                uint64_t off = 0;
                const bool ok = heap.alloc(cap, &off);
                if (ok) {
                    if (live.count(off)) return 3; // a live extent handed out again
                    live[off] = pmc_extent{off, cap, (uint32_t)v, 0, 1};
                }
                printf("{\"ok\": %d, \"off\": %" PRIu64 ", \"cap\": %u, \"used\": %" PRIu64 ", \"reserved\": %" PRIu64 "}\n",
                       ok ? 1 : 0, ok ? off : 0, cap, heap.used, heap.bump);
            } else if (op == 'r') {
                auto it = live.find(v);
                if (it == live.end()) return 3;
                heap.release(it->second);
                if (it->second.flags != 0) return 3;
                heap.release(it->second); // an extent that is not live: nothing
                live.erase(it);
                printf("{\"used\": %" PRIu64 ", \"reserved\": %" PRIu64 "}\n", heap.used, heap.bump);
            } else {
                return 2;
            }
        }
        return 0;
    }
    return 2;
}

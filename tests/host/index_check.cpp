// index_check.cpp -- the member index's host arithmetic (csrc/pmc_plan.hpp idx_plan, idx_parse), for
// tests/test_host_index.py.  Plain C++ with no HIP in it; the test builds it with the address and
// undefined-behaviour sanitizers and runs it directly.
//
//   index_check plan <C> <len> ...      one JSON object per length: {"len", "indexed", "K", "hdr"}
//   index_check parse <hex bytes> ...   one JSON object per byte string: {"ok", "chunk", "K", "isize", "hdr"}
//                                       (each string is parsed in a heap buffer of exactly its length)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../poor-man-s-cache_amd/csrc/pmc_plan.hpp"

using namespace pmc;

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "plan")) {
        if (argc < 4) return 2;
        const uint32_t C = (uint32_t)strtoull(argv[2], nullptr, 10);
        for (int k = 3; k < argc; k++) {
            const uint64_t len = strtoull(argv[k], nullptr, 10);
            const IdxPlan p = idx_plan(len, C);
            printf("{\"len\": %" PRIu64 ", \"indexed\": %d, \"K\": %u, \"hdr\": %u}\n", len, p.indexed ? 1 : 0, p.K, p.hdr);
        }
        return 0;
    }
    if (!strcmp(argv[1], "parse")) {
        for (int k = 2; k < argc; k++) {
            const size_t n = strlen(argv[k]) / 2;
            uint8_t *m = (uint8_t *)malloc(n ? n : 1); // exactly n bytes: a read past them is the sanitizer's
            if (!m) return 3;
            for (size_t i = 0; i < n; i++) {
                const int hi = hexval(argv[k][2 * i]), lo = hexval(argv[k][2 * i + 1]);
                if (hi < 0 || lo < 0) return 2;
                m[i] = (uint8_t)(hi << 4 | lo);
            }
            uint32_t lg = 0, K = 0, isz = 0, hdr = 0;
            const bool ok = idx_parse((const uint8_t *)m, n, &lg, &K, &isz, &hdr);
            printf("{\"ok\": %d, \"chunk\": %u, \"K\": %u, \"isize\": %u, \"hdr\": %u}\n", ok ? 1 : 0, ok ? 1u << lg : 0u, K,
                   isz, hdr);
            free(m);
        }
        return 0;
    }
    return 2;
}

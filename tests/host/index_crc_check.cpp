// index_crc_check.cpp -- the chunk CRCs' host arithmetic (csrc/pmc_plan.hpp idx_plan with the CRC switch,
// idx_crc_parse), for tests/test_host_index_crc.py.  Plain C++ with no HIP in it; the test builds it with the
// address and undefined-behaviour sanitizers and runs it directly.
//
//   index_crc_check plan <C> <crc 0|1> <len> ...   one JSON object per length:
//                                                  {"len", "indexed", "K", "hdr", "crcs", "crc_at"}
//   index_crc_check parse <hex bytes> ...          one JSON object per byte string: {"ok", "K", "crc_at", "crcs"}
//                                                  (each string is parsed in a heap buffer of exactly its length)
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
        if (argc < 5) return 2;
        const uint32_t C = (uint32_t)strtoull(argv[2], nullptr, 10);
        const bool crc = strtoull(argv[3], nullptr, 10) != 0;
        for (int k = 4; k < argc; k++) {
            const uint64_t len = strtoull(argv[k], nullptr, 10);
            const IdxPlan p = idx_plan(len, C, crc);
            printf("{\"len\": %" PRIu64 ", \"indexed\": %d, \"K\": %u, \"hdr\": %u, \"crcs\": %d, \"crc_at\": %u}\n", len,
                   p.indexed ? 1 : 0, p.K, p.hdr, p.crcs ? 1 : 0, p.crc_at);
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
            uint32_t K = 0, at = 0;
            const bool ok = idx_crc_parse((const uint8_t *)m, n, &K, &at);
            printf("{\"ok\": %d, \"K\": %u, \"crc_at\": %u, \"crcs\": [", ok ? 1 : 0, ok ? K : 0u, ok ? at : 0u);
            for (uint32_t j = 0; ok && j < K; j++) {
                const uint8_t *e = m + at + 4 * j;
                printf("%s%u", j ? ", " : "", (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24);
            }
            printf("]}\n");
            free(m);
        }
        return 0;
    }
    return 2;
}

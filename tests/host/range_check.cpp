// range_check.cpp -- the host arithmetic of ranged reads (csrc/pmc_plan.hpp range_of, plan_range), for
// tests/test_host_range.py.  Plain C++ with no HIP in it; the test builds it with the address and
// undefined-behaviour sanitizers and runs it directly.
//
//   range_check of <isize> <lg> <off> <len> ...      one JSON object per (isize, lg, off, len)
//   range_check plan <cus> <per_cu> <n> ...          one JSON object per n
//   range_check budget                               the constants
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../poor-man-s-cache_amd/csrc/pmc_plan.hpp"

using namespace pmc;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "of")) {
        if ((argc - 2) % 4) return 2;
        for (int k = 2; k + 3 < argc; k += 4) {
            const uint32_t isize = (uint32_t)strtoull(argv[k], nullptr, 10), lg = (uint32_t)strtoull(argv[k + 1], nullptr, 10);
            const uint32_t off = (uint32_t)strtoull(argv[k + 2], nullptr, 10), len = (uint32_t)strtoull(argv[k + 3], nullptr, 10);
            const RangeOf r = range_of(isize, lg, off, len);
            printf("{\"o\": %u, \"L\": %u, \"k0\": %u, \"items\": %u}\n", r.o, r.L, r.k0, r.items);
        }
        return 0;
    }
    if (!strcmp(argv[1], "plan")) {
        if (argc < 5) return 2;
        const uint64_t cus = strtoull(argv[2], nullptr, 10), per_cu = strtoull(argv[3], nullptr, 10);
        for (int k = 4; k < argc; k++) {
            const uint64_t n = strtoull(argv[k], nullptr, 10);
            const RangePlan P = plan_range(n, cus, per_cu, 1024);
            printf("{\"n\": %" PRIu64 ", \"mb\": %u, \"cb\": %u, \"row_per_request\": %d, \"rows\": %" PRIu64
                   ", \"cnt\": %" PRIu64 ", \"fail\": %" PRIu64 ", \"pre\": %" PRIu64 ", \"bsum\": %" PRIu64
                   ", \"total\": %" PRIu64 ", \"rows_off\": %" PRIu64 ", \"edge_bytes\": %" PRIu64 ", \"bytes\": %" PRIu64
                   "}\n",
                   n, P.mb, P.cb, P.row_per_request ? 1 : 0, P.rows, P.idx.cnt, P.idx.fail, P.idx.pre, P.idx.bsum,
                   P.idx.total, P.rows_off, P.edge_bytes, P.bytes);
        }
        return 0;
    }
    if (!strcmp(argv[1], "budget")) {
        printf("{\"log2_max\": %u, \"row_bytes\": %" PRIu64 ", \"budget\": %" PRIu64 ", \"fallback\": %" PRIu64 "}\n",
               kRangeLog2Max, kRangeRowBytes, kRangeScratchBudget, kRangeFallbackBudget);
        return 0;
    }
    return 2;
}

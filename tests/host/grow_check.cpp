// grow_check.cpp -- the host arithmetic of growing writes (csrc/pmc_plan.hpp grow_of), for tests/test_host_grow.py.
// Plain C++ with no HIP in it; the test builds it with the address and undefined-behaviour sanitizers and runs it
// directly.
//
//   grow_check of <isize> <lg> <off> <len> ...      one JSON object per (isize, lg, off, len)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../poor-man-s-cache_amd/csrc/pmc_plan.hpp"

using namespace pmc;

int main(int argc, char **argv) {
    if (argc < 2 || strcmp(argv[1], "of") || (argc - 2) % 4) return 2;
    for (int k = 2; k + 3 < argc; k += 4) {
        const uint32_t isize = (uint32_t)strtoull(argv[k], nullptr, 10), lg = (uint32_t)strtoull(argv[k + 1], nullptr, 10);
        const uint32_t off = (uint32_t)strtoull(argv[k + 2], nullptr, 10), len = (uint32_t)strtoull(argv[k + 3], nullptr, 10);
        const GrowOf g = grow_of(isize, lg, off, len);
        printf("{\"verdict\": %u, \"grows\": %d, \"S2\": %u, \"K2\": %u, \"a\": %u, \"b\": %u, \"items\": %u, \"edge_a\": %d, "
               "\"edge_b\": %d}\n",
               g.verdict, g.grows ? 1 : 0, g.S2, g.K2, g.a, g.b, g.items, g.edge_a ? 1 : 0, g.edge_b ? 1 : 0);
    }
    return 0;
}

// patch_check.cpp -- the host arithmetic of ranged writes (csrc/pmc_plan.hpp patch_of, crc_fold_host, plan_patch,
// plan_patch_round), for tests/test_host_patch.py.  Plain C++ with no HIP in it; the test builds it with the
// address and undefined-behaviour sanitizers and runs it directly.
//
//   patch_check of <isize> <lg> <off> <len> ...      one JSON object per (isize, lg, off, len)
//   patch_check fold <isize> <lg> <crc> ...          the fold of the K = ceil(isize / 2^lg) entries
//   patch_check plan <cus> <n> ...                   one JSON object per n
//   patch_check round <cus> <items> ...              one JSON object per items
//   patch_check budget                               the constants
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
            const PatchOf p = patch_of(isize, lg, off, len);
            printf("{\"ok\": %d, \"a\": %u, \"b\": %u, \"items\": %u, \"edge_a\": %d, \"edge_b\": %d}\n", p.ok ? 1 : 0, p.a,
                   p.b, p.items, p.edge_a ? 1 : 0, p.edge_b ? 1 : 0);
        }
        return 0;
    }
    if (!strcmp(argv[1], "fold")) {
        if (argc < 5) return 2;
        const uint32_t isize = (uint32_t)strtoull(argv[2], nullptr, 10), lg = (uint32_t)strtoull(argv[3], nullptr, 10);
        const uint32_t K = (uint32_t)(((uint64_t)isize + (1u << lg) - 1) >> lg);
        if ((uint32_t)(argc - 4) != K) return 2;
        std::vector<uint32_t> e(K);
        for (uint32_t k = 0; k < K; k++) e[k] = (uint32_t)strtoull(argv[4 + k], nullptr, 10);
        printf("{\"K\": %u, \"crc\": %u}\n", K, crc_fold_host(e.data(), K, isize, lg));
        return 0;
    }
    if (!strcmp(argv[1], "plan")) {
        if (argc < 4) return 2;
        const uint64_t cus = strtoull(argv[2], nullptr, 10);
        for (int k = 3; k < argc; k++) {
            const uint64_t n = strtoull(argv[k], nullptr, 10);
            const PatchPlan P = plan_patch(n, cus, 1024);
            printf("{\"n\": %" PRIu64 ", \"mb\": %u, \"cnt\": %" PRIu64 ", \"ka\": %" PRIu64 ", \"fail\": %" PRIu64
                   ", \"pfail\": %" PRIu64 ", \"lv_val\": %" PRIu64 ", \"seg0\": %" PRIu64 ", \"rlen\": %" PRIu64
                   ", \"roff\": %" PRIu64 ", \"pre\": %" PRIu64 ", \"bsum\": %" PRIu64 ", \"total\": %" PRIu64
                   ", \"bytes\": %" PRIu64 "}\n",
                   n, P.mb, P.cnt, P.ka, P.fail, P.pfail, P.lv_val, P.seg0, P.rlen, P.roff, P.pre, P.bsum, P.total, P.bytes);
        }
        return 0;
    }
    if (!strcmp(argv[1], "round")) {
        if (argc < 4) return 2;
        const uint64_t cus = strtoull(argv[2], nullptr, 10);
        for (int k = 3; k < argc; k++) {
            const uint64_t items = strtoull(argv[k], nullptr, 10);
            const PatchRound R = plan_patch_round(items, cus);
            printf("{\"items\": %" PRIu64 ", \"waves\": %" PRIu64 ", \"stage\": %" PRIu64 ", \"tok\": %" PRIu64
                   ", \"seg_val\": %" PRIu64 ", \"seg_tok0\": %" PRIu64 ", \"seg_tok\": %" PRIu64 ", \"slots\": %" PRIu64
                   ", \"span\": %" PRIu64 ", \"crc\": %" PRIu64 ", \"slabs\": %" PRIu64 ", \"bytes\": %" PRIu64 "}\n",
                   items ? items : 1, R.waves, R.stage, R.tok, R.seg_val, R.seg_tok0, R.seg_tok, R.slots, R.span, R.crc,
                   R.slabs, R.bytes);
        }
        return 0;
    }
    if (!strcmp(argv[1], "budget")) {
        printf("{\"round_chunks\": %" PRIu64 ", \"budget\": %" PRIu64 ", \"slab\": %" PRIu64 ", \"max_waves\": %" PRIu64
               ", \"slot\": %" PRIu64 ", \"slot_bound\": %" PRIu64 ", \"segs\": %u, \"max_chunks\": %u}\n",
               kPatchRoundChunks, kPatchScratchBudget, kPatchSlabBytes, kPatchMaxWaves, kPatchSlotBytes,
               (gzip_bound(kIdxChunk) + 16 + 15) & ~(uint64_t)15, kPatchSegs, kIdxCrcMaxChunks);
        return 0;
    }
    return 2;
}

// dict_train_check.cpp -- dictionary training in plain C++, written from the text of include/pmc_codec.h
// "dictionary training", and the bounds of csrc/pmc_plan.hpp plan_dict_train; for tests/test_host_dict_train.py.
// No HIP in it; the test builds it with the address and undefined-behaviour sanitizers and runs it directly.  Built
// with -O2 and no sanitizer it is the one-thread CPU yardstick of scripts/dict_train_bench.py.
//
//   dict_train_check train <file>          one line per case: the dictionary in hex ("-" for 0 bytes)
//   dict_train_check time <file> <reps>    one line per case: the fastest of <reps> runs, in milliseconds
//   dict_train_check plan <n> <D> <cus> ...  one JSON object per triple, after checking the plan's bounds
// <file>: u32 cases; per case u32 n, u32 D, n x u32 length, then the samples' bytes back to back (little endian).
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../poor-man-s-cache_amd/csrc/pmc_plan.hpp"

using namespace pmc;

struct Case {
    uint32_t D;
    std::vector<uint32_t> len;
    std::vector<uint64_t> off;
    std::vector<uint8_t> bytes;
};

static uint32_t hash_at(const uint8_t *p) {
    uint64_t w = 0;
    for (int k = 7; k >= 0; k--) w = (w << 8) | p[k];
    return (uint32_t)((w * 0x9E3779B185EBCA87ull) >> 44);
}

static std::vector<uint8_t> train(const Case &c) {
    const uint32_t n = (uint32_t)c.len.size(), E = c.D / 64;
    std::vector<uint32_t> freq(1u << 20, 0);
    std::vector<uint16_t> in_window(1u << 20, 0); // how often a hash value lies in the current window
    std::vector<uint32_t> h;
    auto hashes = [&](uint32_t i) {
        const uint32_t len = std::min<uint32_t>(c.len[i], 16382);
        h.clear();
        for (uint32_t p = 0; p + 8 <= len; p++) h.push_back(hash_at(c.bytes.data() + c.off[i] + p));
        return len;
    };
    for (uint32_t i = 0; i < n; i++) {
        hashes(i);
        for (uint32_t x : h) freq[x]++;
    }
    std::vector<std::vector<uint8_t>> segs;
    for (uint32_t e = 0; e < E; e++) {
        uint64_t best = 0;
        uint32_t bi = 0, bq = 0;
        for (uint32_t i = (uint32_t)((uint64_t)e * n / E); i < (uint32_t)(((uint64_t)e + 1) * n / E); i++) {
            const uint32_t len = hashes(i);
            if (len < 64) continue;
            // the window slides: a hash value's count enters the score when it enters the window for the first
            // time, and leaves with its last copy
            uint64_t s = 0;
            auto add = [&](uint32_t x) {
                if (in_window[x]++ == 0) s += freq[x];
            };
            auto drop = [&](uint32_t x) {
                if (--in_window[x] == 0) s -= freq[x];
            };
            for (uint32_t p = 0; p < 56; p++) add(h[p]);
            for (uint32_t q = 0; q + 64 <= len; q++) {
                add(h[q + 56]);
                if (s > best) best = s, bi = i, bq = q; // rising (i, q): strictly greater keeps the lowest
                drop(h[q]);
            }
            for (uint32_t p = len - 64 + 1; p < len - 64 + 1 + 56; p++) drop(h[p]);
        }
        if (best == 0) continue;
        const uint8_t *seg = c.bytes.data() + c.off[bi] + bq;
        for (uint32_t j = 0; j < 57; j++) freq[hash_at(seg + j)] = 0;
        segs.emplace_back(seg, seg + 64);
    }
    std::vector<uint8_t> dict;
    for (size_t k = segs.size(); k-- > 0;) dict.insert(dict.end(), segs[k].begin(), segs[k].end());
    return dict;
}

static bool read_cases(const char *path, std::vector<Case> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint32_t cases = 0;
    bool ok = fread(&cases, 4, 1, f) == 1;
    for (uint32_t k = 0; ok && k < cases; k++) {
        Case c;
        uint32_t n = 0;
        ok = fread(&n, 4, 1, f) == 1 && fread(&c.D, 4, 1, f) == 1 && dict_train_args_ok(n, c.D);
        if (!ok) break;
        c.len.resize(n);
        ok = fread(c.len.data(), 4, n, f) == n;
        uint64_t total = 0;
        for (uint32_t i = 0; ok && i < n; i++) {
            c.off.push_back(total);
            total += c.len[i];
        }
        c.bytes.resize(total + 1);
        ok = ok && fread(c.bytes.data(), 1, total, f) == total;
        out.push_back(std::move(c));
    }
    fclose(f);
    return ok;
}

static int plan(int argc, char **argv) {
    if ((argc - 2) % 3) return 2;
    for (int k = 2; k + 2 < argc; k += 3) {
        const uint32_t n = (uint32_t)strtoull(argv[k], nullptr, 10), D = (uint32_t)strtoull(argv[k + 1], nullptr, 10);
        const uint64_t cus = strtoull(argv[k + 2], nullptr, 10);
        if (!dict_train_args_ok(n, D)) {
            printf("{\"ok\": 0}\n");
            continue;
        }
        const DictTrainPlan P = plan_dict_train(n, D, cus);
        // the epochs partition [0, n) in order; no launch has more blocks than slots or than samples; the regions
        // lie apart, in order, within the stated bound
        uint32_t at = 0, most = 0;
        bool fine = P.E == D / 64 && P.count_blocks >= 1 && P.count_blocks <= n && P.max_blocks >= 1;
        for (uint32_t e = 0; e < P.E; e++) {
            fine = fine && P.lo(e) == at && P.hi(e) >= at && P.blocks(e) <= P.hi(e) - P.lo(e) &&
                   P.blocks(e) <= P.max_blocks && (P.blocks(e) > 0) == (P.hi(e) > P.lo(e));
            at = P.hi(e);
            most = std::max(most, P.blocks(e));
        }
        fine = fine && at == n && most == P.max_blocks;
        fine = fine && P.table == 0 && P.nsel == (4ull << 20) && P.slots >= P.nsel + 4 &&
               P.rows >= P.slots + 16ull * P.max_blocks && P.rows % 256 == 0 && P.bytes == P.rows + 64ull * P.E &&
               P.bytes <= (4ull << 20) + 512 + 16ull * kTrainWavesPerCu * std::max<uint64_t>(1, cus) + 8192;
        printf("{\"ok\": 1, \"fine\": %d, \"E\": %u, \"count_blocks\": %u, \"max_blocks\": %u, \"bytes\": %" PRIu64 "}\n",
               fine ? 1 : 0, P.E, P.count_blocks, P.max_blocks, P.bytes);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return plan(argc, argv);
    if (argc < 3) return 2;
    std::vector<Case> cases;
    if (!read_cases(argv[2], cases)) return 3;
    if (!strcmp(argv[1], "train")) {
        for (const Case &c : cases) {
            const std::vector<uint8_t> d = train(c);
            if (d.empty()) printf("-");
            for (uint8_t b : d) printf("%02x", b);
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "time") && argc == 4) {
        for (const Case &c : cases) {
            double best = 1e30;
            size_t len = 0;
            for (int r = 0; r < atoi(argv[3]); r++) {
                const auto t0 = std::chrono::steady_clock::now();
                len = train(c).size();
                const auto t1 = std::chrono::steady_clock::now();
                best = std::min(best, std::chrono::duration<double, std::milli>(t1 - t0).count());
            }
            printf("{\"n\": %zu, \"D\": %u, \"dict_len\": %zu, \"ms\": %.3f}\n", c.len.size(), c.D, len, best);
        }
        return 0;
    }
    return 2;
}

// plan_check.cpp -- prints the plans of csrc/pmc_plan.hpp as JSON, for tests/test_host_plan.py.
//
//   plan_check lv <fast_seg> <budget> <table file prefix> <index>:<length> ...
//       the rounds of these large values (fast_seg 0: exact level), one JSON object per line; round k's
//       filled host tables are written to <prefix><k>.bin
//   plan_check layout <pcap> <chunk>        the split pipeline's chunk arrays
//   plan_check chunk <n> <budget> <cap>     split_chunk_of and split_value_bytes
//   plan_check route                        one route per input line (the RouteIn fields in order, as
//                                           integers), one JSON object per line
//   plan_check inflate                      one decompress plan per input line (the InflateIn fields in order,
//                                           as integers), one JSON object per line
//   plan_check latency                      inflate_latency of each input line (its arguments in order): 0 or 1
//   plan_check need_hbm                     inflate_need_hbm of each input line (its arguments in order): 0 or 1
//   plan_check host                         the plan and the HostStage of one host-memory call per input line
//   plan_check pinned                       pinned_chunk_of, or the plan and the PinnedSlot of one chunk, per input line
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../poor-man-s-cache_amd/csrc/pmc_plan.hpp"

using namespace pmc;

static uint64_t u64(const char *s) { return strtoull(s, nullptr, 10); }

static int lv(int argc, char **argv) {
    if (argc < 6) return 2;
    const uint32_t fast_seg = (uint32_t)u64(argv[2]);
    const uint64_t budget = u64(argv[3]);
    const std::string prefix = argv[4];
    std::vector<std::pair<uint32_t, uint32_t>> vals;
    for (int k = 5; k < argc; k++) {
        const char *colon = strchr(argv[k], ':');
        if (!colon) return 2;
        vals.push_back({(uint32_t)u64(argv[k]), (uint32_t)u64(colon + 1)});
    }
    std::sort(vals.begin(), vals.end());
    int k = 0;
    for (size_t v0 = 0; v0 < vals.size(); k++) {
        const LvRound r = lv_plan_round(vals.data(), vals.size(), v0, fast_seg, budget);
        std::vector<uint64_t> image((r.tab_bytes + 7) / 8, 0xA5A5A5A5A5A5A5A5ull); // (8-byte aligned; gaps stay 0xA5)
        r.fill((uint8_t *)image.data());
        FILE *f = fopen((prefix + std::to_string(k) + ".bin").c_str(), "wb");
        if (!f || fwrite(image.data(), 1, r.tab_bytes, f) != r.tab_bytes) return 3;
        fclose(f);
        printf("{\"v0\":%zu,\"v1\":%zu,\"nv\":%u,\"nseg\":%" PRIu64 ",\"nch\":%" PRIu64 ",\"P\":%" PRIu64 ",\"tb\":%" PRIu64
               ",\"maxlen\":%" PRIu64,
               r.v0, r.v1, r.nv, r.nseg, r.nch, r.P, r.tb, r.maxlen);
        printf(",\"tab\":[%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 "],\"tab_bytes\":%" PRIu64,
               r.o_val, r.o_pbase, r.o_seg0, r.o_ch0, r.o_seg_val, r.o_seg_tok0, r.o_ch_val, r.tab_bytes);
        printf(",\"scratch\":[%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64
               ",%" PRIu64 "],\"scratch_bytes\":%" PRIu64 "}\n",
               r.b_tmp, r.b_S, r.b_R, r.b_HC, r.b_hist, r.b_tok, r.b_map, r.b_seg_tok, r.b_fail, r.scratch_bytes);
        v0 = r.v1;
    }
    return 0;
}

static int layout(int argc, char **argv) {
    if (argc != 4) return 2;
    const SplitLayout s(u64(argv[2]), u64(argv[3]));
    printf("{\"cT\":%" PRIu64 ",\"cN\":%" PRIu64 ",\"cP\":%" PRIu64 ",\"cG\":%" PRIu64 ",\"cH\":%" PRIu64 ",\"cL\":%" PRIu64
           ",\"cB\":%" PRIu64 ",\"cC\":%" PRIu64 ",\"cD\":%" PRIu64 ",\"cZ\":%" PRIu64 ",\"ord\":%" PRIu64 ",\"obins\":%" PRIu64
           ",\"cQ\":%" PRIu64 ",\"bytes\":%" PRIu64 "}\n",
           s.cT, s.cN, s.cP, s.cG, s.cH, s.cL, s.cB, s.cC, s.cD, s.cZ, s.ord, s.obins, s.cQ, s.bytes());
    return 0;
}

// the integers of a line into v[0 .. want); false unless there are exactly `want`
static bool ints(char *line, long long *v, int want) {
    int got = 0;
    for (char *p = line, *e; got <= want; got++, p = e) {
        const long long x = strtoll(p, &e, 10);
        if (e == p) break;
        if (got < want) v[got] = x;
    }
    return got == want;
}

static int route() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long v[16];
        if (!ints(line, v, 16)) return 2;
        const RouteIn in{(uint64_t)v[0], (uint64_t)v[1], (int)v[2], v[3] != 0, (uint32_t)v[4], (uint64_t)v[5],
                         v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0, (int)v[10], (uint64_t)v[11], (uint64_t)v[12],
                         (uint64_t)v[13], (uint64_t)v[14], (uint64_t)v[15]};
        const Route r = plan_route(in);
        printf("{\"kind\":\"%s\",\"passes\":[", r.kind == Route::kSplit ? "split" : r.kind == Route::kMono ? "mono" : "v1");
        for (int k = 0; k < r.npass; k++)
            printf("%s[%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%d,%d]", k ? "," : "", r.pass[k].lo, r.pass[k].hi, r.pass[k].pcap,
                   (int)r.pass[k].fastp, (int)r.pass[k].dictp);
        printf("],\"lds_cut\":%" PRIu64 ",\"cap\":%" PRIu64 ",\"dict_len\":%u,\"lv\":%d,\"fast_all\":%d,\"hbm_cut\":%" PRIu64
               ",\"gated\":%d,\"rlist\":%d,\"hbm_waves\":%" PRIu64 "}\n",
               r.lds_cut, r.cap, r.dict_len, (int)r.lv, (int)r.fast_all, r.hbm_cut, (int)r.gated, (int)r.rlist, r.hbm_waves);
    }
    return 0;
}

static int inflate() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long v[16];
        if (!ints(line, v, 16)) return 2;
        const InflateIn in{(uint64_t)v[0], (uint64_t)v[1], (uint64_t)v[2], v[3] != 0, v[4] != 0, (uint32_t)v[5],
                           v[6] != 0, v[7] != 0, v[8] != 0, (uint64_t)v[9], (uint64_t)v[10], (uint64_t)v[11],
                           (uint64_t)v[12], (uint64_t)v[13], (uint64_t)v[14], (uint64_t)v[15]};
        const InflatePlan p = plan_inflate(in);
        printf("{\"lane_route\":%d,\"chunk_pass\":%d,\"chunk_all\":%d,\"order\":%d,\"rec\":%d,\"multi_pass\":%d,\"verify\":%d"
               ",\"dict_second\":%d,\"hbm\":%d,\"retry_only\":%d,\"count_retried\":%d",
               (int)p.lane_route, (int)p.chunk_pass, (int)p.chunk_all, (int)p.order, (int)p.rec, (int)p.multi_pass,
               (int)p.verify, (int)p.dict_second, (int)p.hbm, (int)p.retry_only, (int)p.count_retried);
        printf(",\"ob\":%u,\"lb\":%u,\"out1k\":%d,\"rstride\":%u,\"G\":%u,\"rb\":%u,\"rec_max_out\":%u,\"VG\":%u,\"vb\":%u"
               ",\"mb\":%u,\"cb\":%u,\"hbm_waves\":%" PRIu64 ",\"hbm_blocks\":%u",
               p.ob, p.lb, (int)p.out1k, p.rstride, p.G, p.rb, p.rec_max_out, p.VG, p.vb, p.mb, p.cb, p.hbm_waves, p.hbm_blocks);
        printf(",\"crcx\":%" PRIu64 ",\"order_bytes\":%" PRIu64 ",\"recs\":%" PRIu64 ",\"bigl\":%" PRIu64, p.crcx_bytes,
               p.order_bytes, p.recs_bytes, p.bigl_bytes);
        printf(",\"idx\":{\"cnt\":%" PRIu64 ",\"fail\":%" PRIu64 ",\"pre\":%" PRIu64 ",\"bsum\":%" PRIu64 ",\"total\":%" PRIu64
               ",\"bytes\":%" PRIu64 "}",
               p.idx.cnt, p.idx.fail, p.idx.pre, p.idx.bsum, p.idx.total, p.idx.bytes);
        printf(",\"out_cap\":%" PRIu64 ",\"lds_max_in\":%" PRIu64 ",\"dict_out\":%u", p.out_cap, p.lds_max_in, p.dict_out);
        printf(",\"second\":{\"lds_max_out\":%" PRIu64 ",\"lds_max_in\":%" PRIu64 ",\"dict_out\":%u,\"first_img\":%u"
               ",\"first_in\":%u}}\n",
               p.second.lds_max_out, p.second.lds_max_in, p.second.dict_out, p.second.first_img, p.second.first_in);
    }
    return 0;
}

// every integer of a line
static std::vector<uint64_t> all_ints(const std::string &line) {
    std::vector<uint64_t> v;
    for (const char *p = line.c_str();;) {
        char *e;
        const uint64_t x = strtoull(p, &e, 10);
        if (e == p) return v;
        v.push_back(x);
        p = e;
    }
}

// compress level lane_order_ok force_pipeline cus lat_batch lat_max_len out_limit, then runs of values as
// count src_len dst_cap
static int host() {
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        const std::vector<uint64_t> v = all_ints(buf);
        if (v.size() < 11 || (v.size() - 8) % 3) return 2;
        std::vector<uint32_t> slen, dcap;
        for (size_t k = 8; k < v.size(); k += 3) {
            slen.insert(slen.end(), v[k], (uint32_t)v[k + 1]);
            dcap.insert(dcap.end(), v[k], (uint32_t)v[k + 2]);
        }
        const uint32_t n = (uint32_t)slen.size();
        const HostBatchPlan p = plan_host_batch({v[0] != 0, n, slen.data(), dcap.data(), v[4], level_is_fast((int)v[1]),
                                                 v[2] != 0, v[5], v[6], v[7], v[3] != 0});
        const HostStage L(n, p.in_bytes, p.out_bytes);
        printf("{\"in_bytes\":%" PRIu64 ",\"out_bytes\":%" PRIu64 ",\"max_len\":%" PRIu64 ",\"max_in\":%" PRIu64
               ",\"latency\":%d,\"need_hbm\":%d,\"path\":%d",
               p.in_bytes, p.out_bytes, p.max_len, p.max_in, (int)p.latency, (int)p.need_hbm, p.path);
        printf(",\"soff\":%" PRIu64 ",\"doff\":%" PRIu64 ",\"slen\":%" PRIu64 ",\"dcap\":%" PRIu64 ",\"src\":%" PRIu64
               ",\"dlen\":%" PRIu64 ",\"rc\":%" PRIu64 ",\"dst\":%" PRIu64 ",\"down\":%" PRIu64 ",\"up\":%" PRIu64
               ",\"bytes\":%" PRIu64,
               L.soff.off, L.doff.off, L.slen.off, L.dcap.off, L.src.off, L.dlen.off, L.rc.off, L.dst.off, L.down, L.up,
               L.bytes());
        // the arrays HostStage::fill writes (it touches nothing behind them, so a buffer up to `src` will do)
        std::vector<uint64_t> image(L.src.off / 8);
        const HostStage F(n, p.in_bytes, p.out_bytes, image.data());
        F.fill(slen.data(), dcap.data());
        bool same = true;
        for (uint32_t i = 0; i < n; i++) same = same && F.slen.h[i] == slen[i] && F.dcap.h[i] == dcap[i];
        printf(",\"lens_copied\":%d,\"soff_v\":[", (int)same);
        for (uint32_t i = 0; i < n && i < 8; i++) printf("%s%" PRIu64, i ? "," : "", F.soff.h[i]);
        printf("],\"doff_v\":[");
        for (uint32_t i = 0; i < n && i < 8; i++) printf("%s%" PRIu64, i ? "," : "", F.doff.h[i]);
        printf("],\"soff_last\":%" PRIu64 ",\"doff_last\":%" PRIu64 "}\n", F.soff.h[n - 1], F.doff.h[n - 1]);
    }
    return 0;
}

// "n chunk": pinned_chunk_of; "packed a m", then src_off src_len dst_off dst_cap of every value of the batch:
// the plan and the device slot of the chunk [a, a + m)
static int pinned() {
    static char buf[1 << 20];
    while (fgets(buf, sizeof buf, stdin)) {
        const std::vector<uint64_t> v = all_ints(buf);
        if (v.size() == 2) {
            const PinnedChunks c = pinned_chunk_of((uint32_t)v[0], (uint32_t)v[1]);
            printf("{\"chunk\":%u,\"nchunks\":%u}\n", c.chunk, c.nchunks);
            continue;
        }
        if (v.size() < 7 || (v.size() - 3) % 4) return 2;
        std::vector<uint64_t> soff, doff;
        std::vector<uint32_t> slen, dcap;
        for (size_t k = 3; k < v.size(); k += 4) {
            soff.push_back(v[k]);
            slen.push_back((uint32_t)v[k + 1]);
            doff.push_back(v[k + 2]);
            dcap.push_back((uint32_t)v[k + 3]);
        }
        const uint32_t a = (uint32_t)v[1], m = (uint32_t)v[2];
        if (m == 0 || (uint64_t)a + m > soff.size()) return 2;
        const PinnedChunk k = plan_pinned_chunk(soff.data(), slen.data(), v[0] ? nullptr : doff.data(), dcap.data(), a, m);
        const PinnedSlot L(m, k);
        printf("{\"sb\":%" PRIu64 ",\"se\":%" PRIu64 ",\"db\":%" PRIu64 ",\"de\":%" PRIu64 ",\"compact\":%d,\"nb\":%u", k.sb,
               k.se, k.db, k.de, (int)k.compact, k.nb);
        printf(",\"soff\":%" PRIu64 ",\"doff\":%" PRIu64 ",\"poff\":%" PRIu64 ",\"slen\":%" PRIu64 ",\"dcap\":%" PRIu64
               ",\"dlen\":%" PRIu64 ",\"rc\":%" PRIu64 ",\"bsum\":%" PRIu64 ",\"meta\":%" PRIu64 ",\"src\":%" PRIu64
               ",\"dst\":%" PRIu64 ",\"packed\":%" PRIu64 ",\"need\":%" PRIu64 "}\n",
               L.soff.off, L.doff.off, L.poff.off, L.slen.off, L.dcap.off, L.dlen.off, L.rc.off, L.bsum.off, L.meta,
               L.src.off, L.dst.off, L.packed.off, L.need);
    }
    return 0;
}

// inflate_latency (8 arguments) or inflate_need_hbm (4) of each input line
static int predicate(int nargs) {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long v[8];
        if (!ints(line, v, nargs)) return 2;
        const bool b = nargs == 8 ? inflate_latency((uint64_t)v[0], (uint64_t)v[1], (uint64_t)v[2], (uint64_t)v[3], (uint64_t)v[4],
                                                    (uint64_t)v[5], v[6] != 0, (uint64_t)v[7])
                                  : inflate_need_hbm(v[0] != 0, (uint64_t)v[1], (uint64_t)v[2], (uint64_t)v[3]);
        printf("%d\n", (int)b);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "lv")) return lv(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "layout")) return layout(argc, argv);
    if (argc == 5 && !strcmp(argv[1], "chunk")) {
        printf("{\"chunk\":%" PRIu64 ",\"value_bytes\":%" PRIu64 "}\n", split_chunk_of(u64(argv[2]), u64(argv[3]), u64(argv[4])),
               split_value_bytes(u64(argv[4])));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "route")) return route();
    if (argc == 2 && !strcmp(argv[1], "inflate")) return inflate();
    if (argc == 2 && !strcmp(argv[1], "latency")) return predicate(8);
    if (argc == 2 && !strcmp(argv[1], "need_hbm")) return predicate(4);
    if (argc == 2 && !strcmp(argv[1], "host")) return host();
    if (argc == 2 && !strcmp(argv[1], "pinned")) return pinned();
    fprintf(stderr, "usage: plan_check lv|layout|chunk|route|inflate|latency|need_hbm|host|pinned ...\n");
    return 2;
}

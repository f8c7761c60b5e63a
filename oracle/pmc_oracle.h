/*
 * pmc_oracle.h -- CPU ORACLE for the value-codec hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this
 * library, and only as the checker.  The product path (poor-man-s-cache_amd/) never
 * links or calls it; it fails loudly when its HIP library is missing.
 *
 * What it restates: the arithmetic behind the reference's GzipCompressor
 * (/root/reference/src/compressor/gzip_compressor.cpp:3-111), which lives entirely in
 * the third-party zlib it links (not vendored under /root/reference; the reference pins
 * no version, Dockerfile:2 `apk add zlib-dev`).  The restatement follows the published
 * zlib 1.2.11 algorithm (deflate.c: deflate_slow / longest_match / fill_window /
 * slide_hash with configuration_table[9] = {32,258,258,4096}; trees.c; inflate.c;
 * crc32.c) with the reference's parameters deflateInit2(9, Z_DEFLATED, 15+16, 8,
 * Z_DEFAULT_STRATEGY) (gzip_compressor.cpp:12) and inflateInit2(15+16)
 * (gzip_compressor.cpp:62).
 *
 * Parity pin: tests/golden/ holds outputs of the reference Compress itself, compiled
 * from /root/reference/src/compressor/gzip_compressor.cpp by oracle/Makefile into
 * oracle/_ref/ (see tests/golden/make_golden.py).  tests/test_oracle.py checks both
 * restatements byte-for-byte against them.
 */
#ifndef PMC_ORACLE_H
#define PMC_ORACLE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Worst-case gzip member size for an input of len bytes (any content, any size). */
size_t oracle_gzip_bound(size_t len);

/* Faithful streaming restatement of zlib 1.2.11 deflate level 9 + gzip wrapper.
 * Returns the number of bytes written to out (capacity >= oracle_gzip_bound(len)). */
size_t oracle_gzip_compress(const uint8_t *in, size_t len, uint8_t *out);

/* Data-parallel-shaped restatement (the decomposition the HIP kernels use):
 * per-position hash -> stable sort by hash -> candidate windows -> serial lazy parse
 * -> per-block Huffman -> bit emit.  Must equal oracle_gzip_compress byte for byte. */
size_t oracle_gzip_compress_dp(const uint8_t *in, size_t len, uint8_t *out);

/* gzip-only inflate with zlib 1.2.11 inflateInit2(31) validation rules.
 * Returns 0 (Z_STREAM_END reached), -3 (Z_DATA_ERROR) or -5 (Z_BUF_ERROR: truncated
 * input -- the reference loops forever here; this is the documented
 * divergence), or ORACLE_E_CAPACITY (-101) when the stream decodes past out_cap: output beyond
 * out_cap is counted but not stored, *out_len receives the decoded size and the caller retries
 * with that capacity (the reference grows its buffer instead, gzip_compressor.cpp:71-77, so
 * capacity is never a verdict).  Bytes after the first member's trailer are ignored
 * (gzip_compressor.cpp:96 stops at Z_STREAM_END). */
#define ORACLE_E_CAPACITY (-101)
int oracle_gzip_decompress(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                           size_t *out_len);

uint32_t oracle_crc32(uint32_t crc, const uint8_t *p, size_t n);

/* Instrumentation for DESIGN.md: counts from the last oracle_gzip_compress_dp call. */
typedef struct {
    uint64_t positions, searches, candidates, literals, matches, blocks;
    uint64_t stored_blocks, fixed_blocks, dynamic_blocks;
} oracle_stats;
void oracle_get_stats(oracle_stats *s);

/* Block facts: what trees.c computes on the way to each block of the last oracle_gzip_compress or
 * oracle_gzip_compress_dp call.  Index 0 is the literal/length tree, 1 the distance tree, 2 the bit-length
 * tree.  leaves: symbols of non-zero frequency before build_tree forces a code (leaves[0] is the heap a
 * lane of the trees kernel must hold); overflow: gen_bitlen's count of nodes cut to max_length;
 * depth_ties: pqdownheap comparisons of two entries of equal frequency and unequal depth (the ones
 * `smaller` decides by depth); opt_len and static_len in bits as _tr_flush_block compares them (tree
 * header included), stored_len in bytes; type 0 stored, 1 fixed, 2 dynamic; symbols: literals + matches.
 * Returns the number of blocks of that call and writes the first min(cap, blocks, 64) of them. */
typedef struct {
    uint32_t leaves[3], overflow[3], depth_ties[3];
    int32_t max_code[3], max_blindex;
    uint32_t type, symbols;
    uint64_t opt_len, static_len, stored_len;
} oracle_block_facts;
size_t oracle_get_block_facts(oracle_block_facts *out, size_t cap);

/* Search log: what the last oracle_gzip_compress_dp call (a value of at most ORACLE_LOG_MAX bytes; longer values
 * leave an empty log; the buffers are allocated by the value's length) did, for tests/front_values.py.  One oracle_search_rec per longest_match call of the lazy
 * parse: the position, prev_length, the candidates examined, the winner (the longest candidate, nearest first:
 * win_ord is its 0-based place in the chain, 0xFFFFFFFF with no candidate; win_len may be <= prev_length, in which
 * case the parse ignores it), first_len the nearest candidate's common prefix (capped at nice), how the walk
 * ended, and whether a candidate of the same hash and other leading bytes was examined.  One oracle_token_rec per
 * symbol: len 0 is a literal whose byte is dist.  Both return the number of records of the call and write the
 * first min(cap, records). */
#define ORACLE_LOG_MAX (1u << 20)
enum { ORACLE_END_HASH = 0,  /* the entry below the chain has another hash */
       ORACLE_END_START,     /* the chain reached the start of the sorted array */
       ORACLE_END_NIL,       /* ... position 0 (or the window base), which zlib reads as NIL */
       ORACLE_END_CAP4096, ORACLE_END_CAP1024, ORACLE_END_NICE, ORACLE_END_DIST };
typedef struct {
    uint32_t pos, prev_length, examined, win_ord, win_len, win_dist, first_len, end, collide;
} oracle_search_rec;
typedef struct { uint32_t pos, len, dist; } oracle_token_rec;
size_t oracle_get_search_log(oracle_search_rec *out, size_t cap);
size_t oracle_get_token_log(oracle_token_rec *out, size_t cap);
/* cnt[p], p <= len - 3: the earlier positions of p's hash, position 0 left out.  Returns len - 2. */
size_t oracle_chain_counts(const uint8_t *in, size_t len, uint32_t *cnt, size_t cap);

/* The dp encoder with exactly one rule altered (never a default; tests define "this value decides rule X" as
 * "the variant's member differs"):
 *   TOO_FAR_GE    a length-3 match is dropped from distance 4096 (zlib: from 4097)
 *   TOO_FAR_4097  ... from 4098
 *   CHAIN_NOCAP   no candidate cap
 *   CAP4096_OFF   no cap of 4096 (the 1024 of prev_length >= 32 stays)
 *   GOOD_OFF      cap 4096 even when prev_length >= 32
 *   GOOD_33       cap 1024 only from prev_length >= 33
 *   TIE_FAR       the farthest candidate of equal length wins
 *   NIL_OK        position 0 is a candidate
 *   LAZY_LT       the pending match is emitted only if match_length < prev_length
 *   LAZY_GE       a match as long as the pending one replaces it (longest_match may return prev_length, and the
 *                 pending match is emitted only if match_length < prev_length): LAZY_LT alone changes nothing,
 *                 because longest_match returns a length above prev_length or none
 *   COLLIDE_FREE  candidates whose three bytes differ do not count towards the cap
 *   FIRST_K       candidates from ordinal arg on are ignored
 *   SKIP_K        exactly the candidate of ordinal arg is ignored (it still counts towards the cap)
 *   NICE_258      nice stays 258 near the end of the value: the compare runs on into the zeros past it, the
 *                 winner is picked by that length and the result clipped to the bytes left
 * Rules only values above one window meet (tests/large_conf_values.py):
 *   MAXDIST_FIRST_LT     the first candidate needs d < MAX_DIST (zlib: d <= MAX_DIST)
 *   MAXDIST_FIRST_32507  the first candidate may lie at d <= MAX_DIST + 1
 *   MAXDIST_LATER_LE     later candidates may lie at d <= MAX_DIST (zlib: d < MAX_DIST)
 *   MAXDIST_LATER_32505  later candidates need d < MAX_DIST - 1
 *   MAX_LAZY_OFF         the search also runs at prev_length == 258
 *   STORED_ANY           tr_flush_block always gets the block's bytes: the window base never forbids a stored block
 *   SLIDE_EARLY          the window base moves when i - B >= W_SIZE + MAX_DIST - 1
 *   SLIDE_LATE           ... when i - B >= W_SIZE + MAX_DIST + 1
 *   SLIDE_NIL_OFF        a candidate at or below the window base is NIL only while the base is 0 */
enum { ORACLE_RULE_ZLIB = 0, ORACLE_RULE_TOO_FAR_GE, ORACLE_RULE_TOO_FAR_4097, ORACLE_RULE_CHAIN_NOCAP,
       ORACLE_RULE_GOOD_OFF, ORACLE_RULE_GOOD_33, ORACLE_RULE_TIE_FAR, ORACLE_RULE_NIL_OK, ORACLE_RULE_LAZY_LT,
       ORACLE_RULE_COLLIDE_FREE, ORACLE_RULE_FIRST_K, ORACLE_RULE_SKIP_K, ORACLE_RULE_NICE_258, ORACLE_RULE_CAP4096_OFF, ORACLE_RULE_LAZY_GE,
       ORACLE_RULE_MAXDIST_FIRST_LT, ORACLE_RULE_MAXDIST_FIRST_32507, ORACLE_RULE_MAXDIST_LATER_LE,
       ORACLE_RULE_MAXDIST_LATER_32505, ORACLE_RULE_MAX_LAZY_OFF, ORACLE_RULE_STORED_ANY, ORACLE_RULE_SLIDE_EARLY,
       ORACLE_RULE_SLIDE_LATE, ORACLE_RULE_SLIDE_NIL_OFF };
size_t oracle_compress_variant(int rule, unsigned arg, const uint8_t *in, size_t len, uint8_t *out);

/* The window base (fill_window's slides so far) at a loop top t of a value of len bytes, as a closed form of t
 * alone; oracle_base_diffs: the loop tops of the last oracle_gzip_compress_dp call at which the base it keeps step
 * by step was another (0 unless the closed form is wrong). */
size_t oracle_window_base(size_t t, size_t len);
uint64_t oracle_base_diffs(void);

/* The speculative parse of the large-value pipeline (csrc/pmc_deflate_large.hip, lv_parse_kernel), stated by the
 * oracle: deflate_slow from a fresh state at `start`, chains over the whole value, up to the first loop top at or
 * past `stop` (stop == len: with deflate_slow's trailing literal).  One oracle_state_rec per loop top at which
 * match_length == 2, so that no match is pending: code 1 with no literal pending, 2 with one, and the tokens
 * emitted so far.  Writes the first min(cap_s, states) states and min(cap_t, tokens) tokens, *ntok receives the
 * token count; returns the number of states.  Leaves the logs of the last compress call alone. */
typedef struct { uint32_t pos, code, ntok; } oracle_state_rec;
size_t oracle_parse_from(const uint8_t *in, size_t len, size_t start, size_t stop, oracle_state_rec *st, size_t cap_s,
                         oracle_token_rec *tk, size_t cap_t, size_t *ntok);

/* splitmix64-based synthetic value generator shared with the GPU generator
 * (SURVEY.md §8d): value i of size V is corpus[off_i : off_i+V],
 * off_i = splitmix64(seed ^ i) mod (corpus_len - V + 1). kind 1 = random [A-Za-z0-9]. */
uint64_t oracle_splitmix64(uint64_t x);
uint64_t oracle_murmur3_x64_128_h1(const uint8_t *data, int len, uint32_t seed);
void oracle_gen_values(const uint8_t *corpus, size_t corpus_len, uint64_t seed, int kind,
                       uint64_t first, uint32_t n, uint32_t vlen, uint8_t *out);
void oracle_gen_values_idx(const uint8_t *corpus, size_t corpus_len, uint64_t seed, int kind,
                           const uint64_t *index, uint32_t n, uint32_t vlen, uint8_t *out);
void oracle_route_keys(uint64_t first, uint64_t n, uint32_t num_shards, uint32_t n_gpus, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif

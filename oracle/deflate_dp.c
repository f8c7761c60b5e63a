/* deflate_dp.c -- CPU ORACLE (test infrastructure only).
 *
 * Data-parallel-shaped restatement of the same zlib 1.2.11 level-9 encoder as
 * deflate_faithful.c, written in the decomposition the HIP kernels use, so each GPU
 * stage has a CPU twin to be diffed against:
 *
 *  1. h(p) = ((b[p]<<10) ^ (b[p+1]<<5) ^ b[p+2]) & 0x7fff for p <= len-3.  With
 *     HASH_SHIFT 5 and 15 hash bits, zlib's rolling UPDATE_HASH depends only on these
 *     three bytes, and every p <= len-3 is inserted (deflate_slow's INSERT_STRING and the
 *     max_insert bound), so the head/prev chain of p is exactly the list of earlier
 *     positions with the same hash, nearest first.
 *  2. A STABLE sort of positions by h turns every chain into a contiguous run walked
 *     backwards: chain(i) = S[rank(i)-1], S[rank(i)-2], ... while the hash matches.
 *  3. longest_match(i, prev_length) (deflate.c) == over the first C candidates
 *     (C = 4096, or 1024 when prev_length >= good_length 32) the NEAREST candidate with the
 *     largest min(LCP, nice), nice = min(258, len-i); it wins only if that exceeds
 *     prev_length.  The first candidate may sit at distance <= MAX_DIST, later ones at
 *     < MAX_DIST (the caller's `strstart - hash_head <= MAX_DIST` vs the loop's
 *     `> limit`), and a candidate at the current window base is NIL (slide_hash).
 *  4. deflate_slow's lazy decision is a cheap serial scan over those search results.
 *  5. Blocks of 16383 symbols go through the trees.c restatement.
 * Window slides (inputs > 65274 B) are tracked as bookkeeping only: they move the NIL
 * position and make a block's bytes unavailable for a stored block. */
#include <stdlib.h>
#include <string.h>
#include "oracle_internal.h"
#include "pmc_oracle.h"

static oracle_stats g_stats;
void oracle_get_stats(oracle_stats *s) { *s = g_stats; }

typedef struct {
    const uint8_t *b;
    size_t len;
    const uint32_t *S;    /* positions sorted stably by hash */
    const uint32_t *rank; /* rank[p] = index of p in S */
    const uint16_t *h;
} dp_ctx;

static unsigned lcp_capped(const dp_ctx *c, size_t i, size_t q, unsigned cap) {
    unsigned l = 0;
    while (l < cap && c->b[i + l] == c->b[q + l]) l++;
    return l;
}

/* Rule variants (oracle_compress_variant): 0 is zlib's rule set, the only one the two compressors use. */
static int g_rule;
static unsigned g_arg;

/* Search log of the last oracle_gzip_compress_dp call (values of at most ORACLE_LOG_MAX bytes), allocated by the
 * value's length: a value of len bytes has at most len searches and len tokens.  The buffers only grow. */
static oracle_search_rec *g_slog;
static oracle_token_rec *g_tlog;
static size_t g_nslog, g_ntlog, g_log_cap;
static int g_log_on;
static uint64_t g_base_diff;

static int log_reserve(size_t len) {
    if (len + 1 > g_log_cap) {
        free(g_slog), free(g_tlog);
        g_log_cap = len + 1;
        g_slog = (oracle_search_rec *)malloc(g_log_cap * sizeof *g_slog);
        g_tlog = (oracle_token_rec *)malloc(g_log_cap * sizeof *g_tlog);
        if (!g_slog || !g_tlog) {
            free(g_slog), free(g_tlog);
            g_slog = NULL, g_tlog = NULL, g_log_cap = 0;
            return 0;
        }
    }
    return 1;
}

size_t oracle_get_search_log(oracle_search_rec *out, size_t cap) {
    size_t n = g_nslog < cap ? g_nslog : cap;
    if (out && n) memcpy(out, g_slog, n * sizeof *out);
    return g_nslog;
}
size_t oracle_get_token_log(oracle_token_rec *out, size_t cap) {
    size_t n = g_ntlog < cap ? g_ntlog : cap;
    if (out && n) memcpy(out, g_tlog, n * sizeof *out);
    return g_ntlog;
}
static void log_token(size_t pos, unsigned len, unsigned dist) {
    if (g_log_on && g_ntlog < g_log_cap) {
        oracle_token_rec *t = &g_tlog[g_ntlog++];
        t->pos = (uint32_t)pos, t->len = len, t->dist = dist;
    }
}

/* The chain of every position of a value, as the sort sees it: cnt[p] = earlier positions of p's hash
 * (position 0, which zlib cannot tell from NIL, not counted), for p <= len - 3.  Returns len - 2 (0 below 3). */
size_t oracle_chain_counts(const uint8_t *in, size_t len, uint32_t *cnt, size_t cap) {
    size_t npos = len >= MIN_MATCH ? len - (MIN_MATCH - 1) : 0;
    uint32_t *seen = (uint32_t *)calloc(HASH_SIZE, sizeof(uint32_t));
    for (size_t p = 0; p < npos && p < cap; p++) {
        unsigned h = ((in[p] << 10) ^ (in[p + 1] << 5) ^ in[p + 2]) & HASH_MASK;
        cnt[p] = seen[h];
        if (p) seen[h]++;
    }
    free(seen);
    return npos;
}

/* Search result for position i: returns the best length (> b0) or 0 if none beats b0. */
static unsigned dp_search(const dp_ctx *c, size_t i, unsigned b0, size_t B, size_t *qbest) {
    unsigned C = b0 >= GOOD_LENGTH ? MAX_CHAIN >> 2 : MAX_CHAIN;
    size_t rk = c->rank[i];
    unsigned nice = (unsigned)((c->len - i) < NICE_LENGTH ? (c->len - i) : NICE_LENGTH);
    unsigned left = nice; /* bytes a match may hold */
    unsigned best = 0, nexam = 0, ncap = 0, best_ord = 0, first_len = 0, collide = 0, end = ORACLE_END_START;
    if (g_rule == ORACLE_RULE_CHAIN_NOCAP) C = 0xFFFFFFFFu;
    if (g_rule == ORACLE_RULE_CAP4096_OFF && C == MAX_CHAIN) C = 0xFFFFFFFFu;
    if (g_rule == ORACLE_RULE_GOOD_OFF) C = MAX_CHAIN;
    if (g_rule == ORACLE_RULE_GOOD_33) C = b0 >= GOOD_LENGTH + 1 ? MAX_CHAIN >> 2 : MAX_CHAIN;
    if (g_rule == ORACLE_RULE_NICE_258) nice = NICE_LENGTH;
    /* the first candidate at a distance of at most first_max, later ones below later_lim */
    size_t first_max = g_rule == ORACLE_RULE_MAXDIST_FIRST_LT ? MAX_DIST - 1
                       : g_rule == ORACLE_RULE_MAXDIST_FIRST_32507 ? MAX_DIST + 1 : MAX_DIST;
    size_t later_lim = g_rule == ORACLE_RULE_MAXDIST_LATER_LE ? MAX_DIST + 1
                       : g_rule == ORACLE_RULE_MAXDIST_LATER_32505 ? MAX_DIST - 1 : MAX_DIST;
    for (size_t k = rk; k-- > 0;) {
        size_t q = c->S[k];
        if (c->h[q] != c->h[i]) { end = ORACLE_END_HASH; break; }
        size_t d = i - q;
        if (g_rule == ORACLE_RULE_NIL_OK ? q < B : g_rule == ORACLE_RULE_SLIDE_NIL_OFF && B > 0 ? 0 : q <= B) {
            end = ORACLE_END_NIL;
            break;
        }
        if (nexam == 0 ? d > first_max : d >= later_lim) { end = ORACLE_END_DIST; break; }
        if (g_rule == ORACLE_RULE_FIRST_K && nexam >= g_arg) { end = ORACLE_END_HASH; break; }
        nexam++;
        if (!(g_rule == ORACLE_RULE_SKIP_K && nexam - 1 == g_arg)) {
            unsigned l = lcp_capped(c, i, q, left);
            if (g_rule == ORACLE_RULE_NICE_258 && l == left) /* the compare runs on: zeros lie past the value */
                while (l < NICE_LENGTH && q + l < c->len && c->b[q + l] == 0) l++;
            if (nexam == 1) first_len = l;
            if (l < MIN_MATCH) collide = 1;
            if (!(g_rule == ORACLE_RULE_COLLIDE_FREE && l < MIN_MATCH)) ncap++;
            if (g_rule == ORACLE_RULE_TIE_FAR ? l >= best : l > best) { /* strictly longer: nearest wins ties */
                best = l;
                best_ord = nexam - 1;
                *qbest = q;
                if (l >= nice) { end = ORACLE_END_NICE; break; }
            }
        } else
            ncap++;
        if (ncap == C) { end = C != MAX_CHAIN >> 2 ? ORACLE_END_CAP4096 : ORACLE_END_CAP1024; break; }
    }
    if (best > left) best = left;
    g_stats.searches++;
    g_stats.candidates += nexam;
    if (g_log_on && g_nslog < g_log_cap) {
        oracle_search_rec *r = &g_slog[g_nslog++];
        r->pos = (uint32_t)i, r->prev_length = b0, r->examined = nexam, r->end = end, r->collide = collide;
        r->first_len = first_len;
        r->win_ord = best ? best_ord : 0xFFFFFFFFu;
        r->win_len = best, r->win_dist = best ? (uint32_t)(i - *qbest) : 0;
    }
    if (g_rule == ORACLE_RULE_LAZY_GE) return best >= b0 && best >= MIN_MATCH ? best : 0;
    return best > b0 ? best : 0;
}

size_t oracle_compress_variant(int rule, unsigned arg, const uint8_t *in, size_t len, uint8_t *out) {
    g_rule = rule, g_arg = arg;
    size_t n = oracle_gzip_compress_dp(in, len, out);
    g_rule = 0, g_arg = 0;
    return n;
}

/* stage 1+2: hashes and a stable counting sort by hash */
typedef struct { uint16_t *h; uint32_t *S, *rank; } dp_sort;
static dp_ctx dp_build(const uint8_t *in, size_t len, dp_sort *m) {
    size_t npos = len >= MIN_MATCH ? len - (MIN_MATCH - 1) : 0, p;
    uint32_t *cnt = (uint32_t *)calloc(HASH_SIZE + 1, sizeof(uint32_t));
    m->h = (uint16_t *)malloc((npos + 1) * sizeof(uint16_t));
    m->S = (uint32_t *)malloc((npos + 1) * sizeof(uint32_t));
    m->rank = (uint32_t *)malloc((npos + 1) * sizeof(uint32_t));
    for (p = 0; p < npos; p++) {
        m->h[p] = (uint16_t)(((in[p] << 10) ^ (in[p + 1] << 5) ^ in[p + 2]) & HASH_MASK);
        cnt[m->h[p] + 1]++;
    }
    for (unsigned k = 0; k < HASH_SIZE; k++) cnt[k + 1] += cnt[k];
    for (p = 0; p < npos; p++) {
        uint32_t r = cnt[m->h[p]]++;
        m->S[r] = (uint32_t)p;
        m->rank[p] = r;
    }
    free(cnt);
    dp_ctx c = {in, len, m->S, m->rank, m->h};
    return c;
}
static void dp_sort_free(dp_sort *m) { free(m->h), free(m->S), free(m->rank); }

/* The window base at a loop top t of a value of len bytes, as a closed form of t alone: fill_window runs at a loop
 * top whose lookahead is below MIN_LOOKAHEAD (t + MIN_LOOKAHEAD beyond the window's end, or beyond the value's) and
 * slides when t - base >= W_SIZE + MAX_DIST.  Every earlier loop top lies below t, so it moved the base no
 * further.  oracle_gzip_compress_dp keeps the base step by step and counts the loop tops at which the two differ
 * (oracle_base_diffs). */
size_t oracle_window_base(size_t t, size_t len) {
    size_t B = 0;
    for (;;) {
        size_t wend = len < B + 2 * W_SIZE ? len : B + 2 * W_SIZE;
        if (t - B >= W_SIZE + MAX_DIST && t + MIN_LOOKAHEAD > wend) B += W_SIZE;
        else return B;
    }
}
uint64_t oracle_base_diffs(void) { return g_base_diff; }

size_t oracle_gzip_compress_dp(const uint8_t *in, size_t len, uint8_t *out) {
    tstate *t = (tstate *)malloc(sizeof(tstate));
    dp_sort srt;
    size_t n;
    memset(&g_stats, 0, sizeof(g_stats));
    g_stats.positions = len;
    g_log_on = len <= ORACLE_LOG_MAX && log_reserve(len);
    g_base_diff = 0;
    g_nslog = g_ntlog = 0;
    dp_ctx c = dp_build(in, len, &srt);

    gz_header(out);
    tr_init(t, out);
    t->pending = 10;

    /* stage 3+4: serial lazy parse (deflate_slow) over search results */
    size_t i = 0, B = 0, wend = 0, block_start = 0;
    unsigned match_length = MIN_MATCH - 1, prev_length, match_start = 0, prev_match;
    int match_available = 0, bflush;
    const size_t slide_at = W_SIZE + MAX_DIST - (g_rule == ORACLE_RULE_SLIDE_EARLY) + (g_rule == ORACLE_RULE_SLIDE_LATE);
    const unsigned max_lazy = g_rule == ORACLE_RULE_MAX_LAZY_OFF ? MAX_MATCH + 1 : MAX_LAZY;
#define FLUSH(end, last)                                                             \
    do {                                                                             \
        tr_flush_block(t, block_start >= B || g_rule == ORACLE_RULE_STORED_ANY ? in + block_start : 0, \
                       (uint64_t)((end) - block_start), (last));                     \
        block_start = (end);                                                         \
    } while (0)
    for (;;) {
        if (wend - i < MIN_LOOKAHEAD) { /* fill_window bookkeeping */
            do {
                if (i - B >= slide_at) B += W_SIZE;
                if (wend == len) break;
                wend = len < B + 2 * W_SIZE ? len : B + 2 * W_SIZE;
            } while (wend - i < MIN_LOOKAHEAD && wend < len);
            if (wend == i) break;
        }
        if (g_rule == 0 && B != oracle_window_base(i, len)) g_base_diff++;
        prev_length = match_length, prev_match = match_start;
        match_length = MIN_MATCH - 1;
        if (i + MIN_MATCH <= len && prev_length < max_lazy) {
            size_t q = 0;
            unsigned m = dp_search(&c, i, prev_length, B, &q);
            if (m) {
                match_length = m;
                match_start = (unsigned)q;
                size_t far = g_rule == ORACLE_RULE_TOO_FAR_GE ? TOO_FAR - 1 : g_rule == ORACLE_RULE_TOO_FAR_4097 ? TOO_FAR + 1 : TOO_FAR;
                if (m == MIN_MATCH && i - q > far) match_length = MIN_MATCH - 1;
            }
        }
        if (prev_length >= MIN_MATCH &&
            (g_rule == ORACLE_RULE_LAZY_LT || g_rule == ORACLE_RULE_LAZY_GE ? match_length < prev_length : match_length <= prev_length)) {
            bflush = tr_tally_dist(t, (unsigned)(i - 1 - prev_match), prev_length - MIN_MATCH);
            log_token(i - 1, prev_length, (unsigned)(i - 1 - prev_match));
            g_stats.matches++;
            i += prev_length - 1;
            match_available = 0;
            match_length = MIN_MATCH - 1;
            if (bflush) FLUSH(i, 0);
        } else if (match_available) {
            bflush = tr_tally_lit(t, in[i - 1]);
            log_token(i - 1, 0, in[i - 1]);
            g_stats.literals++;
            if (bflush) FLUSH(i, 0);
            i++;
        } else {
            match_available = 1;
            i++;
        }
    }
    if (match_available) {
        tr_tally_lit(t, in[i - 1]);
        log_token(i - 1, 0, in[i - 1]);
        g_stats.literals++;
    }
    if (g_rule == 0 && B != oracle_window_base(i, len)) g_base_diff++; /* (the last flush's loop top is len) */
    FLUSH(i, 1);
#undef FLUSH
    g_stats.stored_blocks = t->n_stored;
    g_stats.fixed_blocks = t->n_fixed;
    g_stats.dynamic_blocks = t->n_dynamic;
    g_stats.blocks = t->n_stored + t->n_fixed + t->n_dynamic;
    n = t->pending;
    uint32_t crc = oracle_crc32(0, in, len);
    for (int k = 0; k < 4; k++) out[n++] = (uint8_t)(crc >> (8 * k));
    for (int k = 0; k < 4; k++) out[n++] = (uint8_t)((uint64_t)len >> (8 * k));
    free(t);
    dp_sort_free(&srt);
    return n;
}

/* The speculative parse of the large-value pipeline, stated by the oracle: deflate_slow from a fresh state at
 * `start` (no pending match, no pending literal, zero tokens), chains over the whole value, the window base that
 * of a true parse at each loop top (oracle_window_base), on to the first loop top at or past `stop`; with stop ==
 * len the trailing literal is emitted as deflate_slow does.  One state record per loop top at which match_length
 * == 2, so that no match is pending: code 1 with no literal pending, 2 with one.  Writes the first min(cap_s,
 * states) states and min(cap_t, tokens) tokens; *ntok receives the token count.  Returns the number of states.
 * The search and token logs of the last compress call are left alone. */
size_t oracle_parse_from(const uint8_t *in, size_t len, size_t start, size_t stop, oracle_state_rec *st, size_t cap_s,
                         oracle_token_rec *tk, size_t cap_t, size_t *ntok) {
    dp_sort srt;
    dp_ctx c = dp_build(in, len, &srt);
    const int log_was = g_log_on;
    const oracle_stats stats_was = g_stats;
    size_t i = start, ns = 0, nt = 0;
    unsigned ml = MIN_MATCH - 1, pl, ms = 0, pm;
    int avail = 0;
    g_log_on = 0;
    if (stop > len) stop = len;
#define TOKEN(p, l, d)                                                       \
    do {                                                                     \
        if (tk && nt < cap_t) tk[nt].pos = (uint32_t)(p), tk[nt].len = (l), tk[nt].dist = (d); \
        nt++;                                                                \
    } while (0)
    while (i < stop) {
        if (ml == MIN_MATCH - 1) {
            if (st && ns < cap_s) st[ns].pos = (uint32_t)i, st[ns].code = avail ? 2 : 1, st[ns].ntok = (uint32_t)nt;
            ns++;
        }
        pl = ml, pm = ms;
        ml = MIN_MATCH - 1;
        if (i + MIN_MATCH <= len && pl < MAX_LAZY) {
            size_t q = 0;
            unsigned m = dp_search(&c, i, pl, oracle_window_base(i, len), &q);
            if (m) {
                ml = m;
                ms = (unsigned)q;
                if (m == MIN_MATCH && i - q > TOO_FAR) ml = MIN_MATCH - 1;
            }
        }
        if (pl >= MIN_MATCH && ml <= pl) {
            TOKEN(i - 1, pl, (unsigned)(i - 1 - pm));
            i += pl - 1;
            avail = 0;
            ml = MIN_MATCH - 1;
        } else if (avail) {
            TOKEN(i - 1, 0, in[i - 1]);
            i++;
        } else {
            avail = 1;
            i++;
        }
    }
    if (stop == len && avail) TOKEN(i - 1, 0, in[i - 1]);
#undef TOKEN
    if (ntok) *ntok = nt;
    g_log_on = log_was;
    g_stats = stats_was;
    dp_sort_free(&srt);
    return ns;
}

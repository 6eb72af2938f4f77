/* CPU twin of the pairwise identity (hite_amd/csrc/hite_ident.hip, hite_pair_identity).  Test infrastructure: the product
 * imports none of this.  Written for clarity, not speed: a row-by-row dynamic programme over the band with (cost, -matches) tuples.
 *
 * Definition (the same text is in include/hite_gpu.h):
 * Pair p names two intervals, 0-based and half-open, of sequences in one CSR batch of ASCII bytes.
 *  - A = seq[a_id][a_start:a_end].
 *  - B = seq[b_id][b_start:b_end].  It is reverse-complemented when strand[p] != 0.
 *  - Bytes are upper-cased.  Anything outside ACGT is N.
 *  - N matches nothing, not even N.
 *  - m = |A| and n = |B|.  Both may be 0.
 * Cells (i, j), with 0 <= i <= m and 0 <= j <= n, exist only inside the band lo <= j - i <= hi.
 *  - lo = min(0, n - m) - band.
 *  - hi = max(0, n - m) + band.
 *  - band >= 0 is one value per call.
 * A path runs from (0,0) to (m,n) by three kinds of step, all between cells of the band:
 *  - a diagonal step: a match costs 0 and adds one to matches; a mismatch costs 1;
 *  - a step down, cost 1;
 *  - a step right, cost 1.
 * The result of a pair is the lexicographic optimum: the smallest cost, and among the paths of that cost the largest matches.
 * It is a pair of integers.
 *  - It does not depend on any tie order of the implementation.
 *  - The number of alignment columns is cost + matches.
 *  - The identity is matches / (cost + matches).  Only host code forms that ratio.
 * Limits:
 *  - m, n <= 32 767.  This is the aligner's window limit, STAR_MAX_LEN.
 *  - The band width hi - lo + 1 may not exceed HITE_IDENT_MAX_WIDTH = 2048.
 *  - A pair beyond either limit, or with an id or interval outside its sequence, gets cost = -1, matches = 0.  The other pairs of
 *    the call are unaffected.
 *  - n_pair = 0 is a valid call. */
#include <stdint.h>
#include <stdlib.h>

#define TWIN_MAX_LEN 32767
#define TWIN_MAX_WIDTH 2048

typedef struct { int64_t cost, neg_matches; int exists; } cell_t;

static int better(cell_t a, cell_t b) {      /* a exists; is it lexicographically smaller than b? */
    if (!b.exists) return 1;
    if (a.cost != b.cost) return a.cost < b.cost;
    return a.neg_matches < b.neg_matches;
}

static uint8_t fold(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 'a' + 'A');
    return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : (uint8_t)'N';
}
static uint8_t comp(uint8_t c) {
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T': return 'A';
        default: return 'N';
    }
}

/* A (m bytes) against B (n bytes), both folded already; max_width <= 0: no limit on the band width */
static int pair(const uint8_t *A, int64_t m, const uint8_t *B, int64_t n, int64_t band, int64_t max_width, int32_t *cost, int32_t *matches) {
    const int64_t lo = (n - m < 0 ? n - m : 0) - band, hi = (n - m > 0 ? n - m : 0) + band;
    *cost = -1; *matches = 0;
    if (max_width > 0 && hi - lo + 1 > max_width) return 0;
    cell_t *prev = (cell_t *)calloc((size_t)(n + 1), sizeof(cell_t)), *cur = (cell_t *)calloc((size_t)(n + 1), sizeof(cell_t));
    if (!prev || !cur) { free(prev); free(cur); return -1; }
    for (int64_t i = 0; i <= m; i++) {
        /* only the columns of the band are visited (a pair of 32 767 bases has 10^9 cells outside it); the two columns beside them
         * are marked as not existing, since the row buffers are reused */
        const int64_t j0 = i + lo < 0 ? 0 : i + lo, j1 = i + hi > n ? n : i + hi;
        if (j0 - 1 >= 0) cur[j0 - 1].exists = 0;
        if (j1 + 1 <= n) cur[j1 + 1].exists = 0;
        for (int64_t j = j0; j <= j1; j++) {
            cell_t best = {0, 0, 0};
            if (j - i >= lo && j - i <= hi) {
                if (i == 0 && j == 0) best.exists = 1;
                if (i > 0 && j > 0 && prev[j - 1].exists) {         /* diagonal */
                    cell_t c = prev[j - 1];
                    if (A[i - 1] == B[j - 1] && A[i - 1] != 'N') c.neg_matches -= 1; else c.cost += 1;
                    if (better(c, best)) best = c;
                }
                if (i > 0 && prev[j].exists) {                        /* down */
                    cell_t c = prev[j];
                    c.cost += 1;
                    if (better(c, best)) best = c;
                }
                if (j > 0 && cur[j - 1].exists) {                     /* right */
                    cell_t c = cur[j - 1];
                    c.cost += 1;
                    if (better(c, best)) best = c;
                }
            }
            cur[j] = best;
        }
        cell_t *t = prev; prev = cur; cur = t;
    }
    if (prev[n].exists) { *cost = (int32_t)prev[n].cost; *matches = (int32_t)(-prev[n].neg_matches); }
    free(prev); free(cur);
    return 0;
}

/* the twin of hite_pair_identity (same arguments without the context); max_width: TWIN_MAX_WIDTH as the product has it, <= 0 lifts the
 * limit (the tests of the twin itself use bands that cover the whole matrix).  -> 0, or -1 when memory ran out */
int twin_pair_identity(int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int64_t n_pair, const int32_t *a_id,
                       const int64_t *a_start, const int64_t *a_end, const int32_t *b_id, const int64_t *b_start, const int64_t *b_end,
                       const uint8_t *strand, int32_t band, int32_t max_width, int32_t *cost_out, int32_t *match_out) {
    for (int64_t p = 0; p < n_pair; p++) {
        cost_out[p] = -1; match_out[p] = 0;
        if (a_id[p] < 0 || a_id[p] >= n_seq || b_id[p] < 0 || b_id[p] >= n_seq) continue;
        const int64_t la = seq_off[a_id[p] + 1] - seq_off[a_id[p]], lb = seq_off[b_id[p] + 1] - seq_off[b_id[p]];
        if (a_start[p] < 0 || a_end[p] < a_start[p] || a_end[p] > la) continue;
        if (b_start[p] < 0 || b_end[p] < b_start[p] || b_end[p] > lb) continue;
        const int64_t m = a_end[p] - a_start[p], n = b_end[p] - b_start[p];
        if (m > TWIN_MAX_LEN || n > TWIN_MAX_LEN) continue;
        uint8_t *A = (uint8_t *)malloc((size_t)m + 1), *B = (uint8_t *)malloc((size_t)n + 1);
        if (!A || !B) { free(A); free(B); return -1; }
        const uint8_t *sa = seqs + seq_off[a_id[p]] + a_start[p], *sb = seqs + seq_off[b_id[p]] + b_start[p];
        for (int64_t i = 0; i < m; i++) A[i] = fold(sa[i]);
        for (int64_t j = 0; j < n; j++) B[j] = strand[p] ? comp(fold(sb[n - 1 - j])) : fold(sb[j]);
        const int rc = pair(A, m, B, n, band, max_width, &cost_out[p], &match_out[p]);
        free(A); free(B);
        if (rc) return rc;
    }
    return 0;
}

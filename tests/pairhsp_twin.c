/* TEST INFRASTRUCTURE: the fast form of the CPU twin of hite_pair_hsps (tests/pairhsp_twin.py compiles and loads this file; the
 * definition is in include/hite_gpu.h, "local alignments of pairs of intervals", and tests/pairhsp_twin.py states it readably).
 * Plain C, one pair after the other, every step as the definition numbers it; nothing here is shared with the HIP code. */
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_LEN 32768
#define WORD 12
#define MAX_OCC 8
#define BIN_SHIFT 6
#define MIN_VOTES 8
#define MAX_WINDOWS 4
#define BAND_BELOW 32
#define BAND_ABOVE 160
#define S_MATCH 2
#define S_MISMATCH (-4)
#define S_GAP (-5)
#define MIN_SCORE 56
#define MIN_RECT 28
#define MAX_HSPS 12

typedef struct { int32_t score, matches, columns, qs, ss; } Val;      /* score 0: the empty value */
typedef struct { int32_t qs, qe, ss, se, score, matches, columns; } Hsp;

static int code_of(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

/* a better than b: larger score, matches, columns, then smaller q_start, s_start */
static int better(const Val *a, const Val *b) {
    if (a->score != b->score) return a->score > b->score;
    if (a->matches != b->matches) return a->matches > b->matches;
    if (a->columns != b->columns) return a->columns > b->columns;
    if (a->qs != b->qs) return a->qs < b->qs;
    return a->ss < b->ss;
}

static Val cell(Val diag, Val up, Val left, int ca, int cb, int i, int j) {
    const Val empty = {0, 0, 0, 0, 0};
    const int hit = ca == cb && ca < 4;
    Val d = empty, u = empty, l = empty, v;
    if (diag.score == 0) {
        if (hit) { d.score = S_MATCH; d.matches = 1; d.columns = 1; d.qs = i; d.ss = j; }
    } else {
        d = diag; d.score += hit ? S_MATCH : S_MISMATCH; d.matches += hit; d.columns++;
    }
    if (up.score != 0) { u = up; u.score += S_GAP; u.columns++; }
    if (left.score != 0) { l = left; l.score += S_GAP; l.columns++; }
    if (d.score <= 0) d = empty;
    if (u.score <= 0) u = empty;
    if (l.score <= 0) l = empty;
    v = d;
    if (better(&u, &v)) v = u;
    if (better(&l, &v)) v = l;
    return v;
}

/* the best cell of rows r0 .. r1, columns c0 .. c1 (1-based) inside the band dlo <= j - i <= dhi; returns 0 when no cell is positive.
 * A row of the band is an array over x = j - i - dlo: the diagonal neighbour is x of the row before, the one above x + 1, the left x - 1. */
static int align(const uint8_t *q, const uint8_t *s, int64_t dlo, int64_t dhi, int r0, int r1, int c0, int c1, Hsp *out) {
    const int W = (int)(dhi - dlo + 1);
    Val *prev = (Val *)calloc((size_t)W + 2, sizeof(Val)), *cur = (Val *)calloc((size_t)W + 2, sizeof(Val));
    Val best = {0, 0, 0, 0, 0};
    int bi = 0, bj = 0;
    for (int i = r0; i <= r1; i++) {
        memset(cur, 0, ((size_t)W + 2) * sizeof(Val));
        for (int x = 0; x < W; x++) {
            const int64_t j = (int64_t)i + dlo + x;
            if (j < c0 || j > c1) continue;
            /* slots are x + 1: slot 0 and slot W + 1 stay empty */
            const Val v = cell(prev[x + 1], prev[x + 2], cur[x], q[i - 1], s[j - 1], i, (int)j);
            cur[x + 1] = v;
            if (v.score > 0 && better(&v, &best)) { best = v; bi = i; bj = (int)j; }
        }
        Val *t = prev; prev = cur; cur = t;
    }
    free(prev); free(cur);
    if (best.score <= 0) return 0;
    out->qs = best.qs; out->qe = bi; out->ss = best.ss; out->se = bj;
    out->score = best.score; out->matches = best.matches; out->columns = best.columns;
    return 1;
}

/* step 4 alone, on the bytes of two sequences: out[7] = the record of the best cell; returns 0 when no cell is positive */
int twin_align(const uint8_t *qb, int m, const uint8_t *sb, int n, int64_t dlo, int64_t dhi, int r0, int r1, int c0, int c1, int32_t *out) {
    uint8_t *q = (uint8_t *)malloc((size_t)m + 1), *s = (uint8_t *)malloc((size_t)n + 1);
    Hsp h;
    for (int i = 0; i < m; i++) q[i] = (uint8_t)code_of(qb[i]);
    for (int j = 0; j < n; j++) s[j] = (uint8_t)code_of(sb[j]);
    const int ok = align(q, s, dlo, dhi, r0, r1, c0, c1, &h);
    free(q); free(s);
    if (ok) memcpy(out, &h, 7 * sizeof(int32_t));
    return ok;
}

typedef struct { uint32_t word; int32_t pos; } WordAt;
static int by_word(const void *a, const void *b) {
    const WordAt *x = (const WordAt *)a, *y = (const WordAt *)b;
    if (x->word != y->word) return x->word < y->word ? -1 : 1;
    return x->pos < y->pos ? -1 : x->pos > y->pos;
}
/* the word at position i of c (len codes), or -1 */
static int64_t word_at(const uint8_t *c, int len, int i) {
    int64_t w = 0;
    if (i + WORD > len) return -1;
    for (int k = 0; k < WORD; k++) {
        if (c[i + k] > 3) return -1;
        w = w * 4 + c[i + k];
    }
    return w;
}

static int hsp_order(const Hsp *a, const Hsp *b) {      /* a before b */
    if (a->score != b->score) return a->score > b->score;
    if (a->qs != b->qs) return a->qs < b->qs;
    if (a->ss != b->ss) return a->ss < b->ss;
    if (a->qe != b->qe) return a->qe < b->qe;
    return a->se < b->se;
}

/* the records of one pair (codes q[m], s[n]) into out[MAX_HSPS]; returns their number */
static int pair_one(const uint8_t *q, int m, const uint8_t *s, int n, int32_t diag_min, Hsp *out) {
    const int nbin = ((m + n - 2) >> BIN_SHIFT) + 2;
    int32_t *vote = (int32_t *)calloc((size_t)nbin, sizeof(int32_t));
    WordAt *tab = (WordAt *)malloc(((size_t)m + 1) * sizeof(WordAt));
    int nt = 0;
    for (int i = 0; i < m; i++) {
        const int64_t w = word_at(q, m, i);
        if (w >= 0) { tab[nt].word = (uint32_t)w; tab[nt].pos = i; nt++; }
    }
    qsort(tab, (size_t)nt, sizeof(WordAt), by_word);
    for (int j = 0; j < n; j++) {
        const int64_t w = word_at(s, n, j);
        if (w < 0) continue;
        int lo = 0, hi = nt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tab[mid].word < (uint32_t)w) lo = mid + 1; else hi = mid;
        }
        int e = lo;
        while (e < nt && tab[e].word == (uint32_t)w) e++;
        if (e - lo > MAX_OCC) continue;
        for (int k = lo; k < e; k++) {
            const int64_t d = (int64_t)j - tab[k].pos;
            if (d >= diag_min) vote[(d + m - 1) >> BIN_SHIFT]++;
        }
    }
    free(tab);
    int chosen[MAX_WINDOWS], nc = 0;
    for (int t = 0; t < MAX_WINDOWS; t++) {
        int best_b = -1;
        int64_t best_w = 0;
        for (int b = 0; b < nbin - 1; b++) {
            int near = 0;
            for (int k = 0; k < nc; k++)
                if (abs(b - chosen[k]) < 2) near = 1;
            if (near) continue;
            const int64_t w = (int64_t)vote[b] + vote[b + 1];
            if (w >= MIN_VOTES && w > best_w) { best_w = w; best_b = b; }
        }
        if (best_b < 0) break;
        chosen[nc++] = best_b;
    }
    free(vote);
    Hsp found[MAX_HSPS];
    int nf = 0;
    for (int t = 0; t < nc; t++) {
        int64_t dlo = ((int64_t)chosen[t] << BIN_SHIFT) - BAND_BELOW - (m - 1);
        const int64_t dhi = ((int64_t)chosen[t] << BIN_SHIFT) + BAND_ABOVE - 1 - (m - 1);
        if (dlo < diag_min) dlo = diag_min;
        Hsp h, g;
        if (!align(q, s, dlo, dhi, 1, m, 1, n, &h) || h.score < MIN_SCORE) continue;
        found[nf++] = h;
        if (h.qs - 1 >= MIN_RECT && h.ss - 1 >= MIN_RECT && align(q, s, dlo, dhi, 1, h.qs - 1, 1, h.ss - 1, &g) && g.score >= MIN_SCORE)
            found[nf++] = g;
        if (m - h.qe >= MIN_RECT && n - h.se >= MIN_RECT && align(q, s, dlo, dhi, h.qe + 1, m, h.se + 1, n, &g) && g.score >= MIN_SCORE)
            found[nf++] = g;
    }
    /* a stable insertion sort, then the containment rule */
    for (int a = 1; a < nf; a++) {
        const Hsp h = found[a];
        int b = a;
        while (b > 0 && hsp_order(&h, &found[b - 1])) { found[b] = found[b - 1]; b--; }
        found[b] = h;
    }
    int nk = 0;
    for (int a = 0; a < nf; a++) {
        int inside = 0;
        for (int k = 0; k < nk; k++)
            if (out[k].qs <= found[a].qs && found[a].qe <= out[k].qe && out[k].ss <= found[a].ss && found[a].se <= out[k].se) inside = 1;
        if (!inside) out[nk++] = found[a];
    }
    return nk;
}

/* the twin of hite_pair_hsps (same arguments without the context) */
int twin_pair_hsps(int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int64_t n_pair, const int32_t *a_id, const int64_t *a_start,
                   const int64_t *a_end, const int32_t *b_id, const int64_t *b_start, const int64_t *b_end, int32_t diag_min, int64_t cap,
                   int32_t *status, int64_t *first, int32_t *recs, int64_t *n_out) {
    int64_t total = 0;
    for (int64_t p = 0; p < n_pair; p++) {
        first[p] = total;
        status[p] = -1;
        const int64_t ia = a_id[p], ib = b_id[p];
        if (ia < 0 || ia >= n_seq || ib < 0 || ib >= n_seq) continue;
        const int64_t la = seq_off[ia + 1] - seq_off[ia], lb = seq_off[ib + 1] - seq_off[ib];
        if (a_start[p] < 0 || a_end[p] < a_start[p] || a_end[p] > la || b_start[p] < 0 || b_end[p] < b_start[p] || b_end[p] > lb) continue;
        const int64_t m = a_end[p] - a_start[p], n = b_end[p] - b_start[p];
        if (m < 1 || n < 1 || m > MAX_LEN || n > MAX_LEN) continue;
        uint8_t *q = (uint8_t *)malloc((size_t)m), *s = (uint8_t *)malloc((size_t)n);
        for (int64_t i = 0; i < m; i++) q[i] = (uint8_t)code_of(seqs[seq_off[ia] + a_start[p] + i]);
        for (int64_t j = 0; j < n; j++) s[j] = (uint8_t)code_of(seqs[seq_off[ib] + b_start[p] + j]);
        Hsp out[MAX_HSPS];
        const int k = pair_one(q, (int)m, s, (int)n, diag_min, out);
        free(q); free(s);
        status[p] = k;
        for (int h = 0; h < k; h++) {
            if (total + h < cap) memcpy(recs + 7 * (total + h), &out[h], 7 * sizeof(int32_t));
        }
        total += k;
    }
    first[n_pair] = total;
    *n_out = total;
    return total > cap ? -4 : 0;
}

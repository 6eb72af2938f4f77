/* TEST INFRASTRUCTURE: the fast form of the CPU twin of hite_ltr_scan (tests/ltrscan_twin.py compiles and loads this file; the
 * definition is in include/hite_gpu.h, "LTR candidate scan", and tests/ltrscan_twin.py states it readably).  Plain C, one sequence
 * after the other, every step as the definition numbers it; step 4 is align() of tests/pairhsp_twin.c, included as it stands.
 * Nothing here is shared with the HIP code. */
#include "pairhsp_twin.c"

#define LS_WORD 13
#define LS_MAX_OCC 16
#define LS_BIN_SHIFT 6
#define LS_GAP 100
#define LS_MIN_HITS 4
#define LS_BAND_BELOW 96
#define LS_BAND_ABOVE 96
#define LS_EDGE 32
#define LS_MAX_REDO 3
#define LS_MAX_LTR 8192

typedef struct { uint32_t word; int32_t pos; } LsWord;
typedef struct { int32_t bin, i, d; } LsHit;
typedef struct { int32_t f[8]; } LsRec;

static int ls_by_word(const void *a, const void *b) {
    const LsWord *x = (const LsWord *)a, *y = (const LsWord *)b;
    if (x->word != y->word) return x->word < y->word ? -1 : 1;
    return x->pos < y->pos ? -1 : x->pos > y->pos;
}
static int ls_by_bin(const void *a, const void *b) {
    const LsHit *x = (const LsHit *)a, *y = (const LsHit *)b;
    if (x->bin != y->bin) return x->bin < y->bin ? -1 : 1;
    return x->i < y->i ? -1 : x->i > y->i;
}
/* (seq, ls, re, le, rs, -score, -matches, columns) */
static int ls_by_record(const void *a, const void *b) {
    static const int order[8] = {0, 1, 4, 2, 3, 5, 6, 7}, sign[8] = {1, 1, 1, 1, 1, -1, -1, 1};
    const LsRec *x = (const LsRec *)a, *y = (const LsRec *)b;
    for (int k = 0; k < 8; k++) {
        const int32_t u = x->f[order[k]], v = y->f[order[k]];
        if (u != v) return (u < v ? -1 : 1) * sign[k];
    }
    return 0;
}

typedef struct { LsRec *v; int64_t n, cap; } LsRecs;
static void ls_push(LsRecs *R, const LsRec *r) {
    if (R->n == R->cap) { R->cap = R->cap ? 2 * R->cap : 256; R->v = (LsRec *)realloc(R->v, (size_t)R->cap * sizeof(LsRec)); }
    R->v[R->n++] = *r;
}

/* steps 4 and 5 for one run of sequence q (codes c, length n) */
static void ls_run(int32_t q, const uint8_t *c, int64_t n, int64_t i_lo, int64_t i_hi, int64_t d_lo, int64_t d_hi, int32_t min_len,
                   int32_t max_len, int32_t min_ltr, int32_t max_ltr, int32_t identity, LsRecs *R, int64_t *st) {
    int64_t pads[4] = {256, 1024, 4096, max_ltr};
    const int64_t dc = (d_lo + d_hi) >> 1;
    int pl = 0, pr = 0, redo = 0;
    Hsp h;
    int64_t ls, le, rs, re;
    for (int k = 0; k < 4; k++) if (pads[k] > max_ltr) pads[k] = max_ltr;
    for (;;) {
        const int64_t qb = i_lo - pads[pl] > 0 ? i_lo - pads[pl] : 0, qe = i_hi + LS_WORD + pads[pr] < n ? i_hi + LS_WORD + pads[pr] : n;
        const int64_t sb = qb + dc - LS_BAND_BELOW > 0 ? qb + dc - LS_BAND_BELOW : 0, se = qe + dc + LS_BAND_ABOVE < n ? qe + dc + LS_BAND_ABOVE : n;
        const int64_t dlo = dc - LS_BAND_BELOW - (sb - qb);
        int step = 0;
        st[4]++;
        if (se <= sb || !align(c + qb, c + sb, dlo, dlo + LS_BAND_BELOW + LS_BAND_ABOVE - 1, 1, (int)(qe - qb), 1, (int)(se - sb), &h) ||
            h.score < MIN_SCORE) {
            st[6]++;
            return;
        }
        ls = qb + h.qs - 1; le = qb + h.qe; rs = sb + h.ss - 1; re = sb + h.se;
        if (ls - qb < LS_EDGE && qb > 0 && pl < 3) { pl++; step = 1; }
        if (qe - le < LS_EDGE && qe < n && pr < 3) { pr++; step = 1; }
        if (!step || redo == LS_MAX_REDO) break;
        redo++;
        st[5]++;
    }
    if (le - ls < min_ltr || le - ls > max_ltr || re - rs < min_ltr || re - rs > max_ltr) { st[7]++; return; }
    if (re - ls < min_len || re - ls > max_len) { st[8]++; return; }
    if (le > rs) { st[9]++; return; }
    if ((int64_t)100 * h.matches < (int64_t)identity * h.columns) { st[10]++; return; }
    {
        const LsRec r = {{q, (int32_t)ls, (int32_t)le, (int32_t)rs, (int32_t)re, h.score, h.matches, h.columns}};
        ls_push(R, &r);
    }
}

int twin_ltr_scan(int64_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t min_len, int32_t max_len, int32_t min_ltr, int32_t max_ltr,
                  int32_t identity, int64_t cap, int32_t *recs, int64_t *n_out, int64_t *st) {
    LsRecs R = {0, 0, 0};
    int64_t kept = 0;
    const int64_t dmin = min_ltr, dmax = (int64_t)max_len - min_ltr;
    if (n < 0 || cap < 0 || min_ltr < 1 || min_ltr > max_ltr || max_ltr > LS_MAX_LTR || min_len > max_len || identity < 1 || identity > 100) return -1;
    memset(st, 0, 12 * sizeof(int64_t));
    for (int64_t q = 0; q < n; q++) {
        const int64_t len = seq_off[q + 1] - seq_off[q];
        const uint8_t *b = seqs + seq_off[q];
        int64_t nw = 0, nh = 0;
        uint8_t *c;
        LsWord *w;
        LsHit *hit;
        if (len < LS_WORD) continue;
        c = (uint8_t *)malloc((size_t)len);
        w = (LsWord *)malloc((size_t)len * sizeof(LsWord));
        hit = (LsHit *)malloc((size_t)len * sizeof(LsHit));
        for (int64_t i = 0; i < len; i++) c[i] = (uint8_t)code_of(b[i]);
        for (int64_t i = 0; i + LS_WORD <= len; i++) {           /* 1. words */
            uint32_t x = 0;
            int ok = 1;
            for (int k = 0; k < LS_WORD && ok; k++) { ok = c[i + k] < 4; x = x * 4 + c[i + k]; }
            if (ok) { w[nw].word = x; w[nw].pos = (int32_t)i; nw++; }
        }
        st[0] += nw;
        qsort(w, (size_t)nw, sizeof(LsWord), ls_by_word);
        for (int64_t k = 0; k < nw; k++)                         /* 2. links */
            for (int64_t t = k + 1; t <= k + LS_MAX_OCC && t < nw && w[t].word == w[k].word; t++) {
                const int64_t d = (int64_t)w[t].pos - w[k].pos;
                if (d < dmin) continue;
                if (d <= dmax) { hit[nh].i = w[k].pos; hit[nh].d = (int32_t)d; nh++; }
                break;
            }
        st[1] += nh;
        for (int lam = 0; lam <= 32; lam += 32) {                /* 3. runs */
            for (int64_t k = 0; k < nh; k++) hit[k].bin = (int32_t)(((int64_t)hit[k].d + lam) >> LS_BIN_SHIFT);
            qsort(hit, (size_t)nh, sizeof(LsHit), ls_by_bin);
            for (int64_t k = 0; k < nh;) {
                int64_t e = k + 1, d_lo = hit[k].d, d_hi = hit[k].d;
                while (e < nh && hit[e].bin == hit[k].bin && hit[e].i - hit[e - 1].i <= LS_GAP) {
                    if (hit[e].d < d_lo) d_lo = hit[e].d;
                    if (hit[e].d > d_hi) d_hi = hit[e].d;
                    e++;
                }
                if (e - k >= LS_MIN_HITS) {
                    st[2]++;
                    if ((int64_t)hit[e - 1].i - hit[k].i + LS_WORD > max_ltr) st[3]++;
                    else ls_run((int32_t)q, c, len, hit[k].i, hit[e - 1].i, d_lo, d_hi, min_len, max_len, min_ltr, max_ltr, identity, &R, st);
                }
                k = e;
            }
        }
        free(c); free(w); free(hit);
    }
    qsort(R.v, (size_t)R.n, sizeof(LsRec), ls_by_record);        /* 6. order and duplicates */
    for (int64_t k = 0; k < R.n; k++) {
        if (k > 0 && memcmp(R.v[k].f, R.v[k - 1].f, 5 * sizeof(int32_t)) == 0) continue;
        if (kept < cap) memcpy(recs + 8 * kept, R.v[k].f, sizeof(R.v[k].f));
        kept++;
    }
    free(R.v);
    st[11] = kept;
    *n_out = kept;
    return kept > cap ? -4 : 0;
}

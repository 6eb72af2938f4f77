/* TEST INFRASTRUCTURE: the fast form of the CPU twin of hite_annotate (tests/annotate_twin.py compiles and loads this file; the
 * definition is in include/hite_gpu.h, "genome annotation", and tests/annotate_twin.py states it readably).  Plain C, one piece after
 * the other, every step as the definition numbers it; step 4 is align() of tests/pairhsp_twin.c, included as it stands.  Nothing here
 * is shared with the HIP code. */
#include "pairhsp_twin.c"

#define AN_WORD 13
#define AN_MAX_OCC 16
#define AN_BIN_SHIFT 6
#define AN_GAP 300
#define AN_MIN_HITS 3
#define AN_MAX_SPAN 8192
#define AN_BAND_BELOW 96
#define AN_BAND_ABOVE 96
#define AN_EDGE 32
#define AN_MAX_REDO 3
#define AN_PIECE (1 << 24)
#define AN_MIN_PIECE 256
#define AN_OVERLAP (1 << 16)
#define AN_MAX_LIB_LEN 24576
#define AN_MAX_LIB 32768

typedef struct { uint32_t word; int32_t t, q; } AnEntry;
typedef struct { int32_t t, bin, g, d; } AnHit;
typedef struct { int32_t f[10]; } AnRec;
typedef struct { AnRec *v; int64_t n, cap; } AnRecs;
typedef struct { AnHit *v; int64_t n, cap; } AnHits;

static int an_by_word(const void *a, const void *b) {
    const AnEntry *x = (const AnEntry *)a, *y = (const AnEntry *)b;
    if (x->word != y->word) return x->word < y->word ? -1 : 1;
    if (x->t != y->t) return x->t < y->t ? -1 : 1;
    return x->q < y->q ? -1 : x->q > y->q;
}
static int an_by_bin(const void *a, const void *b) {
    const AnHit *x = (const AnHit *)a, *y = (const AnHit *)b;
    if (x->t != y->t) return x->t < y->t ? -1 : 1;
    if (x->bin != y->bin) return x->bin < y->bin ? -1 : 1;
    return x->g < y->g ? -1 : x->g > y->g;
}
/* the order key: (seq, g_start, g_end, lib, strand, q_start, q_end, -score, -matches, columns) */
static int an_by_record(const void *a, const void *b) {
    static const int sign[10] = {1, 1, 1, 1, 1, 1, 1, -1, -1, 1};
    const AnRec *x = (const AnRec *)a, *y = (const AnRec *)b;
    for (int k = 0; k < 10; k++)
        if (x->f[k] != y->f[k]) return (x->f[k] < y->f[k] ? -1 : 1) * sign[k];
    return 0;
}
static void an_push(AnRecs *R, const AnRec *r) {
    if (R->n == R->cap) { R->cap = R->cap ? 2 * R->cap : 256; R->v = (AnRec *)realloc(R->v, (size_t)R->cap * sizeof(AnRec)); }
    R->v[R->n++] = *r;
}
static void an_hit(AnHits *H, int32_t t, int32_t g, int32_t d) {
    if (H->n == H->cap) { H->cap = H->cap ? 2 * H->cap : 1024; H->v = (AnHit *)realloc(H->v, (size_t)H->cap * sizeof(AnHit)); }
    H->v[H->n].t = t; H->v[H->n].g = g; H->v[H->n].d = d; H->v[H->n].bin = 0;
    H->n++;
}
/* the word at c[i, i + 13), or -1 */
static int64_t an_word_at(const uint8_t *c, int64_t i) {
    int64_t w = 0;
    for (int k = 0; k < AN_WORD; k++) {
        if (c[i + k] > 3) return -1;
        w = w * 4 + c[i + k];
    }
    return w;
}

/* step 4 for one run of text t (codes tc, L bases; L0: the entry's length) on sequence s (codes c, len bases) */
static void an_run(int32_t seq, const uint8_t *c, int64_t len, int32_t t, const uint8_t *tc, int64_t L, int64_t g_lo, int64_t g_hi, int64_t d_lo,
                   int64_t d_hi, AnRecs *R, int64_t *st) {
    static const int64_t pads[4] = {256, 1024, 4096, 8192};
    const int64_t dc = (d_lo + d_hi) >> 1, q_lo = g_lo - dc, q_hi = g_hi - dc;
    int pl = 0, pr = 0, redo = 0;
    Hsp h;
    int64_t qs, qe, gs, ge;
    for (;;) {
        const int64_t qb = q_lo - pads[pl] > 0 ? q_lo - pads[pl] : 0, qend = q_hi + AN_WORD + pads[pr] < L ? q_hi + AN_WORD + pads[pr] : L;
        const int64_t sb = qb + dc - AN_BAND_BELOW > 0 ? qb + dc - AN_BAND_BELOW : 0, se = qend + dc + AN_BAND_ABOVE < len ? qend + dc + AN_BAND_ABOVE : len;
        const int64_t dlo = dc - AN_BAND_BELOW - (sb - qb);
        int step = 0;
        st[5]++;
        if (qend <= qb || se <= sb || !align(tc + qb, c + sb, dlo, dlo + AN_BAND_BELOW + AN_BAND_ABOVE - 1, 1, (int)(qend - qb), 1, (int)(se - sb), &h) ||
            h.score < MIN_SCORE) {
            st[7]++;
            return;
        }
        qs = qb + h.qs - 1; qe = qb + h.qe; gs = sb + h.ss - 1; ge = sb + h.se;
        if (qs - qb < AN_EDGE && qb > 0 && pl < 3) { pl++; step = 1; }
        if (qend - qe < AN_EDGE && qend < L && pr < 3) { pr++; step = 1; }
        if (!step || redo == AN_MAX_REDO) break;
        redo++;
        st[6]++;
    }
    {
        const int rc = t & 1;
        const AnRec r = {{seq, (int32_t)gs, (int32_t)ge, t >> 1, rc, (int32_t)(rc ? L - qe : qs), (int32_t)(rc ? L - qs : qe), h.score, h.matches, h.columns}};
        an_push(R, &r);
    }
}

int twin_annotate(int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int32_t n_lib, const uint8_t *lib, const int64_t *lib_off,
                  int32_t piece_len, int64_t cap, int32_t *recs, int64_t *n_out, int8_t *lib_status, int64_t *st) {
    AnRecs R = {0, 0, 0};
    AnHits H = {0, 0, 0};
    AnEntry *tab;
    uint8_t **tc;
    uint8_t *silent;
    int64_t nt = 0, total = 0, room = 0;
    const int64_t P = piece_len ? piece_len : AN_PIECE;
    if (n_seq < 0 || n_lib < 0 || n_lib > AN_MAX_LIB || cap < 0 || (piece_len != 0 && (piece_len < AN_MIN_PIECE || piece_len > AN_PIECE))) return -1;
    for (int64_t s = 0; s < n_seq; s++) if (seq_off[s + 1] < seq_off[s] || seq_off[s + 1] - seq_off[s] >= ((int64_t)1 << 31)) return -1;
    for (int32_t e = 0; e < n_lib; e++) if (lib_off[e + 1] < lib_off[e]) return -1;
    memset(st, 0, 12 * sizeof(int64_t));
    /* 1. the texts and the table */
    tc = (uint8_t **)calloc((size_t)2 * n_lib + 1, sizeof(uint8_t *));
    for (int32_t e = 0; e < n_lib; e++) {
        const int64_t L = lib_off[e + 1] - lib_off[e];
        lib_status[e] = L > AN_MAX_LIB_LEN ? -1 : 0;
        if (L > AN_MAX_LIB_LEN) { st[2]++; continue; }
        tc[2 * e] = (uint8_t *)malloc((size_t)L + 1);
        tc[2 * e + 1] = (uint8_t *)malloc((size_t)L + 1);
        for (int64_t k = 0; k < L; k++) {
            const int x = code_of(lib[lib_off[e] + k]);
            tc[2 * e][k] = (uint8_t)x;
            tc[2 * e + 1][L - 1 - k] = (uint8_t)(x < 4 ? 3 - x : 4);
        }
        room += 2 * L;
    }
    tab = (AnEntry *)malloc((size_t)(room + 1) * sizeof(AnEntry));
    for (int32_t t = 0; t < 2 * n_lib; t++) {
        const int64_t L = lib_off[(t >> 1) + 1] - lib_off[t >> 1];
        if (!tc[t]) continue;
        for (int64_t q = 0; q + AN_WORD <= L; q++) {
            const int64_t w = an_word_at(tc[t], q);
            if (w >= 0) { tab[nt].word = (uint32_t)w; tab[nt].t = t; tab[nt].q = (int32_t)q; nt++; }
        }
    }
    qsort(tab, (size_t)nt, sizeof(AnEntry), an_by_word);
    silent = (uint8_t *)calloc((size_t)nt + 1, 1);
    for (int64_t a = 0; a < nt;) {
        int64_t b = a + 1;
        while (b < nt && tab[b].word == tab[a].word) b++;
        if (b - a > AN_MAX_OCC) { memset(silent + a, 1, (size_t)(b - a)); st[1] += b - a; }
        a = b;
    }
    st[0] = nt;
    for (int64_t s = 0; s < n_seq && nt > 0; s++) {
        const int64_t len = seq_off[s + 1] - seq_off[s];
        uint8_t *c;
        if (len < AN_WORD) continue;
        c = (uint8_t *)malloc((size_t)len);
        for (int64_t i = 0; i < len; i++) c[i] = (uint8_t)code_of(seqs[seq_off[s] + i]);
        for (int64_t k = 0; k * P < len; k++) {                   /* 2. pieces and hits */
            const int64_t begin = k * P, end = (k + 1) * P + AN_OVERLAP < len ? (k + 1) * P + AN_OVERLAP : len;
            H.n = 0;
            for (int64_t g = begin; g + AN_WORD <= end; g++) {
                const int64_t w = an_word_at(c, g);
                int64_t lo = 0, hi = nt;
                if (w < 0) continue;
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (tab[mid].word < (uint32_t)w) lo = mid + 1; else hi = mid; }
                for (; lo < nt && tab[lo].word == (uint32_t)w && !silent[lo]; lo++) an_hit(&H, tab[lo].t, (int32_t)g, (int32_t)(g - tab[lo].q));
            }
            st[3] += H.n;
            for (int lam = 0; lam <= 32; lam += 32) {             /* 3. runs */
                for (int64_t h = 0; h < H.n; h++) H.v[h].bin = (int32_t)(((int64_t)H.v[h].d - begin + lam + AN_MAX_LIB_LEN) >> AN_BIN_SHIFT);
                qsort(H.v, (size_t)H.n, sizeof(AnHit), an_by_bin);
                for (int64_t a = 0; a < H.n;) {
                    int64_t b = a + 1, d_lo = H.v[a].d, d_hi = H.v[a].d;
                    while (b < H.n && H.v[b].t == H.v[a].t && H.v[b].bin == H.v[a].bin && H.v[b].g - H.v[b - 1].g <= AN_GAP &&
                           H.v[b].g - H.v[a].g < AN_MAX_SPAN) {
                        if (H.v[b].d < d_lo) d_lo = H.v[b].d;
                        if (H.v[b].d > d_hi) d_hi = H.v[b].d;
                        b++;
                    }
                    if (b - a >= AN_MIN_HITS) {
                        const int32_t t = H.v[a].t;
                        st[4]++;
                        an_run((int32_t)s, c, len, t, tc[t], lib_off[(t >> 1) + 1] - lib_off[t >> 1], H.v[a].g, H.v[b - 1].g, d_lo, d_hi, &R, st);
                    }
                    a = b;
                }
            }
        }
        free(c);
    }
    st[8] = R.n;
    qsort(R.v, (size_t)R.n, sizeof(AnRec), an_by_record);        /* 5. resolve: (a) duplicates */
    {
        int64_t m = 0;
        for (int64_t k = 0; k < R.n; k++) {
            if (k > 0 && memcmp(R.v[k].f, R.v[m - 1].f, 7 * sizeof(int32_t)) == 0) { st[9]++; continue; }
            R.v[m++] = R.v[k];
        }
        R.n = m;
    }
    for (int64_t a = 0; a < R.n; a++) {                          /* (b) every A against every B; 6. the order is the sorted one */
        const int32_t *A = R.v[a].f;
        int dropped = 0;
        int64_t b0 = a;      /* (a record is shorter than MAX_LEN: one that begins MAX_LEN before A cannot reach it) */
        while (b0 > 0 && R.v[b0 - 1].f[0] == A[0] && (int64_t)R.v[b0 - 1].f[1] + MAX_LEN > A[1]) b0--;
        for (int64_t b = b0; b < R.n && !dropped; b++) {
            const int32_t *B = R.v[b].f;
            int64_t lo, hi;
            if (B[0] != A[0] || B[1] >= A[2]) break;
            if (b == a) continue;
            lo = A[1] > B[1] ? A[1] : B[1]; hi = A[2] < B[2] ? A[2] : B[2];
            if (hi - lo <= 0 || 5 * (hi - lo) < 4 * ((int64_t)A[2] - A[1])) continue;
            dropped = B[7] > A[7] || (B[7] == A[7] && an_by_record(B, A) < 0);
        }
        if (dropped) { st[10]++; continue; }
        if (total < cap) memcpy(recs + 10 * total, A, 10 * sizeof(int32_t));
        total++;
    }
    for (int32_t t = 0; t < 2 * n_lib; t++) free(tc[t]);
    free(tc); free(tab); free(silent); free(R.v); free(H.v);
    st[11] = total;
    *n_out = total;
    return total > cap ? -4 : 0;
}

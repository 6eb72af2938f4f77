/* protein_twin.c -- the two extension loops of the translated protein search as plain scalar C (the rest of the twin is
 * tests/protein_twin.py; the definition is in include/hite_gpu.h, "translated protein search").  Test infrastructure: the product
 * neither includes nor links this file; tests/protein_twin.py builds it with the host compiler.
 *
 * Sequences are residue codes 0..21 (0..19 standard, 20 X, 21 '*'); tab is the 24 x 24 table of every pair's score. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TABW 24
#define XDROP 16
#define GAP_OPEN 12 /* the first column of a gap: 11 + 1 */
#define GAP_EXT 1

/* step 4: the seed x[i..i+3] / y[j..j+3] extended on its diagonal.  -> score, seg[0..1] = first and last frame position */
int twin_ungapped(const uint8_t *x, int lx, int i, const uint8_t *y, int ly, int j, const int8_t *tab, int *seg) {
    int score = 0, k;
    for (k = 0; k < 4; k++) score += tab[x[i + k] * TABW + y[j + k]];
    /* to the right */
    {
        int a = i + 4, b = j + 4, run = 0, best = 0, best_a = i + 3;
        while (a < lx && b < ly) {
            run += tab[x[a] * TABW + y[b]];
            if (run > best) { best = run; best_a = a; }
            if (best - run > XDROP) break;
            a++; b++;
        }
        score += best;
        seg[1] = best_a;
    }
    /* to the left */
    {
        int a = i - 1, b = j - 1, run = 0, best = 0, best_a = i;
        while (a >= 0 && b >= 0) {
            run += tab[x[a] * TABW + y[b]];
            if (run > best) { best = run; best_a = a; }
            if (best - run > XDROP) break;
            a--; b--;
        }
        score += best;
        seg[0] = best_a;
    }
    return score;
}

typedef struct { int v, si, sj, id, cols; } cell_t; /* v == 0: no alignment ends here */

/* step 6: rows lo..hi of the frame x, diagonals dlo..dhi (j - i), protein y of ly residues; row-major, one cell at a time.
 * out = score, start i, start j, end i, end j, identical, columns (all 0 without an alignment).  -> 0, or -1 without memory */
int twin_gapped(const uint8_t *x, int lo, int hi, const uint8_t *y, int ly, long dlo, long dhi, const int8_t *tab, int *out) {
    cell_t *Hp, *Ep, *Hc, *Ec, *tmp;
    cell_t best;
    int i, bi = 0, bj = 0;
    memset(out, 0, 7 * sizeof(int));
    memset(&best, 0, sizeof best);
    if (ly <= 0 || hi < lo) return 0;
    Hp = calloc((size_t)ly, sizeof(cell_t)); Ep = calloc((size_t)ly, sizeof(cell_t));
    Hc = calloc((size_t)ly, sizeof(cell_t)); Ec = calloc((size_t)ly, sizeof(cell_t));
    if (!Hp || !Ep || !Hc || !Ec) { free(Hp); free(Ep); free(Hc); free(Ec); return -1; }
    for (i = lo; i <= hi; i++) {
        long jlo = (long)i + dlo, jhi = (long)i + dhi, j;
        cell_t F, zero;
        memset(&zero, 0, sizeof zero);
        if (jlo < 0) jlo = 0;
        if (jhi > ly - 1) jhi = ly - 1;
        memset(Hc, 0, (size_t)ly * sizeof(cell_t));
        memset(Ec, 0, (size_t)ly * sizeof(cell_t));
        F = zero;
        for (j = jlo; j <= jhi; j++) {
            const int a = x[i], b = y[j];
            const cell_t hd = j >= 1 ? Hp[j - 1] : zero;   /* (i-1, j-1) */
            const cell_t hu = Hp[j], eu = Ep[j];            /* (i-1, j)   */
            const cell_t hl = j > jlo ? Hc[j - 1] : zero;   /* (i, j-1)   */
            cell_t D, E, H;
            /* diagonal */
            if (hd.v > 0) D = hd; else { D = zero; D.si = i; D.sj = (int)j; }
            D.v = hd.v + tab[a * TABW + b];
            D.id += (a == b && a < 20);
            D.cols += 1;
            /* gap in the protein */
            if (hu.v - GAP_OPEN >= eu.v - GAP_EXT) { E = hu; E.v = hu.v - GAP_OPEN; } else { E = eu; E.v = eu.v - GAP_EXT; }
            E.cols += 1;
            if (E.v <= 0) E = zero;
            /* gap in the frame */
            if (hl.v - GAP_OPEN >= F.v - GAP_EXT) { F = hl; F.v = hl.v - GAP_OPEN; } else { F.v = F.v - GAP_EXT; }
            F.cols += 1;
            if (F.v <= 0) F = zero;
            if (D.v >= E.v && D.v >= F.v) H = D; else if (E.v >= F.v) H = E; else H = F;
            if (H.v <= 0) H = zero;
            Hc[j] = H; Ec[j] = E;
            if (H.v > best.v) { best = H; bi = i; bj = (int)j; }
        }
        tmp = Hp; Hp = Hc; Hc = tmp;
        tmp = Ep; Ep = Ec; Ec = tmp;
    }
    if (best.v > 0) {
        out[0] = best.v; out[1] = best.si; out[2] = best.sj; out[3] = bi; out[4] = bj; out[5] = best.id; out[6] = best.cols;
    }
    free(Hp); free(Ep); free(Hc); free(Ec);
    return 0;
}

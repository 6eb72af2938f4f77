/* TEST INFRASTRUCTURE: the fast form of the CPU twin of hite_frame_cluster (tests/framecluster_twin.py compiles and loads this file;
 * the product links none of it).  The definition is the one of include/hite_gpu.h, "clusters of a group of frames", cell by cell
 * and row by row:
 *   a value is (score, matches, columns, bases of A, bases of B), compared lexicographically; E is all zero; V(i, 0) = V(0, j) = E;
 *   V(i, j) = the largest of V(i-1, j-1) + (+2, 1, 1, 1, 1) [A[i] = B[j], both in ACGT] or + (-2, 0, 1, 1, 1) [else],
 *   V(i-1, j) + (-3, 0, 1, 1, 0) and V(i, j-1) + (-3, 0, 1, 0, 1), replaced by E when its score is <= 0; R = the largest V. */
#include <stdint.h>
#include <string.h>

#define MAX_ROWS 128
#define MAX_LEN 256

/* a value as one signed integer, the score on top: score * 2^37 + matches * 2^28 + columns * 2^18 + a * 2^9 + b.  The four lower
 * fields are never negative and stay below their radix (matches, a, b <= 256, columns <= 512), so the integer order is the
 * lexicographic order of the tuples and a step is one addition. */
typedef int64_t val;
#define ONE ((val)1 << 37)
#define STEP(s, k, c, a, b) ((val)(s) * ONE + ((val)(k) << 28) + ((val)(c) << 18) + ((val)(a) << 9) + (val)(b))

static int code(uint8_t ch) {
    switch (ch) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

/* R(A, B), or R(A, revcomp(B)) */
static val pair_one(const uint8_t *a, int m, const uint8_t *b, int n, int rev) {
    val prev[MAX_LEN + 1], cur[MAX_LEN + 1], best = 0;
    int cb[MAX_LEN + 1];
    for (int j = 1; j <= n; j++) {
        cb[j] = rev ? code(b[n - j]) : code(b[j - 1]);
        if (rev && cb[j] < 4) cb[j] = 3 - cb[j];
    }
    for (int j = 0; j <= n; j++) prev[j] = 0;
    for (int i = 1; i <= m; i++) {
        const int ca = code(a[i - 1]);
        cur[0] = 0;
        for (int j = 1; j <= n; j++) {
            val v = prev[j - 1] + ((ca == cb[j] && ca < 4) ? STEP(2, 1, 1, 1, 1) : STEP(-2, 0, 1, 1, 1));
            const val u = prev[j] + STEP(-3, 0, 1, 1, 0), l = cur[j - 1] + STEP(-3, 0, 1, 0, 1);
            if (u > v) v = u;
            if (l > v) v = l;
            if (v < ONE) v = 0;         /* score <= 0 */
            cur[j] = v;
            if (v > best) best = v;
        }
        memcpy(prev, cur, sizeof(val) * (size_t)(n + 1));
    }
    return best;
}

static val pair_value(const uint8_t *a, int m, const uint8_t *b, int n, int both) {
    val r = pair_one(a, m, b, n, 0);
    if (both) {
        const val r2 = pair_one(a, m, b, n, 1);
        if (r2 > r) r = r2;
    }
    return r;
}

#define F_K(r) ((int)(((r) >> 28) & 511))
#define F_C(r) ((int)(((r) >> 18) & 1023))
#define F_A(r) ((int)(((r) >> 9) & 511))
#define F_B(r) ((int)((r) & 511))

void twin_pair_value(const uint8_t *a, int m, const uint8_t *b, int n, int both, int32_t *out) {
    const val r = pair_value(a, m, b, n, both);
    out[0] = (int32_t)(r >> 37); out[1] = F_K(r); out[2] = F_C(r); out[3] = F_A(r); out[4] = F_B(r);
}

static int similar(val r, int la, int lb, double ident, double cov_short, double cov_long, int min_cov) {
    return F_C(r) > 0 && (double)F_K(r) >= ident * (double)F_C(r) && F_A(r) >= min_cov && F_B(r) >= min_cov &&
           (double)F_A(r) >= cov_long * (double)la && (double)F_B(r) >= cov_short * (double)lb;
}

int twin_frame_cluster(int64_t n_group, const int64_t *row_off, const uint8_t *seqs, const int64_t *seq_off, double ident,
                       double cov_short, double cov_long, int32_t min_cov, int32_t min_len, int32_t both, int32_t *cluster_of_row,
                       int32_t *n_cluster) {
    for (int64_t g = 0; g < n_group; g++) {
        const int64_t r0 = row_off[g], r1 = row_off[g + 1];
        int beyond = r1 - r0 > MAX_ROWS;
        for (int64_t r = r0; r < r1; r++) {
            cluster_of_row[r] = -1;
            if (seq_off[r + 1] - seq_off[r] > MAX_LEN) beyond = 1;
        }
        n_cluster[g] = beyond ? -1 : 0;
        if (beyond) continue;
        int64_t order[MAX_ROWS], rep[MAX_ROWS];
        int n = 0, n_rep = 0;
        for (int64_t r = r0; r < r1; r++) {         /* insertion: length descending, then row index */
            const int64_t len = seq_off[r + 1] - seq_off[r];
            if (len <= min_len) continue;
            int at = n++;
            while (at > 0 && seq_off[order[at - 1] + 1] - seq_off[order[at - 1]] < len) { order[at] = order[at - 1]; at--; }
            order[at] = r;
        }
        for (int k = 0; k < n; k++) {
            const int64_t r = order[k];
            const int lb = (int)(seq_off[r + 1] - seq_off[r]);
            int found = -1;
            for (int c = 0; c < n_rep && found < 0; c++) {
                const int64_t q = rep[c];
                const int la = (int)(seq_off[q + 1] - seq_off[q]);
                if (similar(pair_value(seqs + seq_off[q], la, seqs + seq_off[r], lb, both), la, lb, ident, cov_short, cov_long, min_cov))
                    found = c;
            }
            if (found < 0) { found = n_rep; rep[n_rep++] = r; }
            cluster_of_row[r] = found;
        }
        n_cluster[g] = n_rep;
    }
    return 0;
}

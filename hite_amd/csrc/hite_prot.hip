// hite_prot.hip -- translated protein-domain search (second half): the in-tree stage where the reference
// runs `blastx -evalue 1e-20 -outfmt 6` of the low-copy candidates against TIRPeps.lib / HelitronPeps.lib / non_LTR.lib
// (get_domain_info Util.py:4571-4612, multiple_alignment_blastx_v1 :1006-1262).  The tool is not pinned (no machine of the project has
// it): parity is the written definition in include/hite_gpu.h ("translated protein search"), its CPU twin tests/protein_twin.py +
// tests/protein_twin.c, HIP == twin record for record, and a recall measurement against planted domains (tools/protein_bench.py).
//
// Stages of one hite_protein_search call (all temporaries from the grow-only arena of the library handle):
//   prot_translate_kernel   one thread per frame residue: six frames of every query as residue codes, frames concatenated (CSR)
//   prot_seed_count_kernel  one thread per frame residue: its 4-mer's bucket and the bucket's length; a scan of the lengths hands
//   prot_ungapped_kernel    ONE THREAD PER SEED HIT its (frame position, library position): X-drop extension on the diagonal,
//                           survivors (segment score >= 41) appended through an atomic counter as two sort keys
//   sort (hite_sort.h, two stable LSD stages: (diagonal, segment), then (frame, protein)) + prot_unique_* : the order and the set of
//                           the survivors do not depend on the order of the append
//   host                    clusters of diagonals -> pieces -> tasks (sequential per (frame, protein) group; prot_form_tasks)
//   prot_gapped_kernel      ONE WAVEFRONT PER TASK, lane = one of the 64 diagonals of the band, H / E / F and the payload (start cell,
//                           identical columns, columns) in registers, neighbours by lane shifts.  Cell (i, d) depends on (i, d-1) and on
//                           (i-1, d+1): a schedule linear in (i, d) needs two steps per row (a step = 2 (i - lo) + lane), so a task of
//                           r rows takes 2 r + 62 steps and a lane is active at every other one.
//   host                    threshold flag -> HSP filter per (frame, protein) -> base coordinates -> final order
// The library index (hite_protein_lib_build): prot_kmer_kernel (bucket of every library 4-mer + bucket counts), a scan of the counts
// (hite_scan.h) -> the 20^4-bucket directory, and a stable radix sort of (bucket, position) as the fill: entries in position order.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include "hite_arena.h"
#include "hite_scan.h"
#include "hite_sort.h"
#include <math.h>
#include <algorithm>
#include <vector>
#include <new>

#ifndef PROT_TAB
#define PROT_TAB static __device__ const
#endif

// >>> prot_tables
// residue codes: 0..19 = ARNDCQEGHILKMFPSTWYV (the order of the BLOSUM62 rows below), 20 = X, 21 = '*'
#define PROT_X 20
#define PROT_STOP 21
#define PROT_NCODE 22
#define PROT_TABW 24               // row width of the expanded score table (prot_score of every code pair)
#define PROT_GAP_OPEN 12           // a gap of g residues costs 11 + g: the first gap column 12,
#define PROT_GAP_EXT 1             // every further one 1
#define PROT_XDROP 16
#define PROT_UNGAPPED_MIN 41
#define PROT_BUCKETS 160000        // 20^4
#define PROT_DIAG_JOIN 16          // a survivor joins the open cluster while d <= c + 16
#define PROT_SPLIT 128             // ... and a cluster splits where a segment starts more than 128 residues after the largest end so far
#define PROT_BAND_LO 24            // band: diagonals c - 24 .. c + 39
#define PROT_BAND_HI 39
#define PROT_MAX_AA 65535          // residues of a library protein / of a frame
PROT_TAB int8_t prot_blosum62[400] = {
     4, -1, -2, -2,  0, -1, -1,  0, -2, -1, -1, -1, -1, -2, -1,  1,  0, -3, -2,  0,
    -1,  5,  0, -2, -3,  1,  0, -2,  0, -3, -2,  2, -1, -3, -2, -1, -1, -3, -2, -3,
    -2,  0,  6,  1, -3,  0,  0,  0,  1, -3, -3,  0, -2, -3, -2,  1,  0, -4, -2, -3,
    -2, -2,  1,  6, -3,  0,  2, -1, -1, -3, -4, -1, -3, -3, -1,  0, -1, -4, -3, -3,
     0, -3, -3, -3,  9, -3, -4, -3, -3, -1, -1, -3, -1, -2, -3, -1, -1, -2, -2, -1,
    -1,  1,  0,  0, -3,  5,  2, -2,  0, -3, -2,  1,  0, -3, -1,  0, -1, -2, -1, -2,
    -1,  0,  0,  2, -4,  2,  5, -2,  0, -3, -3,  1, -2, -3, -1,  0, -1, -3, -2, -2,
     0, -2,  0, -1, -3, -2, -2,  6, -2, -4, -4, -2, -3, -3, -2,  0, -2, -2, -3, -3,
    -2,  0,  1, -1, -3,  0,  0, -2,  8, -3, -3, -1, -2, -1, -2, -1, -2, -2,  2, -3,
    -1, -3, -3, -3, -1, -3, -3, -4, -3,  4,  2, -3,  1,  0, -3, -2, -1, -3, -1,  3,
    -1, -2, -3, -4, -1, -2, -3, -4, -3,  2,  4, -2,  2,  0, -3, -2, -1, -2, -1,  1,
    -1,  2,  0, -1, -3,  1,  1, -2, -1, -3, -2,  5, -1, -3, -1,  0, -1, -3, -2, -2,
    -1, -1, -2, -3, -1,  0, -2, -3, -2,  1,  2, -1,  5,  0, -2, -1, -1, -1, -1,  1,
    -2, -3, -3, -3, -2, -3, -3, -3, -1,  0,  0, -3,  0,  6, -4, -2, -2,  1,  3, -1,
    -1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4,  7, -1, -1, -4, -3, -2,
     1, -1,  1,  0, -1,  0,  0,  0, -1, -2, -2,  0, -1, -2, -1,  4,  1, -3, -2, -2,
     0, -1,  0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1,  1,  5, -2, -2,  0,
    -3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1,  1, -4, -3, -2, 11,  2, -3,
    -2, -2, -2, -3, -2, -1, -2, -3,  2, -1, -1, -2, -1,  3, -3, -2, -2,  2,  7, -1,
     0, -3, -3, -3, -1, -2, -2, -3, -3,  3,  1, -2,  1, -1, -2, -2,  0, -3, -1,  4};
// the standard genetic code, codon index = 16 b0 + 4 b1 + b2 with T = 0, C = 1, A = 2, G = 3; values are residue codes
// (F F L L S S S S Y Y * * C C * W / L L L L P P P P H H Q Q R R R R / I I I M T T T T N N K K S S R R / V V V V A A A A D D E E G G G G)
PROT_TAB uint8_t prot_codon_tab[64] = {
    13, 13, 10, 10, 15, 15, 15, 15, 18, 18, 21, 21,  4,  4, 21, 17,
    10, 10, 10, 10, 14, 14, 14, 14,  8,  8,  5,  5,  1,  1,  1,  1,
     9,  9,  9, 12, 16, 16, 16, 16,  2,  2, 11, 11, 15, 15,  1,  1,
    19, 19, 19, 19,  0,  0,  0,  0,  3,  3,  6,  6,  7,  7,  7,  7};
// a query byte (either case) as a base code T 0 / C 1 / A 2 / G 3 / anything else 4; comp: of the complementary base
__device__ __forceinline__ int prot_base_code(uint8_t c, bool comp) {
    int b;
    switch (c & 0xDF) {      // letters to upper case
        case 'T': b = 0; break;
        case 'C': b = 1; break;
        case 'A': b = 2; break;
        case 'G': b = 3; break;
        default: return 4;
    }
    return comp ? (b ^ 2) : b;     // T <-> A, C <-> G
}
__device__ __forceinline__ int prot_codon(int b0, int b1, int b2) {
    return (b0 | b1 | b2) & 4 ? PROT_X : prot_codon_tab[16 * b0 + 4 * b1 + b2];
}
// a library byte as a residue code: the 20 standard letters (either case), everything else X
__device__ __forceinline__ int prot_letter_code(uint8_t c) {
    switch (c & 0xDF) {
        case 'A': return 0;  case 'R': return 1;  case 'N': return 2;  case 'D': return 3;  case 'C': return 4;
        case 'Q': return 5;  case 'E': return 6;  case 'G': return 7;  case 'H': return 8;  case 'I': return 9;
        case 'L': return 10; case 'K': return 11; case 'M': return 12; case 'F': return 13; case 'P': return 14;
        case 'S': return 15; case 'T': return 16; case 'W': return 17; case 'Y': return 18; case 'V': return 19;
        default: return PROT_X;
    }
}
// '*' against anything -4, then X against anything -1, then BLOSUM62
__device__ __forceinline__ int prot_score(int a, int b) {
    if (a == PROT_STOP || b == PROT_STOP) return -4;
    if (a == PROT_X || b == PROT_X) return -1;
    return prot_blosum62[a * 20 + b];
}
// the bucket of the 4-mer (c0, c1, c2, c3), or -1 when it is no seed: a non-standard residue, or fewer than three distinct letters
__device__ __forceinline__ int prot_seed_key(int c0, int c1, int c2, int c3) {
    if (c0 >= 20 || c1 >= 20 || c2 >= 20 || c3 >= 20) return -1;
    const int distinct = 1 + (c1 != c0) + (c2 != c0 && c2 != c1) + (c3 != c0 && c3 != c1 && c3 != c2);
    if (distinct < 3) return -1;
    return ((c0 * 20 + c1) * 20 + c2) * 20 + c3;
}
// the ungapped filter: the seed x[i .. i+3] == y[j .. j+3] extended along its diagonal, to the right from the seed's last column and
// to the left from its first.  Each side keeps the best running sum (the first position that reaches it; 0 = no extension) and stops
// at either sequence's end or as soon as the running sum has dropped MORE than PROT_XDROP below that best (a drop of exactly 16 goes
// on).  -> the segment's score; *i0 .. *i1 = its frame positions (inclusive).  tab: prot_score of every code pair, PROT_TABW a row.
__device__ __forceinline__ int prot_ungapped(const uint8_t *x, int lx, int i, const uint8_t *y, int ly, int j, const int8_t *tab,
                                             int *i0, int *i1) {
    int seed = 0;
    for (int k = 0; k < 4; k++) seed += tab[x[i + k] * PROT_TABW + y[j + k]];
    int run = 0, best = 0, ext = 0;
    const int nr = min(lx - (i + 4), ly - (j + 4));
    for (int k = 0; k < nr; k++) {
        run += tab[x[i + 4 + k] * PROT_TABW + y[j + 4 + k]];
        if (run > best) { best = run; ext = k + 1; }
        else if (best - run > PROT_XDROP) break;
    }
    *i1 = i + 3 + ext;
    int total = seed + best;
    run = 0; best = 0; ext = 0;
    const int nl = min(i, j);
    for (int k = 0; k < nl; k++) {
        run += tab[x[i - 1 - k] * PROT_TABW + y[j - 1 - k]];
        if (run > best) { best = run; ext = k + 1; }
        else if (best - run > PROT_XDROP) break;
    }
    *i0 = i - ext;
    return total + best;
}
// <<< prot_tables

#define PROT_WAVES 4

__device__ __forceinline__ void prot_fill_tab(int8_t *tab) {
    for (int k = threadIdx.x; k < PROT_TABW * PROT_TABW; k += blockDim.x) {
        const int a = k / PROT_TABW, b = k % PROT_TABW;
        tab[k] = (a < PROT_NCODE && b < PROT_NCODE) ? (int8_t)prot_score(a, b) : (int8_t)0;
    }
    __syncthreads();
}

// ---- translation: frame gf = 6 q + f (f 0..2: strands +1 +2 +3, 3..5: -1 -2 -3), residue t covers strand bases (f % 3) + 3 t .. + 2 --------
__global__ __launch_bounds__(256) void prot_translate_kernel(const uint8_t *__restrict__ nt, const int64_t *__restrict__ nt_off,
                                                             const int64_t *__restrict__ frame_off, int64_t n_frames, int ascii,
                                                             uint8_t *__restrict__ out) {
    const int64_t R = frame_off[n_frames];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
        const int64_t gf = last_le(frame_off, n_frames, r);
        const int64_t q = gf / 6;
        const int f = (int)(gf % 6);
        const int64_t L = nt_off[q + 1] - nt_off[q], p = (f % 3) + 3 * (r - frame_off[gf]);
        const uint8_t *s = nt + nt_off[q];
        int b0, b1, b2;
        if (f < 3) { b0 = prot_base_code(s[p], false); b1 = prot_base_code(s[p + 1], false); b2 = prot_base_code(s[p + 2], false); }
        else { b0 = prot_base_code(s[L - 1 - p], true); b1 = prot_base_code(s[L - 2 - p], true); b2 = prot_base_code(s[L - 3 - p], true); }
        const int c = prot_codon(b0, b1, b2);
        out[r] = ascii ? (uint8_t)("ARNDCQEGHILKMFPSTWYVX*"[c]) : (uint8_t)c;
    }
}

// ---- library index ---------------------------------------------------------------------------------------------------------------
// per library position g: its protein, its residue code, the bucket of the 4-mer that starts there (PROT_BUCKETS: none) and the bucket counts
__global__ __launch_bounds__(256) void prot_kmer_kernel(const uint8_t *__restrict__ aa, const int64_t *__restrict__ aa_off, int64_t n_prot,
                                                        int32_t *__restrict__ prot_of, unsigned long long *__restrict__ keys,
                                                        unsigned *__restrict__ vals, int32_t *__restrict__ cnt) {
    const int64_t N = aa_off[n_prot];
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < N; g += (int64_t)gridDim.x * 256) {
        const int64_t p = last_le(aa_off, n_prot, g);
        prot_of[g] = (int32_t)p;
        int key = -1;
        if (g + 3 < aa_off[p + 1]) key = prot_seed_key(aa[g], aa[g + 1], aa[g + 2], aa[g + 3]);
        keys[g] = key < 0 ? (unsigned long long)PROT_BUCKETS : (unsigned long long)key;
        vals[g] = (unsigned)g;
        if (key >= 0) atomicAdd(&cnt[key], 1);
    }
}
__global__ __launch_bounds__(256) void prot_encode_kernel(const uint8_t *__restrict__ in, int64_t n, uint8_t *__restrict__ out) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) out[g] = (uint8_t)prot_letter_code(in[g]);
}

// ---- seeds -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prot_seed_count_kernel(const uint8_t *__restrict__ fr, const int64_t *__restrict__ frame_off,
                                                              int64_t n_frames, const int64_t *__restrict__ dir, int32_t *__restrict__ key_out,
                                                              int32_t *__restrict__ cnt_out) {
    const int64_t R = frame_off[n_frames];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
        const int64_t gf = last_le(frame_off, n_frames, r);
        int key = -1;
        if (r + 3 < frame_off[gf + 1]) key = prot_seed_key(fr[r], fr[r + 1], fr[r + 2], fr[r + 3]);
        key_out[r] = key;
        cnt_out[r] = key < 0 ? 0 : (int32_t)(dir[key + 1] - dir[key]);
    }
}

struct ProtUngapArgs {
    const uint8_t *fr; const int64_t *frame_off; int64_t n_frames;
    const uint8_t *aa; const int64_t *aa_off; const int32_t *prot_of;
    const int64_t *dir; const unsigned *ent;
    const int32_t *key; const int64_t *hit_off; int64_t n_res, n_hits;
    unsigned long long *k1, *k2, *count; int64_t cap;
};
// one thread per seed hit.  Survivor keys: k1 = frame << 32 | protein, k2 = (diagonal + 65535) << 32 | segment start << 16 | segment end
__global__ __launch_bounds__(256) void prot_ungapped_kernel(ProtUngapArgs a) {
    __shared__ int8_t tab[PROT_TABW * PROT_TABW];
    prot_fill_tab(tab);
    for (int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x; h < a.n_hits; h += (int64_t)gridDim.x * 256) {
        const int64_t r = last_le(a.hit_off, a.n_res, h);
        const int64_t g = a.ent[a.dir[a.key[r]] + (h - a.hit_off[r])];
        const int64_t gf = last_le(a.frame_off, a.n_frames, r);
        const int32_t p = a.prot_of[g];
        const int i = (int)(r - a.frame_off[gf]), j = (int)(g - a.aa_off[p]);
        const int lx = (int)(a.frame_off[gf + 1] - a.frame_off[gf]), ly = (int)(a.aa_off[p + 1] - a.aa_off[p]);
        int i0, i1;
        const int s = prot_ungapped(a.fr + a.frame_off[gf], lx, i, a.aa + a.aa_off[p], ly, j, tab, &i0, &i1);
        if (s >= PROT_UNGAPPED_MIN) {
            const unsigned long long slot = atomicAdd(a.count, 1ull);
            if ((int64_t)slot < a.cap) {
                a.k1[slot] = ((unsigned long long)gf << 32) | (unsigned)p;
                a.k2[slot] = ((unsigned long long)(j - i + PROT_MAX_AA) << 32) | ((unsigned long long)i0 << 16) | (unsigned long long)i1;
            }
        }
    }
}
__global__ __launch_bounds__(256) void prot_iota_kernel(unsigned *__restrict__ v, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) v[k] = (unsigned)k;
}
__global__ __launch_bounds__(256) void prot_gather_kernel(const unsigned long long *__restrict__ in, const unsigned *__restrict__ idx, int64_t n,
                                                          unsigned long long *__restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) out[k] = in[idx[k]];
}
__global__ __launch_bounds__(256) void prot_unique_flag_kernel(const unsigned long long *__restrict__ k1, const unsigned long long *__restrict__ k2,
                                                               int64_t n, int32_t *__restrict__ flag) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256)
        flag[k] = (k == 0 || k1[k] != k1[k - 1] || k2[k] != k2[k - 1]) ? 1 : 0;
}
__global__ __launch_bounds__(256) void prot_unique_compact_kernel(const unsigned long long *__restrict__ k1, const unsigned long long *__restrict__ k2,
                                                                  const int32_t *__restrict__ flag, const int64_t *__restrict__ pos, int64_t n,
                                                                  unsigned long long *__restrict__ o1, unsigned long long *__restrict__ o2) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256)
        if (flag[k]) { o1[pos[k]] = k1[k]; o2[pos[k]] = k2[k]; }
}

// ---- gapped alignment ---------------------------------------------------------------------------------------------------------------
struct ProtTask { int32_t gf, prot, c, lo, hi, smin, pad0, pad1; };   // frame rows lo .. hi (inclusive), band c - 24 .. c + 39

// One wavefront per task; lane l owns diagonal d = c - 24 + l and computes row i at step 2 (i - lo) + l.  At the start of that step
// its own registers hold (i-1, d) = the diagonal predecessor, lane l+1's hold (i-1, d+1) = the cell above (E: a gap in the protein)
// and lane l-1's hold (i, d-1) = the cell to the left (F: a gap in the frame); a cell that does not exist leaves zeros.  A value of 0
// means "no alignment ends here".  Payload of H, E and F: start cell (i << 16 | j) and identical columns | columns << 32.
__global__ __launch_bounds__(PROT_WAVES * 64) void prot_gapped_kernel(const ProtTask *__restrict__ tasks, int64_t n_tasks,
                                                                      const uint8_t *__restrict__ fr, const int64_t *__restrict__ frame_off,
                                                                      const uint8_t *__restrict__ aa, const int64_t *__restrict__ aa_off,
                                                                      int32_t *__restrict__ out) {
    __shared__ int8_t tab[PROT_TABW * PROT_TABW];
    prot_fill_tab(tab);
    const int lane = lane_id(), w = wave_id();
    const unsigned long long ONE_COL = 1ull << 32;
    for (int64_t k = (int64_t)blockIdx.x * PROT_WAVES + w; k < n_tasks; k += (int64_t)gridDim.x * PROT_WAVES) {
        const ProtTask T = tasks[k];
        const uint8_t *x = fr + frame_off[T.gf], *y = aa + aa_off[T.prot];
        const int ly = (int)(aa_off[T.prot + 1] - aa_off[T.prot]);
        const int d = T.c - PROT_BAND_LO + lane, rows = T.hi - T.lo + 1;
        int H = 0, E = 0, F = 0;
        unsigned Hs = 0, Es = 0, Fs = 0;
        unsigned long long Hp = 0, Ep = 0, Fp = 0;
        int best = 0, bi = 0, bj = 0;
        unsigned bs = 0;
        unsigned long long bp = 0;
        const int steps = 2 * rows + 62;
        for (int t = 0; t < steps; t++) {
            int uH = __shfl_down(H, 1, 64), uE = __shfl_down(E, 1, 64);
            const unsigned uHs = __shfl_down(Hs, 1, 64), uEs = __shfl_down(Es, 1, 64);
            const unsigned long long uHp = __shfl_down(Hp, 1, 64), uEp = __shfl_down(Ep, 1, 64);
            int lH = __shfl_up(H, 1, 64), lF = __shfl_up(F, 1, 64);
            const unsigned lHs = __shfl_up(Hs, 1, 64), lFs = __shfl_up(Fs, 1, 64);
            const unsigned long long lHp = __shfl_up(Hp, 1, 64), lFp = __shfl_up(Fp, 1, 64);
            if (lane == 63) { uH = 0; uE = 0; }
            if (lane == 0) { lH = 0; lF = 0; }
            const int tt = t - lane;
            if (tt < 0 || (tt & 1) || (tt >> 1) >= rows) continue;
            const int i = T.lo + (tt >> 1), j = i + d;
            if (j < 0 || j >= ly) { H = 0; E = 0; F = 0; continue; }
            const int ca = x[i], cb = y[j];
            const unsigned long long idt = (ca == cb && ca < 20) ? 1ull : 0ull;
            // diagonal: extends the alignment that ends in (i-1, j-1), or starts one here
            const int Dv = H + tab[ca * PROT_TABW + cb];
            const unsigned Ds = H > 0 ? Hs : ((unsigned)i << 16 | (unsigned)j);
            const unsigned long long Dp = (H > 0 ? Hp : 0ull) + idt + ONE_COL;
            // E: a gap in the protein (from the cell above); opening preferred over extending
            int Ev; unsigned Es_; unsigned long long Ep_;
            if (uH - PROT_GAP_OPEN >= uE - PROT_GAP_EXT) { Ev = uH - PROT_GAP_OPEN; Es_ = uHs; Ep_ = uHp + ONE_COL; }
            else { Ev = uE - PROT_GAP_EXT; Es_ = uEs; Ep_ = uEp + ONE_COL; }
            if (Ev < 0) Ev = 0;
            // F: a gap in the frame (from the cell to the left)
            int Fv; unsigned Fs_; unsigned long long Fp_;
            if (lH - PROT_GAP_OPEN >= lF - PROT_GAP_EXT) { Fv = lH - PROT_GAP_OPEN; Fs_ = lHs; Fp_ = lHp + ONE_COL; }
            else { Fv = lF - PROT_GAP_EXT; Fs_ = lFs; Fp_ = lFp + ONE_COL; }
            if (Fv < 0) Fv = 0;
            // H: diagonal, then E, then F
            int h; unsigned hs; unsigned long long hp;
            if (Dv >= Ev && Dv >= Fv) { h = Dv; hs = Ds; hp = Dp; }
            else if (Ev >= Fv) { h = Ev; hs = Es_; hp = Ep_; }
            else { h = Fv; hs = Fs_; hp = Fp_; }
            if (h < 0) h = 0;
            H = h; Hs = hs; Hp = hp;
            E = Ev; Es = Es_; Ep = Ep_;
            F = Fv; Fs = Fs_; Fp = Fp_;
            if (h > best) { best = h; bi = i; bj = j; bs = hs; bp = hp; }
        }
        // the first maximum in row-major order: largest score, then smallest i, then smallest j
        unsigned long long key = ((unsigned long long)(unsigned)best << 32) | ((unsigned)(0xFFFF - bi) << 16) | (unsigned)(0xFFFF - bj);
        unsigned long long top = key;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned long long other = __shfl_xor(top, s, 64);
            top = other > top ? other : top;
        }
        int32_t *o = out + 8 * k;
        if ((top >> 32) == 0) {
            if (lane < 8) o[lane] = 0;
        } else if (key == top) {       // (i, j) is unique to one lane
            o[0] = best; o[1] = (int32_t)(bs >> 16); o[2] = (int32_t)(bs & 0xFFFF); o[3] = bi; o[4] = bj;
            o[5] = (int32_t)(bp & 0xFFFFFFFFull); o[6] = (int32_t)(bp >> 32); o[7] = best >= T.smin ? 1 : 0;
        }
    }
}

// ---- host: library handle ----------------------------------------------------------------------------------------------------------
struct ProtLib {
    hite_ctx *ctx = nullptr;
    int64_t n_prot = 0, n_res = 0;
    std::vector<int64_t> h_aa_off;
    uint8_t *d_aa = nullptr;          // residue codes (+ 16 bytes)
    int64_t *d_aa_off = nullptr;
    int32_t *d_prot_of = nullptr;
    int64_t *d_dir = nullptr;         // PROT_BUCKETS + 1
    unsigned *d_ent = nullptr;        // library positions by (bucket, position)
    Arena arena;                      // temporaries of the build and of every search
};

static inline unsigned prot_grid(int64_t n, int per_block) {
    int64_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > 256 * 32) b = 256 * 32;
    return (unsigned)b;
}

extern "C" void hite_protein_lib_release(void *state) {
    ProtLib *L = (ProtLib *)state;
    if (!L) return;
    if (L->ctx) (void)hipSetDevice(L->ctx->device);
    if (L->d_aa) (void)hipFree(L->d_aa);
    if (L->d_aa_off) (void)hipFree(L->d_aa_off);
    if (L->d_prot_of) (void)hipFree(L->d_prot_of);
    if (L->d_dir) (void)hipFree(L->d_dir);
    if (L->d_ent) (void)hipFree(L->d_ent);
    arena_free(L->arena);
    delete L;
}

static int prot_lib_build(hite_ctx *ctx, ProtLib *L, const uint8_t *aa, const int64_t *aa_off) {
    const int64_t N = L->n_res, P = L->n_prot;
    hipStream_t st = nullptr;
    HITE_CHECK(ctx, hipMalloc((void **)&L->d_aa, (size_t)N + 16));
    HITE_CHECK(ctx, hipMalloc((void **)&L->d_aa_off, (size_t)(P + 1) * 8));
    HITE_CHECK(ctx, hipMalloc((void **)&L->d_prot_of, (size_t)(N + 1) * 4));
    HITE_CHECK(ctx, hipMalloc((void **)&L->d_dir, (size_t)(PROT_BUCKETS + 1) * 8));
    HITE_CHECK(ctx, hipMalloc((void **)&L->d_ent, (size_t)(N + 1) * 4));
    HITE_CHECK(ctx, hipMemset(L->d_aa, PROT_X, (size_t)N + 16));
    HITE_CHECK(ctx, hipMemcpy(L->d_aa_off, aa_off, (size_t)(P + 1) * 8, hipMemcpyHostToDevice));
    HITE_CHECK(ctx, hipMemset(L->d_dir, 0, (size_t)(PROT_BUCKETS + 1) * 8));
    if (N == 0) return HITE_OK;
    int rc;
    uint8_t *d_raw; unsigned long long *d_keys; int32_t *d_cnt; int64_t *d_bs;
    HITE_TRY(arena_get(ctx, L->arena, (size_t)N, &d_raw));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(N + 1), &d_keys));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)PROT_BUCKETS, &d_cnt));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)scan_tmp_elems(PROT_BUCKETS), &d_bs));
    HITE_CHECK(ctx, hipMemcpy(d_raw, aa, (size_t)N, hipMemcpyHostToDevice));
    HITE_CHECK(ctx, hipMemsetAsync(d_cnt, 0, (size_t)PROT_BUCKETS * 4, st));
    int tk = hite_prof_begin(ctx, "prot_kmer_kernel", st);
    hipLaunchKernelGGL(prot_encode_kernel, dim3(prot_grid(N, 256)), dim3(256), 0, st, d_raw, N, L->d_aa);
    hipLaunchKernelGGL(prot_kmer_kernel, dim3(prot_grid(N, 256)), dim3(256), 0, st, L->d_aa, L->d_aa_off, P, L->d_prot_of, d_keys, L->d_ent, d_cnt);
    hite_prof_end(ctx, tk, st);
    HITE_CHECK(ctx, hipGetLastError());
    if ((rc = scan_excl_buf<int32_t>(ctx, d_bs, d_cnt, PROT_BUCKETS, L->d_dir, st))) return rc;
    // the fill: a stable sort by bucket leaves every bucket's entries in position order (positions without a seed go behind them all)
    Sorter S;
    HITE_TRY(sorter_init_in(S, ctx, &L->arena, st, N));
    tk = hite_prof_begin(ctx, "prot_index_sort", st);
    rc = sorter_sort(S, d_keys, L->d_ent, N, 18);
    hite_prof_end(ctx, tk, st);
    if (rc) return rc;
    HITE_CHECK(ctx, hipDeviceSynchronize());
    return HITE_OK;
}

extern "C" int hite_protein_lib_build(hite_ctx *ctx, int64_t n_prot, const uint8_t *aa, const int64_t *aa_off, void **state_io) {
    if (!ctx || !state_io || n_prot < 0 || !aa_off || aa_off[0] != 0) return HITE_EINVAL;
    for (int64_t p = 0; p < n_prot; p++) {
        const int64_t l = aa_off[p + 1] - aa_off[p];
        if (l < 0 || l > PROT_MAX_AA) return HITE_EINVAL;
    }
    if (n_prot >= ((int64_t)1 << 31) || aa_off[n_prot] >= ((int64_t)1 << 31) || (aa_off[n_prot] > 0 && !aa)) return HITE_EINVAL;
    HITE_CHECK(ctx, hipSetDevice(ctx->device));
    if (*state_io) { hite_protein_lib_release(*state_io); *state_io = nullptr; }
    ProtLib *L = new (std::nothrow) ProtLib();
    if (!L) return HITE_ENOMEM;
    L->ctx = ctx; L->n_prot = n_prot; L->n_res = aa_off[n_prot];
    L->h_aa_off.assign(aa_off, aa_off + n_prot + 1);
    int rc = prot_lib_build(ctx, L, aa, aa_off);
    if (rc == HITE_OK) rc = arena_reset(ctx, L->arena, false);
    if (rc) { hite_protein_lib_release(L); return rc; }
    *state_io = L;
    return HITE_OK;
}

// ---- host: translation -----------------------------------------------------------------------------------------------------------------
// frame_off[6 n + 1]; HITE_EINVAL when a query is longer than 3 x 65 535 bases
static int prot_frame_offsets(int64_t n, const int64_t *nt_off, int64_t *frame_off) {
    frame_off[0] = 0;
    for (int64_t q = 0; q < n; q++) {
        const int64_t L = nt_off[q + 1] - nt_off[q];
        if (L < 0 || L > 3 * (int64_t)PROT_MAX_AA) return HITE_EINVAL;
        for (int f = 0; f < 6; f++) {
            const int64_t lf = L >= (f % 3) ? (L - (f % 3)) / 3 : 0;
            frame_off[6 * q + f + 1] = frame_off[6 * q + f] + lf;
        }
    }
    return HITE_OK;
}

extern "C" int hite_translate6(hite_ctx *ctx, int64_t n, const uint8_t *nt, const int64_t *nt_off, int64_t cap, uint8_t *aa_out,
                               int64_t *frame_off) {
    if (!ctx || n < 0 || !frame_off || (n > 0 && !nt_off) || cap < 0) return HITE_EINVAL;
    frame_off[0] = 0;
    if (n == 0) return HITE_OK;
    int rc = prot_frame_offsets(n, nt_off, frame_off);
    if (rc) return rc;
    const int64_t R = frame_off[6 * n], nb = nt_off[n] - nt_off[0];
    if (R > cap) return HITE_ECAP;
    if (R == 0) return HITE_OK;
    if (!nt || !aa_out) return HITE_EINVAL;
    HITE_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf d_foff, d_off, d_out, d_nt;          // (freed d_nt, d_out, d_off, d_foff)
    std::vector<int64_t> rel(n + 1);
    for (int64_t q = 0; q <= n; q++) rel[q] = nt_off[q] - nt_off[0];
    hipError_t e = d_nt.alloc((size_t)nb + 16);
    if (e == hipSuccess) e = d_out.alloc((size_t)R);
    if (e == hipSuccess) e = d_off.alloc((size_t)(n + 1) * 8);
    if (e == hipSuccess) e = d_foff.alloc((size_t)(6 * n + 1) * 8);
    if (e == hipSuccess) e = hipMemcpy(d_nt.p, nt + nt_off[0], (size_t)nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_off.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_foff.p, frame_off, (size_t)(6 * n + 1) * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(prot_translate_kernel, dim3(prot_grid(R, 256)), dim3(256), 0, nullptr, d_nt.as<uint8_t>(), d_off.as<int64_t>(),
                           d_foff.as<int64_t>(), 6 * n, 1, d_out.as<uint8_t>());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(aa_out, d_out.p, (size_t)R, hipMemcpyDeviceToHost);
    HITE_CHECK(ctx, e);
    return HITE_OK;
}

// ---- host: threshold, tasks, HSP filter ------------------------------------------------------------------------------------------------
#define PROT_LAMBDA 0.267
#define PROT_K 0.041
static inline double prot_evalue(int64_t m, int64_t n, int32_t s) { return (double)m * (double)n * PROT_K * exp(-PROT_LAMBDA * (double)s); }

// the smallest integer raw score S >= 1 with m n K exp(-lambda S) <= evalue (binary64, no length adjustment)
extern "C" int hite_protein_smin(int64_t m, int64_t n, double evalue, int32_t *smin) {
    if (!smin || m < 0 || n < 0 || !(evalue > 0.0)) return HITE_EINVAL;
    int32_t s = 1;
    if (m > 0 && n > 0) {
        const double g = ceil(log((double)m * (double)n * PROT_K / evalue) / PROT_LAMBDA);
        if (g > 1e9) return HITE_EINVAL;
        if (g > 1.0) s = (int32_t)g;
        while (s > 1 && prot_evalue(m, n, s - 1) <= evalue) s--;      // (the logarithm may be off by one at a rounding boundary:
        while (prot_evalue(m, n, s) > evalue) s++;                      //  the exponential form decides)
    }
    *smin = s;
    return HITE_OK;
}

struct ProtSurv { int32_t gf, prot, d, i0, i1; };
struct ProtSeg { int32_t i0, i1; };

// survivors ordered by (frame, protein, diagonal, segment start, segment end), each once -> tasks, in that order of their groups
static void prot_form_tasks(int64_t n, const ProtSurv *sv, const int32_t *frame_len, std::vector<ProtTask> &tasks) {
    std::vector<ProtSeg> seg;
    int64_t a = 0;
    while (a < n) {
        const int32_t c = sv[a].d;
        int64_t b = a;
        seg.clear();
        while (b < n && sv[b].gf == sv[a].gf && sv[b].prot == sv[a].prot && sv[b].d <= c + PROT_DIAG_JOIN) {
            seg.push_back(ProtSeg{sv[b].i0, sv[b].i1});
            b++;
        }
        std::sort(seg.begin(), seg.end(), [](const ProtSeg &u, const ProtSeg &v) { return u.i0 != v.i0 ? u.i0 < v.i0 : u.i1 < v.i1; });
        const int32_t lf = frame_len[sv[a].gf];
        size_t k = 0;
        while (k < seg.size()) {
            const int32_t first = seg[k].i0;
            int32_t last = seg[k].i1;
            k++;
            while (k < seg.size() && seg[k].i0 - last <= PROT_SPLIT) { if (seg[k].i1 > last) last = seg[k].i1; k++; }
            ProtTask t;
            t.gf = sv[a].gf; t.prot = sv[a].prot; t.c = c;
            t.lo = first - PROT_SPLIT < 0 ? 0 : first - PROT_SPLIT;
            t.hi = last + PROT_SPLIT > lf - 1 ? lf - 1 : last + PROT_SPLIT;
            t.smin = 0; t.pad0 = 0; t.pad1 = 0;
            tasks.push_back(t);
        }
        a = b;
    }
}

extern "C" int hite_protein_tasks(int64_t n, const int32_t *frame, const int32_t *prot, const int32_t *diag, const int32_t *seg_start,
                                  const int32_t *seg_end, int64_t n_frames, const int32_t *frame_len, int64_t cap, int32_t *o_frame,
                                  int32_t *o_prot, int32_t *o_c, int32_t *o_lo, int32_t *o_hi, int64_t *n_out) {
    if (n < 0 || !n_out || (n > 0 && (!frame || !prot || !diag || !seg_start || !seg_end || !frame_len))) return HITE_EINVAL;
    std::vector<ProtSurv> sv((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        if (frame[k] < 0 || frame[k] >= n_frames) return HITE_EINVAL;
        sv[k] = ProtSurv{frame[k], prot[k], diag[k], seg_start[k], seg_end[k]};
    }
    std::vector<ProtTask> tasks;
    prot_form_tasks(n, sv.data(), frame_len, tasks);
    *n_out = (int64_t)tasks.size();
    const int64_t w = *n_out < cap ? *n_out : cap;
    for (int64_t k = 0; k < w; k++) {
        o_frame[k] = tasks[k].gf; o_prot[k] = tasks[k].prot; o_c[k] = tasks[k].c; o_lo[k] = tasks[k].lo; o_hi[k] = tasks[k].hi;
    }
    return *n_out > cap ? HITE_ECAP : HITE_OK;
}

struct ProtHsp { int32_t gf, prot, score, si, sj, ei, ej, ident, cols; };

// the HSPs of one (frame, protein) group: ordered by (score descending, frame start, protein start, frame end, protein end); one is
// dropped when it shares its start cell or its end cell with a kept one or lies inside a kept one on both sequences.  keep[k] for the
// input order.
static void prot_filter_group(int64_t n, const ProtHsp *h, uint8_t *keep) {
    std::vector<int64_t> ord((size_t)n);
    for (int64_t k = 0; k < n; k++) { ord[k] = k; keep[k] = 0; }
    std::sort(ord.begin(), ord.end(), [h](int64_t a, int64_t b) {
        if (h[a].score != h[b].score) return h[a].score > h[b].score;
        if (h[a].si != h[b].si) return h[a].si < h[b].si;
        if (h[a].sj != h[b].sj) return h[a].sj < h[b].sj;
        if (h[a].ei != h[b].ei) return h[a].ei < h[b].ei;
        if (h[a].ej != h[b].ej) return h[a].ej < h[b].ej;
        return a < b;
    });
    std::vector<int64_t> kept;
    for (int64_t o : ord) {
        const ProtHsp &c = h[o];
        bool drop = false;
        for (int64_t q : kept) {
            const ProtHsp &k = h[q];
            if ((c.si == k.si && c.sj == k.sj) || (c.ei == k.ei && c.ej == k.ej) ||
                (c.si >= k.si && c.ei <= k.ei && c.sj >= k.sj && c.ej <= k.ej)) { drop = true; break; }
        }
        if (!drop) { kept.push_back(o); keep[o] = 1; }
    }
}

extern "C" int hite_protein_hsp_filter(int64_t n, const int32_t *score, const int32_t *f_start, const int32_t *p_start, const int32_t *f_end,
                                       const int32_t *p_end, uint8_t *keep) {
    if (n < 0 || (n > 0 && (!score || !f_start || !p_start || !f_end || !p_end || !keep))) return HITE_EINVAL;
    std::vector<ProtHsp> h((size_t)n);
    for (int64_t k = 0; k < n; k++) h[k] = ProtHsp{0, 0, score[k], f_start[k], p_start[k], f_end[k], p_end[k], 0, 0};
    prot_filter_group(n, h.data(), keep);
    return HITE_OK;
}

// ---- host: the search -------------------------------------------------------------------------------------------------------------------
struct ProtOut { int32_t q, prot, f, qs, qe, ss, se, score, ident, cols; };

static int prot_search(hite_ctx *ctx, ProtLib *L, int64_t nq, const uint8_t *nt, const int64_t *nt_off, double evalue,
                       std::vector<ProtOut> &outv, int64_t *stats) {
    hipStream_t st = nullptr;
    int rc;
    const int64_t NF = 6 * nq;
    std::vector<int64_t> foff((size_t)NF + 1), rel((size_t)nq + 1);
    if ((rc = prot_frame_offsets(nq, nt_off, foff.data()))) return rc;
    std::vector<int32_t> smin((size_t)nq), flen((size_t)NF);
    for (int64_t q = 0; q < nq; q++) {
        rel[q] = nt_off[q] - nt_off[0];
        if ((rc = hite_protein_smin((nt_off[q + 1] - nt_off[q]) / 3, L->n_res, evalue, &smin[q]))) return rc;
    }
    rel[nq] = nt_off[nq] - nt_off[0];
    for (int64_t f = 0; f < NF; f++) flen[f] = (int32_t)(foff[f + 1] - foff[f]);
    const int64_t R = foff[NF], nb = rel[nq];
    if (R == 0 || L->n_res == 0) return HITE_OK;
    if ((rc = arena_reset(ctx, L->arena, true))) return rc;
    uint8_t *d_nt, *d_fr; int64_t *d_off, *d_foff, *d_hit_off, *d_bs; int32_t *d_key, *d_cnt;
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(nb + 16), &d_nt));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(R + 16), &d_fr));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(nq + 1), &d_off));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(NF + 1), &d_foff));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)R, &d_key, &d_cnt));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(R + 1), &d_hit_off));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)scan_tmp_elems(R), &d_bs));
    HITE_CHECK(ctx, hipMemcpy(d_nt, nt + nt_off[0], (size_t)nb, hipMemcpyHostToDevice));
    HITE_CHECK(ctx, hipMemcpy(d_off, rel.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    HITE_CHECK(ctx, hipMemcpy(d_foff, foff.data(), (size_t)(NF + 1) * 8, hipMemcpyHostToDevice));
    HITE_CHECK(ctx, hipMemsetAsync(d_fr + R, PROT_X, 16, st));
    int tk = hite_prof_begin(ctx, "prot_translate_kernel", st);
    hipLaunchKernelGGL(prot_translate_kernel, dim3(prot_grid(R, 256)), dim3(256), 0, st, d_nt, d_off, d_foff, NF, 0, d_fr);
    hite_prof_end(ctx, tk, st);
    tk = hite_prof_begin(ctx, "prot_seed_count_kernel", st);
    hipLaunchKernelGGL(prot_seed_count_kernel, dim3(prot_grid(R, 256)), dim3(256), 0, st, d_fr, d_foff, NF, L->d_dir, d_key, d_cnt);
    hite_prof_end(ctx, tk, st);
    HITE_CHECK(ctx, hipGetLastError());
    if ((rc = scan_excl_buf<int32_t>(ctx, d_bs, d_cnt, R, d_hit_off, st))) return rc;
    int64_t n_hits = 0;
    HITE_CHECK(ctx, hipMemcpy(&n_hits, d_hit_off + R, 8, hipMemcpyDeviceToHost));
    if (stats) stats[0] += n_hits;
    if (n_hits == 0) return HITE_OK;

    // ungapped filter; the survivors are counted exactly, so a second run with room for all of them is the only retry there can be
    unsigned long long *d_k1 = nullptr, *d_k2 = nullptr, *d_count;
    HITE_TRY(arena_get(ctx, L->arena, 1, &d_count));
    int64_t cap = n_hits < (1 << 20) ? n_hits : (1 << 20), n_surv = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        HITE_TRY(arena_get(ctx, L->arena, (size_t)(cap + 1), &d_k1, &d_k2));
        HITE_CHECK(ctx, hipMemsetAsync(d_count, 0, 8, st));
        ProtUngapArgs a;
        a.fr = d_fr; a.frame_off = d_foff; a.n_frames = NF; a.aa = L->d_aa; a.aa_off = L->d_aa_off; a.prot_of = L->d_prot_of;
        a.dir = L->d_dir; a.ent = L->d_ent; a.key = d_key; a.hit_off = d_hit_off; a.n_res = R; a.n_hits = n_hits;
        a.k1 = d_k1; a.k2 = d_k2; a.count = d_count; a.cap = cap;
        tk = hite_prof_begin(ctx, "prot_ungapped_kernel", st);
        hipLaunchKernelGGL(prot_ungapped_kernel, dim3(prot_grid(n_hits, 256)), dim3(256), 0, st, a);
        hite_prof_end(ctx, tk, st);
        HITE_CHECK(ctx, hipGetLastError());
        unsigned long long c = 0;
        HITE_CHECK(ctx, hipMemcpy(&c, d_count, 8, hipMemcpyDeviceToHost));
        n_surv = (int64_t)c;
        if (n_surv <= cap) break;
        if (n_surv >= 0xffffffffll) return HITE_ENOMEM;
        cap = n_surv;
    }
    if (n_surv == 0) return HITE_OK;

    // order (two stable stages: (diagonal, segment), then (frame, protein)) and keep each survivor once
    unsigned *d_idx; unsigned long long *d_g1, *d_g2, *d_u1, *d_u2; int32_t *d_flag; int64_t *d_pos, *d_bs2;
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(n_surv + 1), &d_idx, &d_g1, &d_g2, &d_u1, &d_u2));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)n_surv, &d_flag));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(n_surv + 1), &d_pos));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)scan_tmp_elems(n_surv), &d_bs2));
    Sorter S;
    HITE_TRY(sorter_init_in(S, ctx, &L->arena, st, n_surv));
    const unsigned gs = prot_grid(n_surv, 256);
    int fbits = 1;
    while (((int64_t)1 << fbits) < NF) fbits++;
    tk = hite_prof_begin(ctx, "prot_survivor_sort", st);
    hipLaunchKernelGGL(prot_iota_kernel, dim3(gs), dim3(256), 0, st, d_idx, n_surv);
    HITE_CHECK(ctx, hipMemcpyAsync(d_g2, d_k2, (size_t)n_surv * 8, hipMemcpyDeviceToDevice, st));
    if ((rc = sorter_sort(S, d_g2, d_idx, n_surv, 49))) return rc;
    hipLaunchKernelGGL(prot_gather_kernel, dim3(gs), dim3(256), 0, st, d_k1, d_idx, n_surv, d_g1);
    if ((rc = sorter_sort(S, d_g1, d_idx, n_surv, 32 + fbits))) return rc;
    hipLaunchKernelGGL(prot_gather_kernel, dim3(gs), dim3(256), 0, st, d_k2, d_idx, n_surv, d_g2);
    hipLaunchKernelGGL(prot_unique_flag_kernel, dim3(gs), dim3(256), 0, st, d_g1, d_g2, n_surv, d_flag);
    if ((rc = scan_excl_buf<int32_t>(ctx, d_bs2, d_flag, n_surv, d_pos, st))) return rc;
    hipLaunchKernelGGL(prot_unique_compact_kernel, dim3(gs), dim3(256), 0, st, d_g1, d_g2, d_flag, d_pos, n_surv, d_u1, d_u2);
    hite_prof_end(ctx, tk, st);
    HITE_CHECK(ctx, hipGetLastError());
    int64_t n_uniq = 0;
    HITE_CHECK(ctx, hipMemcpy(&n_uniq, d_pos + n_surv, 8, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> h1((size_t)n_uniq), h2((size_t)n_uniq);
    HITE_CHECK(ctx, hipMemcpy(h1.data(), d_u1, (size_t)n_uniq * 8, hipMemcpyDeviceToHost));
    HITE_CHECK(ctx, hipMemcpy(h2.data(), d_u2, (size_t)n_uniq * 8, hipMemcpyDeviceToHost));
    if (stats) stats[1] += n_uniq;

    // tasks
    std::vector<ProtSurv> sv((size_t)n_uniq);
    for (int64_t k = 0; k < n_uniq; k++)
        sv[k] = ProtSurv{(int32_t)(h1[k] >> 32), (int32_t)(h1[k] & 0xFFFFFFFFull), (int32_t)(h2[k] >> 32) - PROT_MAX_AA,
                         (int32_t)((h2[k] >> 16) & 0xFFFF), (int32_t)(h2[k] & 0xFFFF)};
    std::vector<ProtTask> tasks;
    prot_form_tasks(n_uniq, sv.data(), flen.data(), tasks);
    const int64_t n_tasks = (int64_t)tasks.size();
    for (ProtTask &t : tasks) t.smin = smin[t.gf / 6];
    if (stats) stats[2] += n_tasks;
    ProtTask *d_tasks; int32_t *d_res;
    HITE_TRY(arena_get(ctx, L->arena, (size_t)n_tasks, &d_tasks));
    HITE_TRY(arena_get(ctx, L->arena, (size_t)(n_tasks * 8), &d_res));
    HITE_CHECK(ctx, hipMemcpy(d_tasks, tasks.data(), (size_t)n_tasks * sizeof(ProtTask), hipMemcpyHostToDevice));
    tk = hite_prof_begin(ctx, "prot_gapped_kernel", st);
    hipLaunchKernelGGL(prot_gapped_kernel, dim3(prot_grid(n_tasks, PROT_WAVES)), dim3(PROT_WAVES * 64), 0, st, d_tasks, n_tasks, d_fr, d_foff,
                       L->d_aa, L->d_aa_off, d_res);
    hite_prof_end(ctx, tk, st);
    HITE_CHECK(ctx, hipGetLastError());
    std::vector<int32_t> res((size_t)n_tasks * 8);
    HITE_CHECK(ctx, hipMemcpy(res.data(), d_res, (size_t)n_tasks * 32, hipMemcpyDeviceToHost));
    hite_prof_resolve(ctx);

    // threshold flag -> filter per (frame, protein) -> coordinates
    std::vector<ProtHsp> grp;
    std::vector<uint8_t> keep;
    int64_t a = 0;
    while (a < n_tasks) {
        int64_t b = a;
        grp.clear();
        while (b < n_tasks && tasks[b].gf == tasks[a].gf && tasks[b].prot == tasks[a].prot) {
            const int32_t *o = &res[8 * b];
            if (o[7]) grp.push_back(ProtHsp{tasks[b].gf, tasks[b].prot, o[0], o[1], o[2], o[3], o[4], o[5], o[6]});
            b++;
        }
        keep.resize(grp.size());
        prot_filter_group((int64_t)grp.size(), grp.data(), keep.data());
        for (size_t k = 0; k < grp.size(); k++) {
            if (!keep[k]) continue;
            const ProtHsp &h = grp[k];
            const int64_t q = h.gf / 6;
            const int f = h.gf % 6, o = f % 3;
            const int32_t Lq = (int32_t)(nt_off[q + 1] - nt_off[q]);
            ProtOut r;
            r.q = (int32_t)q; r.prot = h.prot; r.f = f;
            if (f < 3) { r.qs = o + 3 * h.si + 1; r.qe = o + 3 * h.ei + 3; }
            else { r.qs = Lq - (o + 3 * h.si); r.qe = Lq - (o + 3 * h.ei + 2); }
            r.ss = h.sj + 1; r.se = h.ej + 1; r.score = h.score; r.ident = h.ident; r.cols = h.cols;
            outv.push_back(r);
        }
        a = b;
    }
    return HITE_OK;
}

extern "C" int hite_protein_search(hite_ctx *ctx, void *state, int64_t n_query, const uint8_t *nt, const int64_t *nt_off, double evalue,
                                   int64_t cap, int32_t *o_query, int32_t *o_prot, int32_t *o_frame, int32_t *o_qstart, int32_t *o_qend,
                                   int32_t *o_sstart, int32_t *o_send, int32_t *o_score, int32_t *o_ident, int32_t *o_cols, int64_t *n_out,
                                   int64_t *stats) {
    ProtLib *L = (ProtLib *)state;
    if (!ctx || !L || L->ctx != ctx || n_query < 0 || cap < 0 || !n_out || !(evalue > 0.0) || (n_query > 0 && !nt_off)) return HITE_EINVAL;
    if (n_query >= ((int64_t)1 << 31) / 6) return HITE_EINVAL;
    if (cap > 0 && (!o_query || !o_prot || !o_frame || !o_qstart || !o_qend || !o_sstart || !o_send || !o_score || !o_ident || !o_cols))
        return HITE_EINVAL;
    *n_out = 0;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (n_query == 0) return HITE_OK;
    if (nt_off[n_query] - nt_off[0] > 0 && !nt) return HITE_EINVAL;
    HITE_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<ProtOut> outv;
    int rc;
    try {
        rc = prot_search(ctx, L, n_query, nt, nt_off, evalue, outv, stats);
    } catch (const std::bad_alloc &) {
        rc = HITE_ENOMEM;
    }
    if (rc) return rc;
    // final order: (query, score descending, protein, frame index, q_start, s_start)
    std::sort(outv.begin(), outv.end(), [](const ProtOut &a, const ProtOut &b) {
        if (a.q != b.q) return a.q < b.q;
        if (a.score != b.score) return a.score > b.score;
        if (a.prot != b.prot) return a.prot < b.prot;
        if (a.f != b.f) return a.f < b.f;
        if (a.qs != b.qs) return a.qs < b.qs;
        return a.ss < b.ss;
    });
    *n_out = (int64_t)outv.size();
    const int64_t w = *n_out < cap ? *n_out : cap;
    for (int64_t k = 0; k < w; k++) {
        const ProtOut &r = outv[k];
        o_query[k] = r.q; o_prot[k] = r.prot; o_frame[k] = r.f < 3 ? r.f + 1 : -(r.f - 2);
        o_qstart[k] = r.qs; o_qend[k] = r.qe; o_sstart[k] = r.ss; o_send[k] = r.se;
        o_score[k] = r.score; o_ident[k] = r.ident; o_cols[k] = r.cols;
    }
    return *n_out > cap ? HITE_ECAP : HITE_OK;
}

// hite_ltrscan.hip -- the LTR candidate scan: genome in, pairs of direct repeats out, where FiLTR runs the vendored LtrDetector and
// HiTE's other branch `gt ltrharvest` and LTR_FINDER.  None of the three is pinned (no machine of the project has them): parity is the
// written definition in include/hite_gpu.h ("LTR candidate scan"), its CPU twin tests/ltrscan_twin.py + tests/ltrscan_twin.c, HIP ==
// twin record for record and counter for counter.
//
// Whole sequences go up in batches of bounded bytes; per batch, positions are bytes of the batch (gp) and a sequence is found again
// through the batch's offsets --
//   1. words: one thread per position forms the 26-bit word (bit 26: no word there); the positions are sorted on those 27 bits with the
//      stable sort of hite_sort.h, so that the positions of a word stay ascending;
//   2. links: one thread per sorted entry looks at most 16 entries ahead (same word, same sequence); the hits (gp, d) are compacted
//      with one atomic per wavefront;
//   3. runs, once per lattice: the hits are sorted on (bin, gp) packed into one 64-bit key -- the sequences of a batch lie one after
//      the other in gp, so the chains of equal (seq, bin) are those of the header's order (seq, bin, i) --, head flags and a scan give
//      every hit its run, a segmented wavefront minimum / maximum of d gives one atomic per run and wavefront, one thread per run
//      applies the hit count and the span limit and emits the run as a task;
//   4. extension: ONE WAVEFRONT PER RUN in the lane layout of ph_align (hite_pairhsp.hip): 64 columns of a strip across the lanes,
//      wave shifts for the neighbours, the last column of a strip in 2 x 192 LDS cells of the wavefront; the redo loop of the pads
//      runs inside the wavefront.
// The filters, the order and the duplicates (steps 5 and 6) are host code.  hite_pairhsp.hip is left as it is: this file carries its
// own copy of the cell and of the strip routine.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include "hite_sort.h"
#include <algorithm>
#include <new>
#include <vector>

#define LS_WAVES 4
#define LS_BAND (HITE_LTRSCAN_BAND_BELOW + HITE_LTRSCAN_BAND_ABOVE)      // diagonals of the band
#define LS_BATCH_BYTES ((int64_t)64 << 20)       // sequence bytes per batch ($HITE_LTRSCAN_BATCH_BYTES overrides)
#define LS_NO_WORD ((unsigned long long)1 << 26)
#define LS_WORD_BITS 27
#define LS_OUT_WORDS 10                           // per run: seq, found, ls, le, rs, re, score, matches, columns, alignments
#define LS_MAX_BLOCKS 2048
#ifndef __host__
#define __host__
#endif

// >>> ltrscan_cell
// The cell of hite_pair_hsps, step 4 (a copy of the pairhsp_cell block of hite_pairhsp.hip).  A cell value (score, matches, columns,
// q_start, s_start) is TWO words.  a = score * 2^40 + matches * 2^20 + columns, signed: matches and columns stay below 2^20 (a window
// holds at most 3 * 8192 + 192 bases), so the integer order of a is the lexicographic order of the first three fields, a step is one
// addition and "score <= 0" is a < 2^40.  b = q_start * 2^16 + s_start (both < 32 768): on equal a the smaller b wins.  The empty
// value is (0, 0).
#define LS_SCORE_ONE ((int64_t)1 << 40)
#define LS_STEP_MATCH (HITE_PAIRHSP_MATCH * LS_SCORE_ONE + ((int64_t)1 << 20) + 1)
#define LS_STEP_MISMATCH (HITE_PAIRHSP_MISMATCH * LS_SCORE_ONE + 1)
#define LS_STEP_GAP (HITE_PAIRHSP_GAP * LS_SCORE_ONE + 1)
struct LsVal { int64_t a; uint32_t b; };
// a byte (either case) as a base code A 0 / C 1 / G 2 / T 3 / anything else 4
__device__ __forceinline__ int ls_code(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}
__device__ __forceinline__ bool ls_better(int64_t a1, uint32_t b1, int64_t a2, uint32_t b2) { return a1 > a2 || (a1 == a2 && b1 < b2); }
__device__ __forceinline__ LsVal ls_cell(LsVal diag, LsVal up, LsVal left, int ca, int cb, int i, int j) {
    LsVal v;
    v.a = diag.a + ((ca == cb && ca < 4) ? LS_STEP_MATCH : LS_STEP_MISMATCH);
    v.b = diag.a == 0 ? ((uint32_t)i << 16 | (uint32_t)j) : diag.b;
    const int64_t ua = up.a + LS_STEP_GAP, la = left.a + LS_STEP_GAP;
    if (ls_better(ua, up.b, v.a, v.b)) { v.a = ua; v.b = up.b; }
    if (ls_better(la, left.b, v.a, v.b)) { v.a = la; v.b = left.b; }
    if (v.a < LS_SCORE_ONE) { v.a = 0; v.b = 0; }
    return v;
}
// the best cell so far: its value and e = i * 2^16 + j; a later cell takes its place when its value is better, or equal at a smaller e
struct LsBest { int64_t a; uint32_t b, e; };
__device__ __forceinline__ bool ls_best_better(int64_t a, uint32_t b, uint32_t e, const LsBest &o) {
    return a > o.a || (a == o.a && (b < o.b || (b == o.b && e < o.e)));
}
// <<< ltrscan_cell

// >>> ltrscan_key
// the word of 13 base codes (the first one in the highest bits), or LS_NO_WORD when one of them is not in ACGT
__host__ __device__ __forceinline__ unsigned long long ls_word_key(const int *codes) {
    unsigned long long w = 0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < HITE_LTRSCAN_WORD; k++) { ok = ok && codes[k] < 4; w = w * 4 + (unsigned long long)(codes[k] & 3); }
    return ok ? w : ((unsigned long long)1 << 26);
}
// a hit on lattice lam (0 or HITE_LTRSCAN_LATTICE) as one key: its bin above the pos_bits bits of its position in the batch
__host__ __device__ __forceinline__ unsigned long long ls_hit_key(uint32_t gp, uint32_t d, int lam, int pos_bits) {
    return (((unsigned long long)d + (unsigned long long)lam) >> HITE_LTRSCAN_BIN_SHIFT) << pos_bits | (unsigned long long)gp;
}
__host__ __device__ __forceinline__ int64_t ls_key_pos(unsigned long long key, int pos_bits) { return (int64_t)(key & (((unsigned long long)1 << pos_bits) - 1)); }
__host__ __device__ __forceinline__ int64_t ls_key_bin(unsigned long long key, int pos_bits) { return (int64_t)(key >> pos_bits); }
// bits that hold every value 0 .. v
__host__ __device__ __forceinline__ int ls_bits(unsigned long long v) { int b = 1; while (b < 64 && (v >> b) != 0) b++; return b; }
// the pad of level k = 0 .. 3
__host__ __device__ __forceinline__ int ls_pad(int k, int max_ltr) {
    const int p = k == 0 ? HITE_LTRSCAN_PAD_0 : k == 1 ? HITE_LTRSCAN_PAD_1 : k == 2 ? HITE_LTRSCAN_PAD_2 : max_ltr;
    return p < max_ltr ? p : max_ltr;
}
// the two windows of a run at the pad levels pl, pr: Q = [qb, qe), S = [sb, se), and the lowest diagonal j - i of the band in the
// 1-based coordinates of the windows (the highest is dlo + 191)
struct LsWin { int64_t qb, qe, sb, se; int dlo; };
__host__ __device__ __forceinline__ LsWin ls_window(int64_t len, int64_t i_lo, int64_t i_hi, int64_t dc, int pl, int pr, int max_ltr) {
    LsWin w;
    w.qb = i_lo - ls_pad(pl, max_ltr); if (w.qb < 0) w.qb = 0;
    w.qe = i_hi + HITE_LTRSCAN_WORD + ls_pad(pr, max_ltr); if (w.qe > len) w.qe = len;
    w.sb = w.qb + dc - HITE_LTRSCAN_BAND_BELOW; if (w.sb < 0) w.sb = 0;
    w.se = w.qe + dc + HITE_LTRSCAN_BAND_ABOVE; if (w.se > len) w.se = len;
    w.dlo = (int)(dc - HITE_LTRSCAN_BAND_BELOW - (w.sb - w.qb));
    return w;
}
// which pads step after an HSP [ls, le) of Q: bit 0 the left one, bit 1 the right one
__host__ __device__ __forceinline__ int ls_pad_steps(const LsWin &w, int64_t len, int64_t ls, int64_t le, int pl, int pr) {
    int s = 0;
    if (ls - w.qb < HITE_LTRSCAN_EDGE && w.qb > 0 && pl < 3) s |= 1;
    if (w.qe - le < HITE_LTRSCAN_EDGE && w.qe < len && pr < 3) s |= 2;
    return s;
}
// <<< ltrscan_key

// >>> ltrscan_filter
// step 5 on a record (seq, ls, le, rs, re, score, matches, columns): 0 = kept, else the number 1 .. 4 of the first filter it fails
__host__ __device__ __forceinline__ int ls_filter(const int32_t *r, int32_t min_len, int32_t max_len, int32_t min_ltr, int32_t max_ltr, int32_t identity) {
    const int64_t ls = r[1], le = r[2], rs = r[3], re = r[4];
    if (le - ls < min_ltr || le - ls > max_ltr || re - rs < min_ltr || re - rs > max_ltr) return 1;
    if (re - ls < min_len || re - ls > max_len) return 2;
    if (le > rs) return 3;
    if ((int64_t)100 * r[6] < (int64_t)identity * r[7]) return 4;
    return 0;
}
// step 6: (seq, ls, re, le, rs, -score, -matches, columns)
__host__ __device__ __forceinline__ bool ls_rec_less(const int32_t *x, const int32_t *y) {
    if (x[0] != y[0]) return x[0] < y[0];
    if (x[1] != y[1]) return x[1] < y[1];
    if (x[4] != y[4]) return x[4] < y[4];
    if (x[2] != y[2]) return x[2] < y[2];
    if (x[3] != y[3]) return x[3] < y[3];
    if (x[5] != y[5]) return x[5] > y[5];
    if (x[6] != y[6]) return x[6] > y[6];
    return x[7] < y[7];
}
__host__ __device__ __forceinline__ bool ls_rec_same_place(const int32_t *x, const int32_t *y) {
    return x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3] && x[4] == y[4];
}
// <<< ltrscan_filter

struct LsTask { int32_t seq, i_lo, i_hi, d_lo, d_hi; };      // a run: the sequence of the batch, positions inside it
enum { LS_C_WORDS = 0, LS_C_HITS, LS_C_RUNS, LS_C_SPAN, LS_C_TASKS, LS_C_N };

// the sequence of the batch that holds byte gp: the last q with off[q] <= gp (off[0] = 0 <= gp < off[n]; empty sequences are stepped over)
__device__ __forceinline__ int ls_seq_of(const int64_t *__restrict__ off, int n, int64_t gp) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= gp) lo = mid; else hi = mid;
    }
    return lo;
}

// adds the number of lanes with `flag` to *counter with one atomic per wavefront; returns the lane's place among them (every lane of
// the wavefront must come here)
__device__ __forceinline__ unsigned long long ls_wave_take(bool flag, unsigned long long *counter) {
    const unsigned long long mask = __ballot(flag);
    const int lane = lane_id();
    unsigned long long base = 0;
    if (lane == 0 && mask) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    base = (unsigned long long)__shfl((long long)base, 0, 64);
    return base + (unsigned long long)__popcll(mask & (((unsigned long long)1 << lane) - 1));
}

__global__ __launch_bounds__(256) void ls_word_kernel(const uint8_t *__restrict__ seqs, const int64_t *__restrict__ off, int n_seq, int64_t nb,
                                                      unsigned long long *__restrict__ keys, unsigned *__restrict__ vals,
                                                      unsigned long long *__restrict__ counters) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long key = LS_NO_WORD;
    if (p < nb) {
        const int q = ls_seq_of(off, n_seq, p);
        if (p + HITE_LTRSCAN_WORD <= off[q + 1]) {
            int codes[HITE_LTRSCAN_WORD];
#pragma unroll
            for (int k = 0; k < HITE_LTRSCAN_WORD; k++) codes[k] = ls_code(seqs[p + k]);
            key = ls_word_key(codes);
        }
        keys[p] = key;
        vals[p] = (unsigned)p;
    }
    (void)ls_wave_take(key != LS_NO_WORD, &counters[LS_C_WORDS]);
}

// entry e of the sorted words: the first of the next HITE_LTRSCAN_MAX_OCC entries of the same word and sequence at a distance >= dmin is
// its link, a hit when the distance is <= dmax
__global__ __launch_bounds__(256) void ls_link_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ vals, int64_t nb,
                                                      const int64_t *__restrict__ off, int n_seq, int64_t dmin, int64_t dmax,
                                                      unsigned *__restrict__ hit_gp, unsigned *__restrict__ hit_d,
                                                      unsigned long long *__restrict__ counters) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    int64_t i = 0, d = 0;
    if (e < nb) {
        const unsigned long long w = keys[e];
        if (w != LS_NO_WORD) {
            i = vals[e];
            const int64_t end = off[ls_seq_of(off, n_seq, i) + 1];
            for (int t = 1; t <= HITE_LTRSCAN_MAX_OCC; t++) {
                if (e + t >= nb || keys[e + t] != w) break;
                const int64_t j = vals[e + t];
                if (j >= end) break;
                d = j - i;
                if (d >= dmin) { hit = d <= dmax; break; }
            }
        }
    }
    const unsigned long long at = ls_wave_take(hit, &counters[LS_C_HITS]);
    if (hit) { hit_gp[at] = (unsigned)i; hit_d[at] = (unsigned)d; }      // at most one hit per entry: at < nb
}

__global__ __launch_bounds__(256) void ls_hit_key_kernel(const unsigned *__restrict__ hit_gp, const unsigned *__restrict__ hit_d, int64_t nh, int lam,
                                                         int pos_bits, unsigned long long *__restrict__ keys, unsigned *__restrict__ vals) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    keys[h] = ls_hit_key(hit_gp[h], hit_d[h], lam, pos_bits);
    vals[h] = hit_d[h];
}

// 1 where a run begins: another bin, another sequence, or more than HITE_LTRSCAN_GAP after the hit before
__global__ __launch_bounds__(256) void ls_head_kernel(const unsigned long long *__restrict__ keys, int64_t nh, int pos_bits,
                                                      const int64_t *__restrict__ off, int n_seq, int32_t *__restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    bool head = h == 0;
    if (!head) {
        const unsigned long long k = keys[h], kp = keys[h - 1];
        const int64_t gp = ls_key_pos(k, pos_bits), gpp = ls_key_pos(kp, pos_bits);
        head = ls_key_bin(k, pos_bits) != ls_key_bin(kp, pos_bits) || gp - gpp > HITE_LTRSCAN_GAP ||
               off[ls_seq_of(off, n_seq, gp)] > gpp;
    }
    flags[h] = head ? 1 : 0;
}

// every hit: its run r = (heads up to and with it) - 1; the head writes start[r]; the smallest and the largest d of the run's hits in
// this wavefront go to d_lo[r] / d_hi[r] by one atomic each (the runs of a wavefront's hits ascend: a segmented scan over the lanes)
__global__ __launch_bounds__(256) void ls_run_fill_kernel(const unsigned *__restrict__ vals, const int32_t *__restrict__ flags,
                                                          const int64_t *__restrict__ excl, int64_t nh, int64_t n_runs,
                                                          unsigned *__restrict__ start, int *__restrict__ d_lo, int *__restrict__ d_hi) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    const bool act = h < nh;
    long long r = -1;
    int lo = 0, hi = 0;
    if (act) {
        r = excl[h] + flags[h] - 1;
        lo = hi = (int)vals[h];
        if (flags[h]) start[r] = (unsigned)h;
        if (h == nh - 1) start[n_runs] = (unsigned)nh;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const long long r2 = __shfl_up(r, s, 64);
        const int lo2 = __shfl_up(lo, s, 64), hi2 = __shfl_up(hi, s, 64);
        if (lane >= s && r2 == r) { lo = min(lo, lo2); hi = max(hi, hi2); }
    }
    const long long rn = __shfl_down(r, 1, 64);
    if (act && (lane == 63 || rn != r)) { atomicMin(&d_lo[r], lo); atomicMax(&d_hi[r], hi); }
}

// one thread per run: the hit count, the span limit, the task
__global__ __launch_bounds__(256) void ls_run_emit_kernel(const unsigned long long *__restrict__ keys, int pos_bits, const unsigned *__restrict__ start,
                                                          const int *__restrict__ d_lo, const int *__restrict__ d_hi, int64_t n_runs,
                                                          const int64_t *__restrict__ off, int n_seq, int max_ltr, LsTask *__restrict__ tasks,
                                                          int64_t task_cap, unsigned long long *__restrict__ counters) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool counted = false, wide = false;
    LsTask T = {0, 0, 0, 0, 0};
    if (r < n_runs) {
        const unsigned a = start[r], b = start[r + 1];
        if (b - a >= HITE_LTRSCAN_MIN_HITS) {
            counted = true;
            const int64_t g_lo = ls_key_pos(keys[a], pos_bits), g_hi = ls_key_pos(keys[b - 1], pos_bits);
            wide = g_hi - g_lo + HITE_LTRSCAN_WORD > max_ltr;
            const int q = ls_seq_of(off, n_seq, g_lo);
            T.seq = q; T.i_lo = (int32_t)(g_lo - off[q]); T.i_hi = (int32_t)(g_hi - off[q]); T.d_lo = d_lo[r]; T.d_hi = d_hi[r];
        }
    }
    (void)ls_wave_take(counted, &counters[LS_C_RUNS]);
    (void)ls_wave_take(wide, &counters[LS_C_SPAN]);
    const bool go = counted && !wide;
    const unsigned long long at = ls_wave_take(go, &counters[LS_C_TASKS]);
    if (go && (int64_t)at < task_cap) tasks[at] = T;
}

// lane l takes the value of lane l - 1 (wave_shr1), lane 0 gets 0 and the caller puts its own value there
__device__ __forceinline__ LsVal ls_up1(LsVal v) {
    LsVal r;
    const uint32_t lo = (uint32_t)wave_shr1((int)(uint32_t)v.a), hi = (uint32_t)wave_shr1((int)(uint32_t)((uint64_t)v.a >> 32));
    r.a = (int64_t)((uint64_t)hi << 32 | lo);
    r.b = (uint32_t)wave_shr1((int)v.b);
    return r;
}

__device__ __forceinline__ LsBest ls_wave_best(LsBest v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        LsBest y;
        y.a = __shfl_xor((long long)v.a, d, 64);
        y.b = __shfl_xor(v.b, d, 64);
        y.e = __shfl_xor(v.e, d, 64);
        if (ls_best_better(y.a, y.b, y.e, v)) v = y;
    }
    return v;
}

// The best cell of rows r0 .. r1 and columns c0 .. c1 (1-based, inside [1, m] x [1, n]) within the band dlo <= j - i <= dhi
// (dhi - dlo < LS_BAND), by one wavefront; q / s: the bytes of the two windows; bnd_a / bnd_b: 2 x LS_BAND words of the wavefront.  The
// strip routine of ph_align (hite_pairhsp.hip): lane l is on row first + d - 1 - l at step d; the cell above is the lane's own last
// value, the cell to the left the last value of lane l - 1, the diagonal cell what lane l - 1 handed over one step earlier.  All lanes
// return the same value; a == 0: no cell has a positive score.
__device__ __forceinline__ LsBest ls_align(const uint8_t *q, int m, const uint8_t *s, int dlo, int dhi, int r0, int r1, int c0, int c1,
                                           long long *bnd_a, uint32_t *bnd_b) {
    const int lane = lane_id();
    LsBest best = {0, 0, 0};
    const int cs = max(c0, r0 + dlo), ce = min(c1, r1 + dhi);      // the columns the band reaches inside the rectangle
    int buf = 0;
    for (int js = cs; js <= ce; js += 64, buf ^= 1) {
        const int nl = min(64, ce - js + 1);
        const bool more = js + 64 <= ce;
        const int first = max(r0, js - dhi), last = min(r1, js + nl - 1 - dlo);      // the rows where the band meets the strip
        const int ib = first - 1, j = js + lane;
        const int cb = lane < nl ? ls_code(s[j - 1]) : 4;
        const long long *rd_a = bnd_a + (buf ^ 1) * LS_BAND;
        const uint32_t *rd_b = bnd_b + (buf ^ 1) * LS_BAND;
        long long *wr_a = bnd_a + buf * LS_BAND;
        uint32_t *wr_b = bnd_b + buf * LS_BAND;
        // V(row, js - 1): the last column of the strip before, the empty value outside the band or the rectangle
        auto edge = [&](int row) {
            LsVal v = {0, 0};
            const int dd = js - 1 - row;
            if (js > cs && row >= r0 && row <= r1 && dd >= dlo && dd <= dhi) { v.a = (int64_t)rd_a[dhi - dd]; v.b = rd_b[dhi - dd]; }
            return v;
        };
        LsVal cur = {0, 0}, diag = {0, 0};
        if (lane == 0) diag = edge(ib);
        LsVal ahead = edge(ib + 1);      // lane 0's left neighbour of the next step
        int ca = 4, a64 = 4;             // the lane's base of Q; Q[ib + 64 k + lane] of the current 64 rows
        const int steps = last - ib + nl - 1;
        for (int d = 1; d <= steps; d++) {
            const int i = ib + d - lane;
            if (((d - 1) & 63) == 0) {
                const int r = ib + d + lane;
                a64 = (r >= 1 && r <= m) ? ls_code(q[r - 1]) : 4;
            }
            const int a_new = __builtin_amdgcn_readlane(a64, (d - 1) & 63);      // the code of row ib + d
            ca = wave_shr1(ca);
            LsVal left = ls_up1(cur);
            if (lane == 0) { ca = a_new; left = ahead; }
            ahead = edge(ib + d + 1);
            const bool on = lane < nl && i >= r0 && i <= r1 && j - i >= dlo && j - i <= dhi;
            LsVal v = ls_cell(diag, cur, left, ca, cb, i, j);
            diag = left;
            if (!on) { v.a = 0; v.b = 0; }
            cur = v;
            if (on) {
                const uint32_t e = (uint32_t)i << 16 | (uint32_t)j;
                if (v.a > 0 && ls_best_better(v.a, v.b, e, best)) { best.a = v.a; best.b = v.b; best.e = e; }
                if (more && lane == 63) { wr_a[dhi - (j - i)] = (long long)v.a; wr_b[dhi - (j - i)] = v.b; }
            }
        }
        __threadfence_block();          // lane 0 of the next strip reads what lane 63 wrote
    }
    return ls_wave_best(best);
}

// wavefront per run: step 4 of the header with its redo loop
__global__ __launch_bounds__(LS_WAVES * 64) void ls_extend_kernel(const LsTask *__restrict__ tasks, int64_t n_tasks, const uint8_t *__restrict__ seqs,
                                                                  const int64_t *__restrict__ off, int max_ltr, int32_t *__restrict__ out) {
    __shared__ long long s_bnd_a[LS_WAVES][2 * LS_BAND];
    __shared__ uint32_t s_bnd_b[LS_WAVES][2 * LS_BAND];
    const int lane = lane_id(), w = wave_id();
    for (int64_t t = (int64_t)blockIdx.x * LS_WAVES + w; t < n_tasks; t += (int64_t)gridDim.x * LS_WAVES) {
        const LsTask T = tasks[t];
        const uint8_t *s = seqs + off[T.seq];
        const int64_t len = off[T.seq + 1] - off[T.seq];
        const int64_t dc = ((int64_t)T.d_lo + T.d_hi) >> 1;
        int pl = 0, pr = 0, n_align = 0, found = 0;
        int64_t ls = 0, le = 0, rs = 0, re = 0;
        LsBest h = {0, 0, 0};
        for (;;) {
            const LsWin W = ls_window(len, T.i_lo, T.i_hi, dc, pl, pr, max_ltr);
            const int m = (int)(W.qe - W.qb), n = (int)(W.se - W.sb);
            n_align++;
            found = 0;
            if (m < 1 || n < 1 || m >= HITE_PAIRHSP_MAX_LEN || n >= HITE_PAIRHSP_MAX_LEN) break;      // (m, n >= 1 by construction, < 32 768 by the limits)
            h = ls_align(s + W.qb, m, s + W.sb, W.dlo, W.dlo + LS_BAND - 1, 1, m, 1, n, s_bnd_a[w], s_bnd_b[w]);
            if ((int)(h.a >> 40) < HITE_PAIRHSP_MIN_SCORE) break;
            found = 1;
            ls = W.qb + (int64_t)(h.b >> 16) - 1; le = W.qb + (int64_t)(h.e >> 16);
            rs = W.sb + (int64_t)(h.b & 0xFFFFu) - 1; re = W.sb + (int64_t)(h.e & 0xFFFFu);
            const int step = ls_pad_steps(W, len, ls, le, pl, pr);
            if (step == 0 || n_align > HITE_LTRSCAN_MAX_REDO) break;
            pl += step & 1;
            pr += step >> 1;
        }
        if (lane == 0) {
            int32_t *o = out + t * LS_OUT_WORDS;
            o[0] = T.seq; o[1] = found; o[2] = (int32_t)ls; o[3] = (int32_t)le; o[4] = (int32_t)rs; o[5] = (int32_t)re;
            o[6] = (int32_t)(h.a >> 40); o[7] = (int32_t)((h.a >> 20) & 0xFFFFF); o[8] = (int32_t)(h.a & 0xFFFFF); o[9] = n_align;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
#define LS_ALLOC(ptr, bytes) HITE_CHECK(ctx, B.alloc(ptr, (size_t)(bytes)))
static inline unsigned ls_grid(int64_t n) { return (unsigned)((n + 255) / 256); }
struct LsRec { int32_t f[8]; };

// one batch: the sequences first .. last - 1 of the call, nb > 0 bytes in all; appends the unfiltered records, adds to st[0 .. 6]
static int ls_batch(hite_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t first, int64_t last, int32_t max_len, int32_t min_ltr,
                    int32_t max_ltr, std::vector<LsRec> &found, int64_t *st) {
    const int64_t nb = seq_off[last] - seq_off[first];
    const int n_seq = (int)(last - first);
    hipStream_t stream = nullptr;
    DevPool B;
    std::vector<int64_t> rel((size_t)n_seq + 1);
    for (int q = 0; q <= n_seq; q++) rel[(size_t)q] = seq_off[first + q] - seq_off[first];
    uint8_t *d_seq; int64_t *d_off; unsigned long long *d_keys, *d_cnt; unsigned *d_vals, *d_hgp, *d_hd;
    LS_ALLOC(d_seq, nb + 16);
    LS_ALLOC(d_off, (n_seq + 1) * 8);
    LS_ALLOC(d_keys, (nb + 1) * 8);
    LS_ALLOC(d_vals, (nb + 1) * 4);
    LS_ALLOC(d_hgp, nb * 4);
    LS_ALLOC(d_hd, nb * 4);
    LS_ALLOC(d_cnt, LS_C_N * 8);
    HITE_CHECK(ctx, hipMemcpyAsync(d_seq, seqs + seq_off[first], (size_t)nb, hipMemcpyHostToDevice, stream));
    HITE_CHECK(ctx, hipMemcpyAsync(d_off, rel.data(), (size_t)(n_seq + 1) * 8, hipMemcpyHostToDevice, stream));
    HITE_CHECK(ctx, hipMemsetAsync(d_cnt, 0, LS_C_N * 8, stream));
    struct SortGuard { Sorter S; bool on = false; ~SortGuard() { if (on) sorter_free(S); } } G;
    G.on = true;
    int rc = sorter_init(G.S, ctx, stream, nb);
    if (rc) return rc;

    int tk = hite_prof_begin(ctx, "ltrscan_words", stream);
    hipLaunchKernelGGL(ls_word_kernel, dim3(ls_grid(nb)), dim3(256), 0, stream, d_seq, d_off, n_seq, nb, d_keys, d_vals, d_cnt);
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipGetLastError());
    tk = hite_prof_begin(ctx, "ltrscan_word_sort", stream);
    rc = sorter_sort_bits(G.S, d_keys, d_vals, nb, 0, LS_WORD_BITS);
    hite_prof_end(ctx, tk, stream);
    if (rc) return rc;
    const int64_t dmin = min_ltr, dmax = (int64_t)max_len - min_ltr;
    tk = hite_prof_begin(ctx, "ltrscan_links", stream);
    hipLaunchKernelGGL(ls_link_kernel, dim3(ls_grid(nb)), dim3(256), 0, stream, d_keys, d_vals, nb, d_off, n_seq, dmin, dmax, d_hgp, d_hd, d_cnt);
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipGetLastError());
    unsigned long long h_cnt[LS_C_N];
    HITE_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
    HITE_CHECK(ctx, hipStreamSynchronize(stream));
    const int64_t nh = (int64_t)h_cnt[LS_C_HITS];
    st[0] += (int64_t)h_cnt[LS_C_WORDS];
    st[1] += nh;
    if (nh < HITE_LTRSCAN_MIN_HITS) return HITE_OK;

    // the runs of both lattices; the word keys and positions are done with: the hit keys take their place
    const int64_t task_cap = nh / 2 + 2;      // a run that counts holds >= 4 hits, on each of two lattices
    int32_t *d_flags; int64_t *d_excl, *d_bs; unsigned *d_start; int *d_dlo, *d_dhi; LsTask *d_tasks;
    LS_ALLOC(d_flags, nh * 4);
    LS_ALLOC(d_excl, (nh + 1) * 8);
    LS_ALLOC(d_bs, scan_tmp_elems(nh) * 8);
    LS_ALLOC(d_start, (nh + 2) * 4);
    LS_ALLOC(d_dlo, nh * 4);
    LS_ALLOC(d_dhi, nh * 4);
    LS_ALLOC(d_tasks, task_cap * sizeof(LsTask));
    const int pos_bits = ls_bits((unsigned long long)(nb - 1));
    const int bin_bits = ls_bits((unsigned long long)((std::max<int64_t>(dmax, 0) + HITE_LTRSCAN_LATTICE) >> HITE_LTRSCAN_BIN_SHIFT));
    tk = hite_prof_begin(ctx, "ltrscan_runs", stream);
    for (int lam = 0; lam <= HITE_LTRSCAN_LATTICE; lam += HITE_LTRSCAN_LATTICE) {
        hipLaunchKernelGGL(ls_hit_key_kernel, dim3(ls_grid(nh)), dim3(256), 0, stream, d_hgp, d_hd, nh, lam, pos_bits, d_keys, d_vals);
        HITE_CHECK(ctx, hipGetLastError());
        if ((rc = sorter_sort_bits(G.S, d_keys, d_vals, nh, 0, pos_bits + bin_bits))) return rc;
        hipLaunchKernelGGL(ls_head_kernel, dim3(ls_grid(nh)), dim3(256), 0, stream, d_keys, nh, pos_bits, d_off, n_seq, d_flags);
        HITE_CHECK(ctx, hipGetLastError());
        if ((rc = scan_excl_buf<int32_t>(ctx, d_bs, d_flags, nh, d_excl, stream))) return rc;
        int64_t n_runs = 0;
        HITE_CHECK(ctx, hipMemcpyAsync(&n_runs, d_excl + nh, 8, hipMemcpyDeviceToHost, stream));
        HITE_CHECK(ctx, hipStreamSynchronize(stream));
        if (n_runs < 1 || n_runs > nh) { snprintf(ctx->err, sizeof(ctx->err), "hite_ltr_scan: %lld runs of %lld hits", (long long)n_runs, (long long)nh); return HITE_EHIP; }
        HITE_CHECK(ctx, hipMemsetAsync(d_dlo, 0x7f, (size_t)n_runs * 4, stream));
        HITE_CHECK(ctx, hipMemsetAsync(d_dhi, 0, (size_t)n_runs * 4, stream));
        hipLaunchKernelGGL(ls_run_fill_kernel, dim3(ls_grid(nh)), dim3(256), 0, stream, d_vals, d_flags, d_excl, nh, n_runs, d_start, d_dlo, d_dhi);
        hipLaunchKernelGGL(ls_run_emit_kernel, dim3(ls_grid(n_runs)), dim3(256), 0, stream, d_keys, pos_bits, d_start, d_dlo, d_dhi, n_runs, d_off,
                           n_seq, (int)max_ltr, d_tasks, task_cap, d_cnt);
        HITE_CHECK(ctx, hipGetLastError());
    }
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
    HITE_CHECK(ctx, hipStreamSynchronize(stream));
    st[2] += (int64_t)h_cnt[LS_C_RUNS];
    st[3] += (int64_t)h_cnt[LS_C_SPAN];
    const int64_t n_tasks = (int64_t)h_cnt[LS_C_TASKS];
    if (n_tasks > task_cap) { snprintf(ctx->err, sizeof(ctx->err), "hite_ltr_scan: %lld runs beyond the room for %lld", (long long)n_tasks, (long long)task_cap); return HITE_EHIP; }
    if (n_tasks == 0) return HITE_OK;

    int32_t *d_out;
    LS_ALLOC(d_out, n_tasks * LS_OUT_WORDS * 4);
    const unsigned blocks = (unsigned)std::min<int64_t>((n_tasks + LS_WAVES - 1) / LS_WAVES, LS_MAX_BLOCKS);
    tk = hite_prof_begin(ctx, "ltrscan_extend", stream);
    hipLaunchKernelGGL(ls_extend_kernel, dim3(blocks), dim3(LS_WAVES * 64), 0, stream, d_tasks, n_tasks, d_seq, d_off, (int)max_ltr, d_out);
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipGetLastError());
    std::vector<int32_t> h_out((size_t)n_tasks * LS_OUT_WORDS);
    HITE_CHECK(ctx, hipMemcpyAsync(h_out.data(), d_out, h_out.size() * 4, hipMemcpyDeviceToHost, stream));
    HITE_CHECK(ctx, hipStreamSynchronize(stream));
    for (int64_t t = 0; t < n_tasks; t++) {
        const int32_t *o = h_out.data() + t * LS_OUT_WORDS;
        st[4] += o[9];
        st[5] += o[9] - 1;
        if (!o[1]) { st[6]++; continue; }
        LsRec r;
        r.f[0] = (int32_t)(first + o[0]);
        memcpy(r.f + 1, o + 2, 7 * sizeof(int32_t));
        found.push_back(r);
    }
    return HITE_OK;
}

extern "C" int hite_ltr_scan(hite_ctx *ctx, int64_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t min_len, int32_t max_len,
                             int32_t min_ltr, int32_t max_ltr, int32_t identity, int64_t cap, int32_t *recs, int64_t *n_out, int64_t *stats) {
    if (!ctx || !n_out || n < 0 || n >= ((int64_t)1 << 31) || cap < 0 || (cap > 0 && !recs) || (n > 0 && !seq_off)) return HITE_EINVAL;
    if (min_ltr < 1 || min_ltr > max_ltr || max_ltr > HITE_LTRSCAN_MAX_LTR || min_len > max_len || identity < 1 || identity > 100) return HITE_EINVAL;
    *n_out = 0;
    int64_t st[HITE_LTRSCAN_STATS] = {0};
    if (stats) memset(stats, 0, sizeof(st));
    if (n > 0) {
        if (!csr_sorted(seq_off, n)) return HITE_EINVAL;
        for (int64_t q = 0; q < n; q++) if (seq_off[q + 1] - seq_off[q] >= ((int64_t)1 << 31)) return HITE_EINVAL;
        if (seq_off[n] > seq_off[0] && !seqs) return HITE_EINVAL;
    }
    const int64_t batch_bytes = ctx->ltrscan_batch_bytes > 0 ? ctx->ltrscan_batch_bytes : LS_BATCH_BYTES;
    try {
        std::vector<LsRec> found;
        if (n > 0 && seq_off[n] - seq_off[0] >= HITE_LTRSCAN_WORD) {
            HITE_CHECK(ctx, hipSetDevice(ctx->device));
            // whole sequences, as many as stay within the bound; a longer one goes alone
            for (int64_t first = 0; first < n;) {
                int64_t last = first + 1;
                while (last < n && seq_off[last + 1] - seq_off[first] <= batch_bytes) last++;
                if (seq_off[last] - seq_off[first] >= HITE_LTRSCAN_WORD) {
                    const int rc = ls_batch(ctx, seqs, seq_off, first, last, max_len, min_ltr, max_ltr, found, st);
                    if (rc) return rc;
                }
                first = last;
            }
            hite_prof_resolve(ctx);
        }
        // steps 5 and 6
        std::vector<LsRec> kept;
        for (const LsRec &r : found) {
            const int why = ls_filter(r.f, min_len, max_len, min_ltr, max_ltr, identity);
            if (why) st[6 + why]++;
            else kept.push_back(r);
        }
        std::sort(kept.begin(), kept.end(), [](const LsRec &x, const LsRec &y) { return ls_rec_less(x.f, y.f); });
        int64_t total = 0;
        for (size_t k = 0; k < kept.size(); k++) {
            if (k > 0 && ls_rec_same_place(kept[k].f, kept[k - 1].f)) continue;
            if (total < cap) memcpy(recs + 8 * total, kept[k].f, sizeof(kept[k].f));
            total++;
        }
        st[11] = total;
        *n_out = total;
        if (stats) memcpy(stats, st, sizeof(st));
        return total > cap ? HITE_ECAP : HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

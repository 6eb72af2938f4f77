// hite_hsp.h -- the banded local aligner of hite_pair_hsps, step 4 (include/hite_gpu.h, "local alignments of pairs of intervals"), once:
// the cell value and its recurrence, the strip routine a wavefront runs it with, and the word key and word kernel of the stages that
// seed it from 13-base words.  Its users are hite_pairhsp.hip (a band per voted window), hite_ltrscan.hip and hite_annotate.hip (a
// band per run of hits, with a redo loop of growing pads around it).
//
// hsp_align: the lanes are 64 columns of a strip, lane l on row first + d - 1 - l at step d, so that the cell above is the lane's own
// last value, the cell to the left the last value of lane l - 1 and the diagonal cell what lane l - 1 handed over one step earlier
// (data-parallel moves, no LDS).  Only the rows where the band meets the strip are visited (at most 255).  The last column of a strip
// stays in LDS, indexed by its diagonal (HSP_BAND values, two buffers in turn), and is what lane 0 of the next strip reads.
//
// The blocks between `// >>> name` and `// <<< name` are also compiled for the host (tests/hsp_host.py).
#pragma once
#include "hite_common.h"

// >>> hsp_cell
// A cell value (score, matches, columns, q_start, s_start) is TWO words.  a = score * 2^40 + matches * 2^20 + columns, signed: matches
// <= 32 768 and columns <= 65 536 are never negative and stay below 2^20, so the integer order of a is the lexicographic order of the
// first three fields, a step is one addition and "score <= 0" is a < 2^40.  b = q_start * 2^16 + s_start (both <= 32 768): on equal a
// the smaller b wins.  The empty value is (0, 0).
#define HSP_BAND 192                               // diagonals of a band: every user's BAND_BELOW + BAND_ABOVE
#define HSP_SCORE_ONE ((int64_t)1 << 40)
#define HSP_STEP_MATCH (HITE_PAIRHSP_MATCH * HSP_SCORE_ONE + ((int64_t)1 << 20) + 1)
#define HSP_STEP_MISMATCH (HITE_PAIRHSP_MISMATCH * HSP_SCORE_ONE + 1)
#define HSP_STEP_GAP (HITE_PAIRHSP_GAP * HSP_SCORE_ONE + 1)
struct HspVal { int64_t a; uint32_t b; };
// a byte (either case) as a base code A 0 / C 1 / G 2 / T 3 / anything else 4
__device__ __forceinline__ int hsp_code(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}
__device__ __forceinline__ bool hsp_better(int64_t a1, uint32_t b1, int64_t a2, uint32_t b2) { return a1 > a2 || (a1 == a2 && b1 < b2); }
// V(i, j) from diag = V(i-1, j-1), up = V(i-1, j), left = V(i, j-1); a path that leaves the empty value starts at (i, j) (only a
// match can: every other step from the empty value has a score <= 0)
__device__ __forceinline__ HspVal hsp_cell(HspVal diag, HspVal up, HspVal left, int ca, int cb, int i, int j) {
    HspVal v;
    v.a = diag.a + ((ca == cb && ca < 4) ? HSP_STEP_MATCH : HSP_STEP_MISMATCH);
    v.b = diag.a == 0 ? ((uint32_t)i << 16 | (uint32_t)j) : diag.b;
    const int64_t ua = up.a + HSP_STEP_GAP, la = left.a + HSP_STEP_GAP;
    if (hsp_better(ua, up.b, v.a, v.b)) { v.a = ua; v.b = up.b; }
    if (hsp_better(la, left.b, v.a, v.b)) { v.a = la; v.b = left.b; }
    if (v.a < HSP_SCORE_ONE) { v.a = 0; v.b = 0; }
    return v;
}
// the best cell so far: its value and e = i * 2^16 + j; a later cell takes its place when its value is better, or equal at a smaller e
struct HspBest { int64_t a; uint32_t b, e; };
__device__ __forceinline__ bool hsp_best_better(int64_t a, uint32_t b, uint32_t e, const HspBest &o) {
    return a > o.a || (a == o.a && (b < o.b || (b == o.b && e < o.e)));
}
// the fields of a best cell (a, b, e): the path runs from (q_start, s_start) to (q_end, s_end), 1-based and inclusive.  Macros and not
// functions: a call stays opaque to the passes that run before the inliner, and ph_pair_kernel then comes out in other registers.
#define hsp_score(a) ((int)((a) >> 40))
#define hsp_matches(a) ((int)(((a) >> 20) & 0xFFFFF))
#define hsp_columns(a) ((int)((a) & 0xFFFFF))
#define hsp_q_start(b) ((int)((b) >> 16))
#define hsp_s_start(b) ((int)((b) & 0xFFFFu))
#define hsp_q_end(e) ((int)((e) >> 16))
#define hsp_s_end(e) ((int)((e) & 0xFFFFu))
// <<< hsp_cell

// >>> hsp_key
// the word of WORD base codes (the first one in the highest bits), or the "no word" value 1 << 2 * WORD when one of them is not in ACGT
template <int WORD>
__host__ __device__ __forceinline__ unsigned long long hsp_word_key(const int *codes) {
    unsigned long long w = 0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < WORD; k++) { ok = ok && codes[k] < 4; w = w * 4 + (unsigned long long)(codes[k] & 3); }
    return ok ? w : ((unsigned long long)1 << 2 * WORD);
}
// bits that hold every value 0 .. v
__host__ __device__ __forceinline__ int hsp_bits(unsigned long long v) { int b = 1; while (b < 64 && (v >> b) != 0) b++; return b; }
// <<< hsp_key

// lane l takes the value of lane l - 1 (wave_shr1), lane 0 gets 0 and the caller puts its own value there
__device__ __forceinline__ HspVal hsp_up1(HspVal v) {
    HspVal r;
    const uint32_t lo = (uint32_t)wave_shr1((int)(uint32_t)v.a), hi = (uint32_t)wave_shr1((int)(uint32_t)((uint64_t)v.a >> 32));
    r.a = (int64_t)((uint64_t)hi << 32 | lo);
    r.b = (uint32_t)wave_shr1((int)v.b);
    return r;
}

__device__ __forceinline__ HspBest hsp_wave_best(HspBest v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        HspBest y;
        y.a = __shfl_xor((long long)v.a, d, 64);
        y.b = __shfl_xor(v.b, d, 64);
        y.e = __shfl_xor(v.e, d, 64);
        if (hsp_best_better(y.a, y.b, y.e, v)) v = y;
    }
    return v;
}

// The best cell of rows r0 .. r1 and columns c0 .. c1 (1-based, inside [1, m] x [1, n]) within the band dlo <= j - i <= dhi
// (dhi - dlo < HSP_BAND), by one wavefront; q / s: the bytes of the two intervals; bnd_a / bnd_b: 2 x HSP_BAND words of the wavefront.
// All lanes return the same value; a == 0: no cell has a positive score.
__device__ __forceinline__ HspBest hsp_align(const uint8_t *q, int m, const uint8_t *s, int dlo, int dhi, int r0, int r1, int c0, int c1,
                                             long long *bnd_a, uint32_t *bnd_b) {
    const int lane = lane_id();
    HspBest best = {0, 0, 0};
    const int cs = max(c0, r0 + dlo), ce = min(c1, r1 + dhi);      // the columns the band reaches inside the rectangle
    int buf = 0;
    for (int js = cs; js <= ce; js += 64, buf ^= 1) {
        const int nl = min(64, ce - js + 1);
        const bool more = js + 64 <= ce;
        const int first = max(r0, js - dhi), last = min(r1, js + nl - 1 - dlo);      // the rows where the band meets the strip
        const int ib = first - 1, j = js + lane;
        const int cb = lane < nl ? hsp_code(s[j - 1]) : 4;
        const long long *rd_a = bnd_a + (buf ^ 1) * HSP_BAND;
        const uint32_t *rd_b = bnd_b + (buf ^ 1) * HSP_BAND;
        long long *wr_a = bnd_a + buf * HSP_BAND;
        uint32_t *wr_b = bnd_b + buf * HSP_BAND;
        // V(row, js - 1): the last column of the strip before, the empty value outside the band or the rectangle
        auto edge = [&](int row) {
            HspVal v = {0, 0};
            const int dd = js - 1 - row;
            if (js > cs && row >= r0 && row <= r1 && dd >= dlo && dd <= dhi) { v.a = (int64_t)rd_a[dhi - dd]; v.b = rd_b[dhi - dd]; }
            return v;
        };
        HspVal cur = {0, 0}, diag = {0, 0};
        if (lane == 0) diag = edge(ib);
        HspVal ahead = edge(ib + 1);     // lane 0's left neighbour of the next step
        int ca = 4, a64 = 4;             // the lane's base of Q; Q[ib + 64 k + lane] of the current 64 rows
        const int steps = last - ib + nl - 1;
        for (int d = 1; d <= steps; d++) {
            const int i = ib + d - lane;
            if (((d - 1) & 63) == 0) {
                const int r = ib + d + lane;
                a64 = r <= m ? hsp_code(q[r - 1]) : 4;      // r >= 1: first >= r0 >= 1, so ib >= 0, and d >= 1
            }
            const int a_new = __builtin_amdgcn_readlane(a64, (d - 1) & 63);      // the code of row ib + d
            ca = wave_shr1(ca);
            HspVal left = hsp_up1(cur);
            if (lane == 0) { ca = a_new; left = ahead; }
            ahead = edge(ib + d + 1);
            const bool on = lane < nl && i >= r0 && i <= r1 && j - i >= dlo && j - i <= dhi;
            HspVal v = hsp_cell(diag, cur, left, ca, cb, i, j);
            diag = left;
            if (!on) { v.a = 0; v.b = 0; }
            cur = v;
            if (on) {
                const uint32_t e = (uint32_t)i << 16 | (uint32_t)j;
                if (v.a > 0 && hsp_best_better(v.a, v.b, e, best)) { best.a = v.a; best.b = v.b; best.e = e; }
                if (more && lane == 63) { wr_a[dhi - (j - i)] = (long long)v.a; wr_b[dhi - (j - i)] = v.b; }
            }
        }
        __threadfence_block();          // lane 0 of the next strip reads what lane 63 wrote
    }
    return hsp_wave_best(best);
}

// one thread per byte of a batch of nb bytes (off: the n sequences' offsets in it, off[0] = 0): the word that begins there, or the
// "no word" value where the sequence ends sooner, as keys[p] beside vals[p] = p; *counter gains the number of words
template <int WORD>
static __global__ void __launch_bounds__(256) hsp_word_kernel(const uint8_t *__restrict__ seqs, const int64_t *__restrict__ off, int n, int64_t nb,
                                                              unsigned long long *__restrict__ keys, unsigned *__restrict__ vals,
                                                              unsigned long long *__restrict__ counter) {
    const unsigned long long no_word = (unsigned long long)1 << 2 * WORD;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long key = no_word;
    if (p < nb) {
        const int q = last_le(off, n, p);
        if (p + WORD <= off[q + 1]) {
            int codes[WORD];
#pragma unroll
            for (int k = 0; k < WORD; k++) codes[k] = hsp_code(seqs[p + k]);
            key = hsp_word_key<WORD>(codes);
        }
        keys[p] = key;
        vals[p] = (unsigned)p;
    }
    (void)wave_take_flag(key != no_word, counter);
}

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
//   4. extension: ONE WAVEFRONT PER RUN through hsp_align (hite_hsp.h: the cell and the strip routine of hite_pair_hsps, which the
//      word key and the word kernel of step 1 come from as well); the redo loop of the pads runs inside the wavefront.
// The filters, the order and the duplicates (steps 5 and 6) are host code.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include "hite_hsp.h"
#include "hite_sort.h"
#include <algorithm>
#include <new>
#include <vector>

#define LS_WAVES 4
static_assert(HITE_LTRSCAN_BAND_BELOW + HITE_LTRSCAN_BAND_ABOVE == HSP_BAND, "the band of a run is the band of hsp_align");
#define LS_BATCH_BYTES ((int64_t)64 << 20)       // sequence bytes per batch ($HITE_LTRSCAN_BATCH_BYTES overrides)
#define LS_NO_WORD ((unsigned long long)1 << 2 * HITE_LTRSCAN_WORD)      // what hsp_word_key gives a position without a word
#define LS_WORD_BITS 27
#define LS_OUT_WORDS 10                           // per run: seq, found, ls, le, rs, re, score, matches, columns, alignments
#define LS_MAX_BLOCKS 2048
#ifndef __host__
#define __host__
#endif

// >>> ltrscan_key
// a hit on lattice lam (0 or HITE_LTRSCAN_LATTICE) as one key: its bin above the pos_bits bits of its position in the batch
__host__ __device__ __forceinline__ unsigned long long ls_hit_key(uint32_t gp, uint32_t d, int lam, int pos_bits) {
    return (((unsigned long long)d + (unsigned long long)lam) >> HITE_LTRSCAN_BIN_SHIFT) << pos_bits | (unsigned long long)gp;
}
__host__ __device__ __forceinline__ int64_t ls_key_pos(unsigned long long key, int pos_bits) { return (int64_t)(key & (((unsigned long long)1 << pos_bits) - 1)); }
__host__ __device__ __forceinline__ int64_t ls_key_bin(unsigned long long key, int pos_bits) { return (int64_t)(key >> pos_bits); }
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
            const int64_t end = off[last_le(off, n_seq, i) + 1];
            for (int t = 1; t <= HITE_LTRSCAN_MAX_OCC; t++) {
                if (e + t >= nb || keys[e + t] != w) break;
                const int64_t j = vals[e + t];
                if (j >= end) break;
                d = j - i;
                if (d >= dmin) { hit = d <= dmax; break; }
            }
        }
    }
    const unsigned long long at = wave_take_flag(hit, &counters[LS_C_HITS]);
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
               off[last_le(off, n_seq, gp)] > gpp;
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
            const int q = last_le(off, n_seq, g_lo);
            T.seq = q; T.i_lo = (int32_t)(g_lo - off[q]); T.i_hi = (int32_t)(g_hi - off[q]); T.d_lo = d_lo[r]; T.d_hi = d_hi[r];
        }
    }
    (void)wave_take_flag(counted, &counters[LS_C_RUNS]);
    (void)wave_take_flag(wide, &counters[LS_C_SPAN]);
    const bool go = counted && !wide;
    const unsigned long long at = wave_take_flag(go, &counters[LS_C_TASKS]);
    if (go && (int64_t)at < task_cap) tasks[at] = T;
}

// wavefront per run: step 4 of the header with its redo loop
__global__ __launch_bounds__(LS_WAVES * 64) void ls_extend_kernel(const LsTask *__restrict__ tasks, int64_t n_tasks, const uint8_t *__restrict__ seqs,
                                                                  const int64_t *__restrict__ off, int max_ltr, int32_t *__restrict__ out) {
    __shared__ long long s_bnd_a[LS_WAVES][2 * HSP_BAND];
    __shared__ uint32_t s_bnd_b[LS_WAVES][2 * HSP_BAND];
    const int lane = lane_id(), w = wave_id();
    for (int64_t t = (int64_t)blockIdx.x * LS_WAVES + w; t < n_tasks; t += (int64_t)gridDim.x * LS_WAVES) {
        const LsTask T = tasks[t];
        const uint8_t *s = seqs + off[T.seq];
        const int64_t len = off[T.seq + 1] - off[T.seq];
        const int64_t dc = ((int64_t)T.d_lo + T.d_hi) >> 1;
        int pl = 0, pr = 0, n_align = 0, found = 0;
        int64_t ls = 0, le = 0, rs = 0, re = 0;
        HspBest h = {0, 0, 0};
        for (;;) {
            const LsWin W = ls_window(len, T.i_lo, T.i_hi, dc, pl, pr, max_ltr);
            const int m = (int)(W.qe - W.qb), n = (int)(W.se - W.sb);
            n_align++;
            found = 0;
            if (m < 1 || n < 1 || m >= HITE_PAIRHSP_MAX_LEN || n >= HITE_PAIRHSP_MAX_LEN) break;      // (m, n >= 1 by construction, < 32 768 by the limits)
            h = hsp_align(s + W.qb, m, s + W.sb, W.dlo, W.dlo + HSP_BAND - 1, 1, m, 1, n, s_bnd_a[w], s_bnd_b[w]);
            if (hsp_score(h.a) < HITE_PAIRHSP_MIN_SCORE) break;
            found = 1;
            ls = W.qb + hsp_q_start(h.b) - 1; le = W.qb + hsp_q_end(h.e);
            rs = W.sb + hsp_s_start(h.b) - 1; re = W.sb + hsp_s_end(h.e);
            const int step = ls_pad_steps(W, len, ls, le, pl, pr);
            if (step == 0 || n_align > HITE_LTRSCAN_MAX_REDO) break;
            pl += step & 1;
            pr += step >> 1;
        }
        if (lane == 0) {
            int32_t *o = out + t * LS_OUT_WORDS;
            o[0] = T.seq; o[1] = found; o[2] = (int32_t)ls; o[3] = (int32_t)le; o[4] = (int32_t)rs; o[5] = (int32_t)re;
            o[6] = hsp_score(h.a); o[7] = hsp_matches(h.a); o[8] = hsp_columns(h.a); o[9] = n_align;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
#define LS_ALLOC(ptr, bytes) HITE_CHECK(ctx, B.alloc(ptr, (size_t)(bytes)))
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
    hipLaunchKernelGGL(hsp_word_kernel<HITE_LTRSCAN_WORD>, dim3(grid256(nb)), dim3(256), 0, stream, d_seq, d_off, n_seq, nb, d_keys, d_vals,
                       d_cnt + LS_C_WORDS);
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipGetLastError());
    tk = hite_prof_begin(ctx, "ltrscan_word_sort", stream);
    rc = sorter_sort_bits(G.S, d_keys, d_vals, nb, 0, LS_WORD_BITS);
    hite_prof_end(ctx, tk, stream);
    if (rc) return rc;
    const int64_t dmin = min_ltr, dmax = (int64_t)max_len - min_ltr;
    tk = hite_prof_begin(ctx, "ltrscan_links", stream);
    hipLaunchKernelGGL(ls_link_kernel, dim3(grid256(nb)), dim3(256), 0, stream, d_keys, d_vals, nb, d_off, n_seq, dmin, dmax, d_hgp, d_hd, d_cnt);
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
    const int pos_bits = hsp_bits((unsigned long long)(nb - 1));
    const int bin_bits = hsp_bits((unsigned long long)((std::max<int64_t>(dmax, 0) + HITE_LTRSCAN_LATTICE) >> HITE_LTRSCAN_BIN_SHIFT));
    tk = hite_prof_begin(ctx, "ltrscan_runs", stream);
    for (int lam = 0; lam <= HITE_LTRSCAN_LATTICE; lam += HITE_LTRSCAN_LATTICE) {
        hipLaunchKernelGGL(ls_hit_key_kernel, dim3(grid256(nh)), dim3(256), 0, stream, d_hgp, d_hd, nh, lam, pos_bits, d_keys, d_vals);
        HITE_CHECK(ctx, hipGetLastError());
        if ((rc = sorter_sort_bits(G.S, d_keys, d_vals, nh, 0, pos_bits + bin_bits))) return rc;
        hipLaunchKernelGGL(ls_head_kernel, dim3(grid256(nh)), dim3(256), 0, stream, d_keys, nh, pos_bits, d_off, n_seq, d_flags);
        HITE_CHECK(ctx, hipGetLastError());
        if ((rc = scan_excl_buf<int32_t>(ctx, d_bs, d_flags, nh, d_excl, stream))) return rc;
        int64_t n_runs = 0;
        HITE_CHECK(ctx, hipMemcpyAsync(&n_runs, d_excl + nh, 8, hipMemcpyDeviceToHost, stream));
        HITE_CHECK(ctx, hipStreamSynchronize(stream));
        if (n_runs < 1 || n_runs > nh) { snprintf(ctx->err, sizeof(ctx->err), "hite_ltr_scan: %lld runs of %lld hits", (long long)n_runs, (long long)nh); return HITE_EHIP; }
        HITE_CHECK(ctx, hipMemsetAsync(d_dlo, 0x7f, (size_t)n_runs * 4, stream));
        HITE_CHECK(ctx, hipMemsetAsync(d_dhi, 0, (size_t)n_runs * 4, stream));
        hipLaunchKernelGGL(ls_run_fill_kernel, dim3(grid256(nh)), dim3(256), 0, stream, d_vals, d_flags, d_excl, nh, n_runs, d_start, d_dlo, d_dhi);
        hipLaunchKernelGGL(ls_run_emit_kernel, dim3(grid256(n_runs)), dim3(256), 0, stream, d_keys, pos_bits, d_start, d_dlo, d_dhi, n_runs, d_off,
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

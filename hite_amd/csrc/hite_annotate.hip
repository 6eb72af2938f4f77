// hite_annotate.hip -- the genome annotation: TE library + genome in, annotation records out, where HiTE ends with a RepeatMasker run
// (module/annotate_genome.py:17, module/pan_annotate_genome.py:27).  Not RepeatMasker and not pinned to it (no machine of the project
// has it): parity is the written definition in include/hite_gpu.h ("genome annotation"), its CPU twin tests/annotate_twin.py +
// tests/annotate_twin.c, HIP == twin record for record and counter for counter.  It is the pattern of hite_ltrscan.hip turned from
// genome x genome to library x genome, on both strands --
//   1. table: the texts (every entry and its reverse complement, built on the host) go up once per call; one thread per text
//      position forms the 26-bit word (bit 26: no word there); the positions are sorted on those 27 bits with the stable sort of
//      hite_sort.h.  The sorted words are the table: it stays on the device for all batches;
//   2. hits, per batch of pieces: one thread per base of the batch looks its word up by binary search (the table fits L2), counts
//      the entries of the word (more than HITE_ANNOT_MAX_OCC: silenced) and the hits of a wavefront are compacted with one atomic per
//      wavefront.  A hit is one 64-bit value (t, q, position in the batch).  The room is a guess; when the count says it was too
//      small the pass is run again with the room known;
//   3. runs, once per lattice: the hits are sorted on (t, bin, position) packed into one 64-bit key; the thread of a hit that begins
//      a chain (another t, bin or piece, or more than HITE_ANNOT_GAP after the hit before) walks the chain, closes it where the span
//      limit says so and emits every run as a task with one atomic per run;
//   4. extension: ONE WAVEFRONT PER RUN through hsp_align (hite_hsp.h: the cell and the strip routine of hite_pair_hsps, which the
//      word key and the word kernel of step 1 come from as well), as ls_extend_kernel has it: rows are the text, columns the genome;
//      the redo loop of the pads runs inside the wavefront.
// The resolve and the order (steps 5 and 6) are host code.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include "hite_hsp.h"
#include "hite_sort.h"
#include <algorithm>
#include <new>
#include <vector>

#define AN_WAVES 4
static_assert(HITE_ANNOT_BAND_BELOW + HITE_ANNOT_BAND_ABOVE == HSP_BAND, "the band of a run is the band of hsp_align");
#define AN_BATCH_BYTES ((int64_t)64 << 20)      // bases per batch, the margins included ($HITE_ANNOT_BATCH_BYTES sets a smaller bound)
#define AN_HALO (HITE_ANNOT_PAD_3 + HITE_ANNOT_BAND_ABOVE + HITE_ANNOT_WORD)      // bases beside a piece that a window can reach
#define AN_NO_WORD ((unsigned long long)1 << 2 * HITE_ANNOT_WORD)      // what hsp_word_key gives a position without a word
#define AN_WORD_BITS 27
#define AN_OUT_WORDS 12                          // per run: found, seq, gs, ge, t, qs, qe, score, matches, columns, alignments, fault
#define AN_MAX_BLOCKS 2048
#ifndef __host__
#define __host__
#endif

// >>> annotate_key
// the reverse complement's byte for a byte of the entry: anything outside ACGT (either case) becomes N
__host__ __device__ __forceinline__ uint8_t an_comp(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 'T';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        case 'T': case 't': return 'A';
        default: return 'N';
    }
}
// a hit as one value: t above q above the position gp in the batch
#define AN_Q_BITS 15                             // q < HITE_ANNOT_MAX_LIB_LEN <= 2^15
#define AN_POS_BITS 26                           // a position in a batch of <= 64 MiB
__host__ __device__ __forceinline__ unsigned long long an_hit_pack(uint32_t t, uint32_t q, uint32_t gp) {
    return ((unsigned long long)t << AN_Q_BITS | q) << AN_POS_BITS | gp;
}
__host__ __device__ __forceinline__ uint32_t an_hit_t(unsigned long long h) { return (uint32_t)(h >> (AN_Q_BITS + AN_POS_BITS)); }
__host__ __device__ __forceinline__ uint32_t an_hit_q(unsigned long long h) { return (uint32_t)(h >> AN_POS_BITS) & ((1u << AN_Q_BITS) - 1); }
__host__ __device__ __forceinline__ uint32_t an_hit_gp(unsigned long long h) { return (uint32_t)h & ((1u << AN_POS_BITS) - 1); }
// the diagonal of a hit as the sort carries it: g_rel - q + HITE_ANNOT_MAX_LIB_LEN >= 0, g_rel counted from the piece's first base
__host__ __device__ __forceinline__ uint32_t an_diag(int64_t g_rel, uint32_t q) { return (uint32_t)(g_rel - (int64_t)q + HITE_ANNOT_MAX_LIB_LEN); }
// a hit on lattice lam (0 or HITE_ANNOT_LATTICE) as one sort key: t, the bin, the position in the batch
__host__ __device__ __forceinline__ unsigned long long an_run_key(uint32_t t, uint32_t diag, uint32_t gp, int lam, int bin_bits, int pos_bits) {
    return ((unsigned long long)t << bin_bits | (unsigned long long)((diag + (uint32_t)lam) >> HITE_ANNOT_BIN_SHIFT)) << pos_bits | gp;
}
__host__ __device__ __forceinline__ int64_t an_key_pos(unsigned long long key, int pos_bits) { return (int64_t)(key & (((unsigned long long)1 << pos_bits) - 1)); }
__host__ __device__ __forceinline__ unsigned long long an_key_group(unsigned long long key, int pos_bits) { return key >> pos_bits; }
// the pad of level k = 0 .. 3
__host__ __device__ __forceinline__ int an_pad(int k) { return k == 0 ? HITE_ANNOT_PAD_0 : k == 1 ? HITE_ANNOT_PAD_1 : k == 2 ? HITE_ANNOT_PAD_2 : HITE_ANNOT_PAD_3; }
// the two windows of a run at the pad levels pl, pr: Q = [qb, qe) of a text of L bases, S = [sb, se) of a sequence of len bases, and
// the lowest diagonal j - i of the band in the 1-based coordinates of the windows (the highest is dlo + 191)
struct AnWin { int64_t qb, qe, sb, se; int dlo; };
__host__ __device__ __forceinline__ AnWin an_window(int64_t L, int64_t len, int64_t g_lo, int64_t g_hi, int64_t dc, int pl, int pr) {
    AnWin w;
    w.qb = g_lo - dc - an_pad(pl); if (w.qb < 0) w.qb = 0;
    w.qe = g_hi - dc + HITE_ANNOT_WORD + an_pad(pr); if (w.qe > L) w.qe = L;
    w.sb = w.qb + dc - HITE_ANNOT_BAND_BELOW; if (w.sb < 0) w.sb = 0;
    w.se = w.qe + dc + HITE_ANNOT_BAND_ABOVE; if (w.se > len) w.se = len;
    w.dlo = (int)(dc - HITE_ANNOT_BAND_BELOW - (w.sb - w.qb));
    return w;
}
// which pads step after an HSP [qs, qe) of the text: bit 0 the left one, bit 1 the right one
__host__ __device__ __forceinline__ int an_pad_steps(const AnWin &w, int64_t L, int64_t qs, int64_t qe, int pl, int pr) {
    int s = 0;
    if (qs - w.qb < HITE_ANNOT_EDGE && w.qb > 0 && pl < 3) s |= 1;
    if (w.qe - qe < HITE_ANNOT_EDGE && w.qe < L && pr < 3) s |= 2;
    return s;
}
// a chain walked hit by hit (step 3): the hit (g, diag) either joins (returns false) or closes the chain and starts the next one
// (returns true: the caller emits *this as it was before the call when n >= HITE_ANNOT_MIN_HITS)
struct AnChain { int64_t g_first, g_last; uint32_t d_lo, d_hi; int64_t n; };
__host__ __device__ __forceinline__ bool an_chain_breaks(const AnChain &c, int64_t g) {
    return g - c.g_last > HITE_ANNOT_GAP || g - c.g_first >= HITE_ANNOT_MAX_SPAN;
}
__host__ __device__ __forceinline__ void an_chain_start(AnChain &c, int64_t g, uint32_t diag) { c.g_first = c.g_last = g; c.d_lo = c.d_hi = diag; c.n = 1; }
__host__ __device__ __forceinline__ void an_chain_add(AnChain &c, int64_t g, uint32_t diag) {
    c.g_last = g; c.n++;
    if (diag < c.d_lo) c.d_lo = diag;
    if (diag > c.d_hi) c.d_hi = diag;
}
// <<< annotate_key

// >>> annotate_resolve
// steps 5 and 6 on records of ten int32 (seq, g_start, g_end, lib, strand, q_start, q_end, score, matches, columns)
struct AnRec { int32_t f[HITE_ANNOT_REC]; };
// the order key: (seq, g_start, g_end, lib, strand, q_start, q_end, -score, -matches, columns)
__host__ __device__ __forceinline__ bool an_rec_less(const int32_t *x, const int32_t *y) {
    for (int k = 0; k < 7; k++) if (x[k] != y[k]) return x[k] < y[k];
    if (x[7] != y[7]) return x[7] > y[7];
    if (x[8] != y[8]) return x[8] > y[8];
    return x[9] < y[9];
}
__host__ __device__ __forceinline__ bool an_rec_same_place(const int32_t *x, const int32_t *y) {
    for (int k = 0; k < 7; k++) if (x[k] != y[k]) return false;
    return true;
}
// B is better than A (two records of one sequence that differ in place): a higher score, then the smaller order key
__host__ __device__ __forceinline__ bool an_rec_better(const int32_t *b, const int32_t *a) { return b[7] != a[7] ? b[7] > a[7] : an_rec_less(b, a); }
// B covers at least 80 % of A
__host__ __device__ __forceinline__ bool an_rec_covers(const int32_t *b, const int32_t *a) {
    const int64_t lo = a[1] > b[1] ? a[1] : b[1], hi = a[2] < b[2] ? a[2] : b[2];
    return hi > lo && 5 * (hi - lo) >= 4 * ((int64_t)a[2] - a[1]);
}
// v: n records in the order of an_rec_less -> the records that stay, in that order; adds the duplicates to *dup, the dominated to *dom.
// A window is shorter than 32 768 bases: a record that overlaps A begins less than 32 768 before A's end.
static void an_resolve(std::vector<AnRec> &v, int64_t *dup, int64_t *dom) {
    std::vector<AnRec> u;
    for (size_t k = 0; k < v.size(); k++) {
        if (k > 0 && an_rec_same_place(v[k].f, v[k - 1].f)) { (*dup)++; continue; }
        u.push_back(v[k]);
    }
    v.clear();
    size_t from = 0;
    for (size_t a = 0; a < u.size(); a++) {
        const int32_t *A = u[a].f;
        while (from < a && (u[from].f[0] != A[0] || (int64_t)u[from].f[1] + HITE_PAIRHSP_MAX_LEN <= A[1])) from++;
        bool dropped = false;
        for (size_t b = from; b < u.size() && !dropped; b++) {
            const int32_t *B = u[b].f;
            if (B[0] != A[0] || B[1] >= A[2]) break;
            if (b != a && an_rec_covers(B, A) && an_rec_better(B, A)) dropped = true;
        }
        if (dropped) (*dom)++;
        else v.push_back(u[a]);
    }
}
// <<< annotate_resolve

// a piece of a batch: its sequence, its bases [begin, end) of the sequence and, with `lead` bases before them and `trail` after, its
// bytes at [at, at + lead + (end - begin) + trail) of the batch
struct AnPiece { int64_t seq_len; int32_t seq, begin, end, lead, trail; int64_t at; };
struct AnTask { int32_t piece, t, g_lo, g_hi, d_lo, d_hi; };      // a run: g in the sequence, d = g - q
enum { AN_C_WORDS = 0, AN_C_SILENT, AN_C_HITS, AN_C_RUNS, AN_C_N };

// the piece of the batch that holds byte gp (at[0] = 0 <= gp < at[n])
__device__ __forceinline__ int an_piece_of(const AnPiece *__restrict__ pc, int n, int64_t gp) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pc[mid].at <= gp) lo = mid; else hi = mid;
    }
    return lo;
}

// the first entry of the sorted table with a key >= w
__device__ __forceinline__ int64_t an_lower(const unsigned long long *__restrict__ keys, int64_t n, unsigned long long w) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one thread per table entry: it is silenced when its word has more than HITE_ANNOT_MAX_OCC entries
__global__ __launch_bounds__(256) void an_silent_kernel(const unsigned long long *__restrict__ keys, int64_t nw, unsigned long long *__restrict__ counters) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool silent = false;
    if (e < nw) {
        const unsigned long long w = keys[e];
        int n = 1;
        for (int64_t k = e - 1; k >= 0 && n <= HITE_ANNOT_MAX_OCC && keys[k] == w; k--) n++;
        for (int64_t k = e + 1; k < nw && n <= HITE_ANNOT_MAX_OCC && keys[k] == w; k++) n++;
        silent = n > HITE_ANNOT_MAX_OCC;
    }
    (void)wave_take_flag(silent, &counters[AN_C_SILENT]);
}

// one thread per byte of the batch: the hits of the position (step 2); written while they fit hit_cap, counted always
__global__ __launch_bounds__(256) void an_hit_kernel(const uint8_t *__restrict__ seqs, int64_t nb, const AnPiece *__restrict__ pc, int n_piece,
                                                     const unsigned long long *__restrict__ tkeys, const unsigned *__restrict__ tvals, int64_t nw,
                                                     const int64_t *__restrict__ text_off, int n_text, unsigned long long *__restrict__ hits,
                                                     int64_t hit_cap, unsigned long long *__restrict__ counters) {
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned n = 0;
    int64_t first = 0;
    if (gp < nb) {
        const AnPiece P = pc[an_piece_of(pc, n_piece, gp)];
        const int64_t lo = P.at + P.lead, hi = lo + (P.end - P.begin);
        if (gp >= lo && gp + HITE_ANNOT_WORD <= hi) {
            int codes[HITE_ANNOT_WORD];
#pragma unroll
            for (int k = 0; k < HITE_ANNOT_WORD; k++) codes[k] = hsp_code(seqs[gp + k]);
            const unsigned long long w = hsp_word_key<HITE_ANNOT_WORD>(codes);
            if (w != AN_NO_WORD) {
                first = an_lower(tkeys, nw, w);
                while (n <= HITE_ANNOT_MAX_OCC && first + n < nw && tkeys[first + n] == w) n++;
                if (n > HITE_ANNOT_MAX_OCC) n = 0;
            }
        }
    }
    const unsigned long long at = wave_take_count(n, &counters[AN_C_HITS]);
    for (unsigned k = 0; k < n; k++) {
        if ((int64_t)(at + k) >= hit_cap) break;
        const int64_t tp = tvals[first + k];
        const int t = last_le(text_off, n_text, tp);
        hits[at + k] = an_hit_pack((uint32_t)t, (uint32_t)(tp - text_off[t]), (uint32_t)gp);
    }
}

__global__ __launch_bounds__(256) void an_run_key_kernel(const unsigned long long *__restrict__ hits, int64_t nh, const AnPiece *__restrict__ pc,
                                                         int n_piece, int lam, int bin_bits, int pos_bits, unsigned long long *__restrict__ keys,
                                                         unsigned *__restrict__ vals) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    const unsigned long long x = hits[h];
    const uint32_t gp = an_hit_gp(x), q = an_hit_q(x);
    const AnPiece P = pc[an_piece_of(pc, n_piece, gp)];
    const uint32_t diag = an_diag((int64_t)gp - P.at - P.lead, q);
    keys[h] = an_run_key(an_hit_t(x), diag, gp, lam, bin_bits, pos_bits);
    vals[h] = diag;
}

// one thread per sorted hit: the one that begins a chain of equal (piece, t, bin) walks it to its end and emits its runs
__global__ __launch_bounds__(256) void an_run_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ vals, int64_t nh,
                                                     int bin_bits, int pos_bits, const AnPiece *__restrict__ pc, int n_piece,
                                                     AnTask *__restrict__ tasks, int64_t task_cap, unsigned long long *__restrict__ counters) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    const unsigned long long key = keys[h], group = an_key_group(key, pos_bits);
    const int64_t gp = an_key_pos(key, pos_bits);
    const int p = an_piece_of(pc, n_piece, gp);
    const AnPiece P = pc[p];
    const int64_t lo = P.at + P.lead, hi = lo + (P.end - P.begin);      // the positions of the piece's own bases
    if (h > 0) {
        const unsigned long long kp = keys[h - 1];
        const int64_t gpp = an_key_pos(kp, pos_bits);
        if (an_key_group(kp, pos_bits) == group && gpp >= lo && gp - gpp <= HITE_ANNOT_GAP) return;      // inside a chain
    }
    const int32_t t = (int32_t)(group >> bin_bits);
    const int64_t to_seq = (int64_t)P.begin - lo;      // position in the batch -> position in the sequence
    const int64_t to_d = (int64_t)P.begin - HITE_ANNOT_MAX_LIB_LEN;
    AnChain c;
    an_chain_start(c, gp, vals[h]);
    auto emit = [&]() {
        if (c.n < HITE_ANNOT_MIN_HITS) return;
        const unsigned long long at = atomicAdd(&counters[AN_C_RUNS], 1ull);
        if ((int64_t)at < task_cap) {
            AnTask T = {p, t, (int32_t)(c.g_first + to_seq), (int32_t)(c.g_last + to_seq), (int32_t)((int64_t)c.d_lo + to_d), (int32_t)((int64_t)c.d_hi + to_d)};
            tasks[at] = T;
        }
    };
    for (int64_t k = h + 1; k < nh; k++) {
        const unsigned long long kk = keys[k];
        const int64_t g = an_key_pos(kk, pos_bits);
        if (an_key_group(kk, pos_bits) != group || g >= hi || g - c.g_last > HITE_ANNOT_GAP) break;
        if (an_chain_breaks(c, g)) { emit(); an_chain_start(c, g, vals[k]); }
        else an_chain_add(c, g, vals[k]);
    }
    emit();
}

// wavefront per run: step 4 of the header with its redo loop.  A window that would leave the bytes the batch holds of the sequence is
// not read: the run is marked (out[11]) and the call fails -- the margins are sized so that this cannot happen.
__global__ __launch_bounds__(AN_WAVES * 64) void an_extend_kernel(const AnTask *__restrict__ tasks, int64_t n_tasks, const uint8_t *__restrict__ seqs,
                                                                  const AnPiece *__restrict__ pc, const uint8_t *__restrict__ text,
                                                                  const int64_t *__restrict__ text_off, int32_t *__restrict__ out) {
    __shared__ long long s_bnd_a[AN_WAVES][2 * HSP_BAND];
    __shared__ uint32_t s_bnd_b[AN_WAVES][2 * HSP_BAND];
    const int lane = lane_id(), w = wave_id();
    for (int64_t k = (int64_t)blockIdx.x * AN_WAVES + w; k < n_tasks; k += (int64_t)gridDim.x * AN_WAVES) {
        const AnTask T = tasks[k];
        const AnPiece P = pc[T.piece];
        const int64_t have_lo = (int64_t)P.begin - P.lead, have_hi = (int64_t)P.end + P.trail;      // the bases of the sequence in the batch
        const uint8_t *s = seqs + P.at - have_lo;      // s[x]: base x of the sequence, for have_lo <= x < have_hi
        const uint8_t *q = text + text_off[T.t];
        const int64_t L = text_off[T.t + 1] - text_off[T.t];
        const int64_t dc = ((int64_t)T.d_lo + T.d_hi) >> 1;
        int pl = 0, pr = 0, n_align = 0, found = 0, fault = 0;
        int64_t qs = 0, qe = 0, gs = 0, ge = 0;
        HspBest h = {0, 0, 0};
        for (;;) {
            const AnWin W = an_window(L, P.seq_len, T.g_lo, T.g_hi, dc, pl, pr);
            const int m = (int)(W.qe - W.qb), n = (int)(W.se - W.sb);
            n_align++;
            found = 0;
            if (W.qe - W.qb < 1 || W.se - W.sb < 1 || W.qe - W.qb >= HITE_PAIRHSP_MAX_LEN || W.se - W.sb >= HITE_PAIRHSP_MAX_LEN || W.sb < have_lo ||
                W.se > have_hi) { fault = 1; break; }
            h = hsp_align(q + W.qb, m, s + W.sb, W.dlo, W.dlo + HSP_BAND - 1, 1, m, 1, n, s_bnd_a[w], s_bnd_b[w]);
            if (hsp_score(h.a) < HITE_PAIRHSP_MIN_SCORE) break;
            found = 1;
            qs = W.qb + hsp_q_start(h.b) - 1; qe = W.qb + hsp_q_end(h.e);
            gs = W.sb + hsp_s_start(h.b) - 1; ge = W.sb + hsp_s_end(h.e);
            const int step = an_pad_steps(W, L, qs, qe, pl, pr);
            if (step == 0 || n_align > HITE_ANNOT_MAX_REDO) break;
            pl += step & 1;
            pr += step >> 1;
        }
        if (lane == 0) {
            int32_t *o = out + k * AN_OUT_WORDS;
            o[0] = found; o[1] = P.seq; o[2] = (int32_t)gs; o[3] = (int32_t)ge; o[4] = T.t; o[5] = (int32_t)qs; o[6] = (int32_t)qe;
            o[7] = hsp_score(h.a); o[8] = hsp_matches(h.a); o[9] = hsp_columns(h.a); o[10] = n_align; o[11] = fault;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
#define AN_ALLOC(pool, ptr, bytes) HITE_CHECK(ctx, (pool).alloc(ptr, (size_t)(bytes)))

// the table of a call on the device
struct AnTable {
    DevPool B;
    uint8_t *d_text = nullptr;
    int64_t *d_off = nullptr;
    unsigned long long *d_keys = nullptr;
    unsigned *d_vals = nullptr;
    int64_t nw = 0;      // entries (the sorted positions with a word come first)
    int n_text = 0;
};

static int an_table(hite_ctx *ctx, const std::vector<uint8_t> &text, const std::vector<int64_t> &off, AnTable &T, int64_t *st) {
    hipStream_t stream = nullptr;
    const int64_t nb = (int64_t)text.size();
    T.n_text = (int)off.size() - 1;
    unsigned long long *d_cnt;
    AN_ALLOC(T.B, T.d_text, nb + 16);
    AN_ALLOC(T.B, T.d_off, off.size() * 8);
    AN_ALLOC(T.B, T.d_keys, (nb + 1) * 8);
    AN_ALLOC(T.B, T.d_vals, (nb + 1) * 4);
    AN_ALLOC(T.B, d_cnt, AN_C_N * 8);
    HITE_CHECK(ctx, hipMemcpyAsync(T.d_text, text.data(), (size_t)nb, hipMemcpyHostToDevice, stream));
    HITE_CHECK(ctx, hipMemcpyAsync(T.d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, stream));
    HITE_CHECK(ctx, hipMemsetAsync(d_cnt, 0, AN_C_N * 8, stream));
    struct SortGuard { Sorter S; bool on = false; ~SortGuard() { if (on) sorter_free(S); } } G;
    G.on = true;
    int rc = sorter_init(G.S, ctx, stream, nb);
    if (rc) return rc;
    int tk = hite_prof_begin(ctx, "annot_table", stream);
    hipLaunchKernelGGL(hsp_word_kernel<HITE_ANNOT_WORD>, dim3(grid256(nb)), dim3(256), 0, stream, T.d_text, T.d_off, T.n_text, nb, T.d_keys, T.d_vals,
                       d_cnt + AN_C_WORDS);
    HITE_CHECK(ctx, hipGetLastError());
    rc = sorter_sort_bits(G.S, T.d_keys, T.d_vals, nb, 0, AN_WORD_BITS);
    if (rc) return rc;
    unsigned long long h_cnt[AN_C_N];
    HITE_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
    HITE_CHECK(ctx, hipStreamSynchronize(stream));
    T.nw = (int64_t)h_cnt[AN_C_WORDS];
    if (T.nw > 0) {
        hipLaunchKernelGGL(an_silent_kernel, dim3(grid256(T.nw)), dim3(256), 0, stream, T.d_keys, T.nw, d_cnt);
        HITE_CHECK(ctx, hipGetLastError());
        HITE_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
    }
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipStreamSynchronize(stream));
    st[0] = T.nw;
    st[1] = (int64_t)h_cnt[AN_C_SILENT];
    return HITE_OK;
}

// one batch of pieces, nb > 0 bytes in all (h_seq: the bytes, laid out as the pieces say); appends the HSPs found, adds to st[3 .. 7]
static int an_batch(hite_ctx *ctx, const AnTable &T, const std::vector<AnPiece> &pieces, const std::vector<uint8_t> &h_seq, std::vector<AnRec> &found,
                    int64_t *st) {
    const int64_t nb = (int64_t)h_seq.size();
    const int n_piece = (int)pieces.size();
    hipStream_t stream = nullptr;
    DevPool B;
    uint8_t *d_seq; AnPiece *d_pc; unsigned long long *d_cnt, *d_hits;
    AN_ALLOC(B, d_seq, nb + 16);
    AN_ALLOC(B, d_pc, (size_t)n_piece * sizeof(AnPiece));
    AN_ALLOC(B, d_cnt, AN_C_N * 8);
    HITE_CHECK(ctx, hipMemcpyAsync(d_seq, h_seq.data(), (size_t)nb, hipMemcpyHostToDevice, stream));
    HITE_CHECK(ctx, hipMemcpyAsync(d_pc, pieces.data(), (size_t)n_piece * sizeof(AnPiece), hipMemcpyHostToDevice, stream));
    unsigned long long h_cnt[AN_C_N];
    int64_t hit_cap = nb / 4 + 4096, nh = 0;
    for (int pass = 0;; pass++) {       // the second pass knows the room
        AN_ALLOC(B, d_hits, hit_cap * 8);
        HITE_CHECK(ctx, hipMemsetAsync(d_cnt, 0, AN_C_N * 8, stream));
        const int tk = hite_prof_begin(ctx, "annot_hits", stream);
        hipLaunchKernelGGL(an_hit_kernel, dim3(grid256(nb)), dim3(256), 0, stream, d_seq, nb, d_pc, n_piece, T.d_keys, T.d_vals, T.nw, T.d_off, T.n_text,
                           d_hits, hit_cap, d_cnt);
        hite_prof_end(ctx, tk, stream);
        HITE_CHECK(ctx, hipGetLastError());
        HITE_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
        HITE_CHECK(ctx, hipStreamSynchronize(stream));
        nh = (int64_t)h_cnt[AN_C_HITS];
        if (nh <= hit_cap) break;
        if (pass > 0) { snprintf(ctx->err, sizeof(ctx->err), "hite_annotate: %lld hits after a count of %lld", (long long)nh, (long long)hit_cap); return HITE_EHIP; }
        hit_cap = nh;
    }
    st[3] += nh;
    if (nh < HITE_ANNOT_MIN_HITS) return HITE_OK;

    // the runs of both lattices
    const int64_t task_cap = 2 * (nh / HITE_ANNOT_MIN_HITS) + 2;
    unsigned long long *d_keys; unsigned *d_vals; AnTask *d_tasks;
    AN_ALLOC(B, d_keys, (nh + 1) * 8);
    AN_ALLOC(B, d_vals, (nh + 1) * 4);
    AN_ALLOC(B, d_tasks, task_cap * sizeof(AnTask));
    struct SortGuard { Sorter S; bool on = false; ~SortGuard() { if (on) sorter_free(S); } } G;
    G.on = true;
    int rc = sorter_init(G.S, ctx, stream, nh);
    if (rc) return rc;
    int64_t widest = 0;
    for (const AnPiece &P : pieces) widest = std::max<int64_t>(widest, P.end - P.begin);
    const int pos_bits = hsp_bits((unsigned long long)(nb - 1));
    const int bin_bits = hsp_bits((unsigned long long)((widest + HITE_ANNOT_MAX_LIB_LEN + HITE_ANNOT_LATTICE) >> HITE_ANNOT_BIN_SHIFT));
    const int t_bits = hsp_bits((unsigned long long)(T.n_text - 1));
    if (pos_bits + bin_bits + t_bits > 64) { snprintf(ctx->err, sizeof(ctx->err), "hite_annotate: a key of %d bits", pos_bits + bin_bits + t_bits); return HITE_EHIP; }
    HITE_CHECK(ctx, hipMemsetAsync(d_cnt, 0, AN_C_N * 8, stream));
    int tk = hite_prof_begin(ctx, "annot_runs", stream);
    for (int lam = 0; lam <= HITE_ANNOT_LATTICE; lam += HITE_ANNOT_LATTICE) {
        hipLaunchKernelGGL(an_run_key_kernel, dim3(grid256(nh)), dim3(256), 0, stream, d_hits, nh, d_pc, n_piece, lam, bin_bits, pos_bits, d_keys, d_vals);
        HITE_CHECK(ctx, hipGetLastError());
        if ((rc = sorter_sort_bits(G.S, d_keys, d_vals, nh, 0, pos_bits + bin_bits + t_bits))) return rc;
        hipLaunchKernelGGL(an_run_kernel, dim3(grid256(nh)), dim3(256), 0, stream, d_keys, d_vals, nh, bin_bits, pos_bits, d_pc, n_piece, d_tasks, task_cap,
                           d_cnt);
        HITE_CHECK(ctx, hipGetLastError());
    }
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, stream));
    HITE_CHECK(ctx, hipStreamSynchronize(stream));
    const int64_t n_tasks = (int64_t)h_cnt[AN_C_RUNS];
    st[4] += n_tasks;
    if (n_tasks > task_cap) { snprintf(ctx->err, sizeof(ctx->err), "hite_annotate: %lld runs beyond the room for %lld", (long long)n_tasks, (long long)task_cap); return HITE_EHIP; }
    if (n_tasks == 0) return HITE_OK;

    int32_t *d_out;
    AN_ALLOC(B, d_out, n_tasks * AN_OUT_WORDS * 4);
    const unsigned blocks = (unsigned)std::min<int64_t>((n_tasks + AN_WAVES - 1) / AN_WAVES, AN_MAX_BLOCKS);
    tk = hite_prof_begin(ctx, "annot_extend", stream);
    hipLaunchKernelGGL(an_extend_kernel, dim3(blocks), dim3(AN_WAVES * 64), 0, stream, d_tasks, n_tasks, d_seq, d_pc, T.d_text, T.d_off, d_out);
    hite_prof_end(ctx, tk, stream);
    HITE_CHECK(ctx, hipGetLastError());
    std::vector<int32_t> h_out((size_t)n_tasks * AN_OUT_WORDS);
    HITE_CHECK(ctx, hipMemcpyAsync(h_out.data(), d_out, h_out.size() * 4, hipMemcpyDeviceToHost, stream));
    HITE_CHECK(ctx, hipStreamSynchronize(stream));
    for (int64_t k = 0; k < n_tasks; k++) {
        const int32_t *o = h_out.data() + k * AN_OUT_WORDS;
        if (o[11]) { snprintf(ctx->err, sizeof(ctx->err), "hite_annotate: a window beyond the bases of its batch"); return HITE_EHIP; }
        st[5] += o[10];
        st[6] += o[10] - 1;
        if (!o[0]) { st[7]++; continue; }
        memcpy(found.emplace_back().f, o + 1, 9 * sizeof(int32_t));      // (seq, gs, ge, t, qs, qe, score, matches, columns): an_finish makes the record
    }
    return HITE_OK;
}

extern "C" int hite_annotate(hite_ctx *ctx, int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int32_t n_lib, const uint8_t *lib,
                             const int64_t *lib_off, int32_t piece_len, int64_t cap, int32_t *recs, int64_t *n_out, int8_t *lib_status, int64_t *stats) {
    if (!ctx || !n_out || n_seq < 0 || n_seq >= ((int64_t)1 << 31) || n_lib < 0 || n_lib > HITE_ANNOT_MAX_LIB || cap < 0 || (cap > 0 && !recs) ||
        (n_seq > 0 && !seq_off) || (n_lib > 0 && !lib_off))
        return HITE_EINVAL;
    if (piece_len != 0 && (piece_len < HITE_ANNOT_MIN_PIECE || piece_len > HITE_ANNOT_PIECE)) return HITE_EINVAL;
    *n_out = 0;
    int64_t st[HITE_ANNOT_STATS] = {0};
    if (stats) memset(stats, 0, sizeof(st));
    if (n_seq > 0) {
        if (!csr_sorted(seq_off, n_seq)) return HITE_EINVAL;
        for (int64_t q = 0; q < n_seq; q++) if (seq_off[q + 1] - seq_off[q] >= ((int64_t)1 << 31)) return HITE_EINVAL;
        if (seq_off[n_seq] > seq_off[0] && !seqs) return HITE_EINVAL;
    }
    if (n_lib > 0) {
        if (!csr_sorted(lib_off, n_lib)) return HITE_EINVAL;
        if (lib_off[n_lib] > lib_off[0] && !lib) return HITE_EINVAL;
    }
    const int64_t P = piece_len ? piece_len : HITE_ANNOT_PIECE;
    const int64_t batch_bytes = ctx->annot_batch_bytes > 0 ? std::min(ctx->annot_batch_bytes, AN_BATCH_BYTES) : AN_BATCH_BYTES;
    try {
        // step 1: the texts
        std::vector<uint8_t> text;
        std::vector<int64_t> off((size_t)2 * n_lib + 1, 0);
        for (int32_t e = 0; e < n_lib; e++) {
            const int64_t L = lib_off[e + 1] - lib_off[e];
            const bool ok = L <= HITE_ANNOT_MAX_LIB_LEN;
            if (lib_status) lib_status[e] = ok ? 0 : -1;
            if (!ok) st[2]++;
            const uint8_t *b = lib + lib_off[e];
            if (ok) {
                text.insert(text.end(), b, b + L);
                off[(size_t)2 * e + 1] = (int64_t)text.size();
                for (int64_t k = L - 1; k >= 0; k--) text.push_back(an_comp(b[k]));
            } else off[(size_t)2 * e + 1] = (int64_t)text.size();
            off[(size_t)2 * e + 2] = (int64_t)text.size();
        }
        std::vector<AnRec> found;
        const bool any = n_seq > 0 && seq_off[n_seq] - seq_off[0] >= HITE_ANNOT_WORD;
        if ((int64_t)text.size() >= HITE_ANNOT_WORD) {
            HITE_CHECK(ctx, hipSetDevice(ctx->device));
            AnTable T;
            int rc = an_table(ctx, text, off, T, st);
            if (rc) return rc;
            // step 2: pieces, as many to a batch as stay within the bound; a larger one goes alone
            std::vector<AnPiece> pieces;
            std::vector<uint8_t> h_seq;
            auto flush = [&]() -> int {
                if (pieces.empty()) return HITE_OK;
                const int r = an_batch(ctx, T, pieces, h_seq, found, st);
                pieces.clear();
                h_seq.clear();
                return r;
            };
            for (int64_t s = 0; any && T.nw > 0 && s < n_seq; s++) {
                const int64_t len = seq_off[s + 1] - seq_off[s];
                for (int64_t k = 0; k * P < len; k++) {
                    AnPiece pc;
                    pc.seq = (int32_t)s; pc.seq_len = len;
                    pc.begin = (int32_t)(k * P);
                    pc.end = (int32_t)std::min<int64_t>(len, (k + 1) * P + HITE_ANNOT_OVERLAP);
                    if (pc.end - pc.begin < HITE_ANNOT_WORD) continue;
                    pc.lead = (int32_t)std::min<int64_t>(pc.begin, AN_HALO);
                    pc.trail = (int32_t)std::min<int64_t>(len - pc.end, AN_HALO);
                    const int64_t bytes = (int64_t)pc.lead + (pc.end - pc.begin) + pc.trail;
                    if (!pieces.empty() && (int64_t)h_seq.size() + bytes > batch_bytes && (rc = flush())) return rc;
                    pc.at = (int64_t)h_seq.size();
                    const uint8_t *b = seqs + seq_off[s] + pc.begin - pc.lead;
                    h_seq.insert(h_seq.end(), b, b + bytes);
                    pieces.push_back(pc);
                }
            }
            if ((rc = flush())) return rc;
            hite_prof_resolve(ctx);
        }
        // steps 5 and 6; the q interval of a reverse-complement text goes to the entry's forward strand first
        for (AnRec &r : found) {
            const int32_t t = r.f[3], qs = r.f[4], qe = r.f[5], score = r.f[6], matches = r.f[7], columns = r.f[8];
            const int32_t L = (int32_t)(lib_off[(t >> 1) + 1] - lib_off[t >> 1]);
            r.f[3] = t >> 1; r.f[4] = t & 1;
            r.f[5] = (t & 1) ? L - qe : qs; r.f[6] = (t & 1) ? L - qs : qe;
            r.f[7] = score; r.f[8] = matches; r.f[9] = columns;
        }
        st[8] = (int64_t)found.size();
        std::sort(found.begin(), found.end(), [](const AnRec &x, const AnRec &y) { return an_rec_less(x.f, y.f); });
        an_resolve(found, &st[9], &st[10]);
        const int64_t total = (int64_t)found.size();
        for (int64_t k = 0; k < total && k < cap; k++) memcpy(recs + HITE_ANNOT_REC * k, found[(size_t)k].f, sizeof(found[(size_t)k].f));
        st[11] = total;
        *n_out = total;
        if (stats) memcpy(stats, st, sizeof(st));
        return total > cap ? HITE_ECAP : HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

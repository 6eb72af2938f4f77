// hite_helitron.hip -- Helitron candidate scan: the in-tree stage where the reference runs HelitronScanner (scanHead, scanTail,
// pairends, draw -pure_helitron per 50 kb part of longest_repeats_{i}.flanked.fa; judge_Helitron_transposons.py:27-34, Util.py:263).
// The tool is not pinned (no machine of the project runs it): parity is the written definition in include/hite_gpu.h ("Helitron
// candidate scan"), its CPU twin tests/helitron_twin.py, HIP == twin record for record and score for score.
//
// Four passes, all on the forward text only (the minus strand is the same text read backwards through the complement):
//  anchors  one thread per base marks the four kinds of anchor that can begin at it: a plus head `TC`, a minus head (`GA`, = TC of the
//           reverse complement), a plus tail `CT[AG][AG]` (marked at its last base) and a minus tail (`[CT][CT]AG`, at its first).
//           Count per base -> exclusive scan (hite_scan.h) -> the anchors in base order, with their sequence.
//  scores   ONE WAVEFRONT PER ANCHOR.  The window of an anchor is the up to 63 + 32 = 95 bytes on the far side of its literal, read
//           outwards (heads: downstream on their strand; tails: upstream).  Lane l fetches window bytes l and l + 64; three ballots per
//           half turn them into bit planes (low code bit, high code bit, not-ACGT), 2 x 64 bits each, held by every lane.  The pattern
//           tables (<= 1024 per side, 16 bytes each: the body as the same three planes in reading order, care bits, gap range) sit in
//           LDS; lane l tests patterns l, l + 64, ...: a test is ((lo ^ P.lo) | (hi ^ P.hi) | nn) & P.care == 0 on the 32 plane bits
//           at each gap of the range that keeps the body inside the sequence.  The score is the sum of popcounts of the ballots.
//  lists    the anchors that reach their threshold, split into plus heads, minus heads, plus tails, minus tails (two scans of packed
//           counters), each list in base order.
//  pairs    one thread per head: binary search of its strand's tail list for the nearest tail downstream whose length is >= len_min;
//           it pairs when that length is <= len_max and the tail lies in the same sequence.  A scan of the found flags and four
//           binary searches per record (the sequence's first head of either strand, the next sequence's) place it in the order
//           (sequence, strand, start, end) with no sort and no atomic.
// Bit planes rather than 2-bit packed bases: a ballot builds a plane in one step, and a 32-position body is one 32-bit word per plane.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include "hite_scan.h"
#include <vector>
#include <new>

#define HELI_WAVES 4
#define HELI_WIN (HITE_HELITRON_MAX_GAP + HITE_HELITRON_MAX_BODY)      // 95 window bytes
#define HELI_HEAD_PLUS 0
#define HELI_HEAD_MINUS 1
#define HELI_TAIL_PLUS 2
#define HELI_TAIL_MINUS 3

// >>> helitron_score
// a pattern as the score pass reads it: body planes in reading order (bit k = the k-th body position met when walking away from the
// anchor), care bit per position (0 under a `.`), g = gap_min | gap_max << 8 | body_len << 16
struct HeliPat { uint32_t lo, hi, care, g; };
// a byte as a base code A 0 / C 1 / G 2 / T 3 (upper case only), anything else 4; comp: of the complementary base
__device__ __forceinline__ int heli_code(uint8_t c, bool comp) {
    int b;
    switch (c) {
        case 'A': b = 0; break;
        case 'C': b = 1; break;
        case 'G': b = 2; break;
        case 'T': b = 3; break;
        default: return 4;
    }
    return comp ? 3 - b : b;
}
// 32 bits of the 128-bit plane (w0 = positions 0..63, w1 = 64..127) from position g <= 63 on
__device__ __forceinline__ uint32_t heli_take(uint64_t w0, uint64_t w1, int g) {
    const uint64_t x = g ? ((w0 >> g) | (w1 << (64 - g))) : w0;
    return (uint32_t)x;
}
// does pattern P match the window (planes lo / hi / nn, `avail` positions inside the sequence) at some gap of its range?
__device__ __forceinline__ bool heli_match(uint64_t lo0, uint64_t lo1, uint64_t hi0, uint64_t hi1, uint64_t nn0, uint64_t nn1, int avail,
                                           HeliPat P) {
    const int gmin = (int)(P.g & 0xFF), gmax = (int)((P.g >> 8) & 0xFF), bl = (int)((P.g >> 16) & 0xFF);
    const int top = gmax < avail - bl ? gmax : avail - bl;
    for (int g = gmin; g <= top; g++) {
        const uint32_t x = ((heli_take(lo0, lo1, g) ^ P.lo) | (heli_take(hi0, hi1, g) ^ P.hi) | heli_take(nn0, nn1, g)) & P.care;
        if (!x) return true;
    }
    return false;
}
// the four anchors that may begin at byte i of a sequence [b, e): bit kind set when the literal lies inside the sequence
__device__ __forceinline__ int heli_anchor_kinds(const uint8_t *s, int64_t i, int64_t b, int64_t e) {
    int k = 0;
    const uint8_t c0 = s[i];
    if (i + 1 < e) {
        const uint8_t c1 = s[i + 1];
        if (c0 == 'T' && c1 == 'C') k |= 1 << 0;       // plus head at p = i
        if (c0 == 'G' && c1 == 'A') k |= 1 << 1;       // minus head: TC of the reverse complement
    }
    if (i - 3 >= b && (c0 == 'A' || c0 == 'G')) {      // plus tail, marked at its last base q = i
        const uint8_t r = s[i - 1];
        if (s[i - 3] == 'C' && s[i - 2] == 'T' && (r == 'A' || r == 'G')) k |= 1 << 2;
    }
    if (i + 3 < e && (c0 == 'C' || c0 == 'T')) {       // minus tail: CT[AG][AG] of the reverse complement, marked at its first base
        const uint8_t y = s[i + 1];
        if ((y == 'C' || y == 'T') && s[i + 2] == 'A' && s[i + 3] == 'G') k |= 1 << 3;
    }
    return k;
}
// where the window of an anchor of `kind` at byte i begins, the direction it is read in and how many of its bytes the sequence holds
__device__ __forceinline__ void heli_window(int kind, int64_t i, int64_t b, int64_t e, int64_t *w0, int *dir, int64_t *avail) {
    switch (kind) {
        case 0: *w0 = i + 2; *dir = 1; *avail = e - (i + 2); break;
        case 1: *w0 = i - 1; *dir = -1; *avail = i - b; break;
        case 2: *w0 = i - 4; *dir = -1; *avail = i - 3 - b; break;
        default: *w0 = i + 4; *dir = 1; *avail = e - (i + 4); break;
    }
}
// the caller's record -> the score pass's; a tail body is met from its last position on.  false: beyond a limit or malformed
static bool heli_compile(const hite_lcv &r, bool tail, HeliPat *out) {
    const int bl = r.body_len;
    if (bl < 1 || bl > HITE_HELITRON_MAX_BODY || r.gap_max > HITE_HELITRON_MAX_GAP || r.gap_min > r.gap_max) return false;
    HeliPat P = {0, 0, 0, (uint32_t)r.gap_min | (uint32_t)r.gap_max << 8 | (uint32_t)bl << 16};
    if (bl < 32 && ((r.body >> (2 * bl)) || (r.care >> (2 * bl)))) return false;
    if (r.body & ~r.care) return false;
    for (int j = 0; j < bl; j++) {
        const unsigned c = (unsigned)(r.care >> (2 * j)) & 3u, v = (unsigned)(r.body >> (2 * j)) & 3u;
        if (c != 0 && c != 3) return false;
        const int d = tail ? bl - 1 - j : j;
        P.lo |= (uint32_t)(v & 1) << d; P.hi |= (uint32_t)(v >> 1) << d; P.care |= (uint32_t)(c ? 1 : 0) << d;
    }
    *out = P;
    return true;
}
// <<< helitron_score

__global__ __launch_bounds__(256) void heli_anchor_count_kernel(const uint8_t *__restrict__ s, const int64_t *__restrict__ off, int64_t n,
                                                                int64_t nb, int32_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t q = last_le(off, n, i);
    cnt[i] = __popc(heli_anchor_kinds(s, i, off[q], off[q + 1]));
}

__global__ __launch_bounds__(256) void heli_anchor_fill_kernel(const uint8_t *__restrict__ s, const int64_t *__restrict__ off, int64_t n,
                                                               int64_t nb, const int64_t *__restrict__ pos, int64_t *__restrict__ key,
                                                               int32_t *__restrict__ seq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t q = last_le(off, n, i);
    const int k = heli_anchor_kinds(s, i, off[q], off[q + 1]);
    int64_t at = pos[i];
    for (int kind = 0; kind < 4; kind++)
        if (k >> kind & 1) { key[at] = i * 4 + kind; seq[at] = (int32_t)q; at++; }
}

__global__ __launch_bounds__(HELI_WAVES * 64) void heli_score_kernel(const uint8_t *__restrict__ s, const int64_t *__restrict__ off,
                                                                     const int64_t *__restrict__ key, const int32_t *__restrict__ seq,
                                                                     int64_t n_anchor, const HeliPat *__restrict__ head, int32_t n_head,
                                                                     const HeliPat *__restrict__ tail, int32_t n_tail,
                                                                     int32_t *__restrict__ score) {
    __shared__ HeliPat s_pat[2 * HITE_HELITRON_MAX_PATTERNS];
    for (int k = threadIdx.x; k < n_head; k += HELI_WAVES * 64) s_pat[k] = head[k];
    for (int k = threadIdx.x; k < n_tail; k += HELI_WAVES * 64) s_pat[HITE_HELITRON_MAX_PATTERNS + k] = tail[k];
    __syncthreads();
    const int lane = lane_id();
    for (int64_t a = (int64_t)blockIdx.x * HELI_WAVES + wave_id(); a < n_anchor; a += (int64_t)gridDim.x * HELI_WAVES) {
        const int64_t ky = key[a];
        const int kind = (int)(ky & 3);
        const int64_t i = ky >> 2, q = seq[a];
        int64_t w0, av;
        int dir;
        heli_window(kind, i, off[q], off[q + 1], &w0, &dir, &av);
        const int avail = av > HELI_WIN ? HELI_WIN : (int)av;
        const bool comp = kind == HELI_HEAD_MINUS || kind == HELI_TAIL_MINUS;
        const int c0 = lane < avail ? heli_code(s[w0 + (int64_t)dir * lane], comp) : 0;
        const int c1 = lane + 64 < avail ? heli_code(s[w0 + (int64_t)dir * (lane + 64)], comp) : 0;
        const uint64_t lo0 = __ballot(c0 & 1), hi0 = __ballot(c0 & 2), nn0 = __ballot(c0 & 4);
        const uint64_t lo1 = __ballot(c1 & 1), hi1 = __ballot(c1 & 2), nn1 = __ballot(c1 & 4);
        const bool is_head = kind == HELI_HEAD_PLUS || kind == HELI_HEAD_MINUS;
        const HeliPat *tab = is_head ? s_pat : s_pat + HITE_HELITRON_MAX_PATTERNS;
        const int np = is_head ? n_head : n_tail;
        int total = 0;
        for (int base = 0; base < np; base += 64) {
            const int k = base + lane;
            const bool m = k < np && heli_match(lo0, lo1, hi0, hi1, nn0, nn1, avail, tab[k]);
            total += __popcll(__ballot(m));
        }
        if (lane == 0) score[a] = total;
    }
}

// packed counters of the anchors that reach their threshold: pass 0 = plus heads | minus heads << 32, pass 1 = the tails likewise
__global__ __launch_bounds__(256) void heli_flag_kernel(const int64_t *__restrict__ key, const int32_t *__restrict__ score, int64_t n_anchor,
                                                        int pass, int32_t thr, int64_t *__restrict__ val) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= n_anchor) return;
    const int kind = (int)(key[a] & 3);
    int64_t v = 0;
    if ((kind >> 1) == pass && score[a] >= thr) v = (kind & 1) ? ((int64_t)1 << 32) : 1;
    val[a] = v;
}

struct HeliList { int64_t *pos; int32_t *score; int32_t *seq; };      // global byte of the anchor, its score, its sequence

__global__ __launch_bounds__(256) void heli_list_kernel(const int64_t *__restrict__ key, const int32_t *__restrict__ score,
                                                        const int32_t *__restrict__ seq, int64_t n_anchor, int pass, int32_t thr,
                                                        const int64_t *__restrict__ pre, HeliList plus, HeliList minus) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= n_anchor) return;
    const int kind = (int)(key[a] & 3);
    if ((kind >> 1) != pass || score[a] < thr) return;
    const HeliList L = (kind & 1) ? minus : plus;
    const int64_t at = (kind & 1) ? (pre[a] >> 32) : (pre[a] & 0xFFFFFFFFll);
    L.pos[at] = key[a] >> 2; L.score[at] = score[a]; L.seq[at] = seq[a];
}

// first index k of the ascending list v[0..n) with v[k] >= x
__device__ __forceinline__ int64_t heli_lower(const int64_t *__restrict__ v, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// last index k with v[k] <= x, or -1
__device__ __forceinline__ int64_t heli_upper_last(const int64_t *__restrict__ v, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// heads 0 .. n_hp - 1 are the plus heads, n_hp .. n_hp + n_hm - 1 the minus heads.  partner = index into the strand's tail list or -1.
// Plus: head T at byte i, tail ends at byte j: length j - i + 1.  Minus (forward bytes): head GA at i, i + 1, tail begins at j <= i:
// the element is bytes j .. i + 1, length i - j + 2; "downstream" on the minus strand is towards smaller j.
__global__ __launch_bounds__(256) void heli_pair_kernel(HeliList hp, int64_t n_hp, HeliList hm, int64_t n_hm, HeliList tp, int64_t n_tp,
                                                        HeliList tm, int64_t n_tm, const int64_t *__restrict__ off, int32_t len_min,
                                                        int32_t len_max, int64_t *__restrict__ partner, int32_t *__restrict__ found_p,
                                                        int32_t *__restrict__ found_m) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= n_hp + n_hm) return;
    int64_t t = -1;
    if (h < n_hp) {
        const int64_t i = hp.pos[h], e = off[hp.seq[h] + 1];
        const int64_t k = heli_lower(tp.pos, n_tp, i + len_min - 1);
        if (k < n_tp && tp.pos[k] < e && tp.pos[k] <= i + (int64_t)len_max - 1) t = k;
        found_p[h] = t >= 0;
    } else {
        const int64_t m = h - n_hp, i = hm.pos[m], b = off[hm.seq[m]];
        const int64_t k = heli_upper_last(tm.pos, n_tm, i + 2 - len_min);
        if (k >= 0 && tm.pos[k] >= b && tm.pos[k] >= i + 2 - (int64_t)len_max) t = k;
        found_m[m] = t >= 0;
    }
    partner[h] = t;
}

struct HeliOut { int32_t *seq, *start, *end, *hscore, *tscore; uint8_t *strand; };

__global__ __launch_bounds__(256) void heli_place_kernel(HeliList hp, int64_t n_hp, HeliList hm, int64_t n_hm, HeliList tp, HeliList tm,
                                                         const int64_t *__restrict__ off, const int64_t *__restrict__ partner,
                                                         const int64_t *__restrict__ pre_p, const int64_t *__restrict__ pre_m, int64_t cap,
                                                         HeliOut o) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= n_hp + n_hm) return;
    const int64_t t = partner[h];
    if (t < 0) return;
    const bool minus = h >= n_hp;
    const int64_t m = h - n_hp;
    const int32_t q = minus ? hm.seq[m] : hp.seq[h];
    const int64_t b = off[q], e = off[q + 1];
    // records of the sequences before q, then (minus strand) the plus records of q, then the rank inside the strand
    const int64_t p0 = pre_p[heli_lower(hp.pos, n_hp, b)], m0 = pre_m[heli_lower(hm.pos, n_hm, b)];
    int64_t at = p0 + m0;
    if (minus) at += pre_p[heli_lower(hp.pos, n_hp, e)] - p0 + pre_m[m] - m0;
    else at += pre_p[h] - p0;
    if (at >= cap) return;
    o.seq[at] = q;
    o.strand[at] = minus ? 1 : 0;
    if (minus) {
        o.start[at] = (int32_t)(tm.pos[t] - b); o.end[at] = (int32_t)(hm.pos[m] + 2 - b);
        o.hscore[at] = hm.score[m]; o.tscore[at] = tm.score[t];
    } else {
        o.start[at] = (int32_t)(hp.pos[h] - b); o.end[at] = (int32_t)(tp.pos[t] + 1 - b);
        o.hscore[at] = hp.score[h]; o.tscore[at] = tp.score[t];
    }
}

// the scores as four dense rows of nb entries, each in its strand's own coordinates: row 0 plus heads at p, row 1 plus tails at q,
// row 2 minus heads at p', row 3 minus tails at q' (positions of the reverse complement), all at off[seq] + position
__global__ __launch_bounds__(256) void heli_dense_kernel(const int64_t *__restrict__ key, const int32_t *__restrict__ seq,
                                                         const int32_t *__restrict__ score, int64_t n_anchor,
                                                         const int64_t *__restrict__ off, int64_t nb, int32_t *__restrict__ dense) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= n_anchor) return;
    const int kind = (int)(key[a] & 3);
    const int64_t i = key[a] >> 2, b = off[seq[a]], e = off[seq[a] + 1], L = e - b, x = i - b;
    switch (kind) {
        case HELI_HEAD_PLUS: dense[i] = score[a]; break;
        case HELI_TAIL_PLUS: dense[nb + i] = score[a]; break;
        case HELI_HEAD_MINUS: dense[2 * nb + b + (L - 2 - x)] = score[a]; break;
        default: dense[3 * nb + b + (L - 1 - x)] = score[a]; break;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
#define HELI_ALLOC(ptr, bytes) HITE_CHECK(ctx, B.alloc(ptr, (size_t)(bytes)))

struct HeliArgs {
    int64_t n; const int64_t *seq_off; int32_t n_head, n_tail; const hite_lcv *head, *tail;
};
static int heli_check(const HeliArgs &a, std::vector<HeliPat> &hp, std::vector<HeliPat> &tp, std::vector<int64_t> &rel) {
    if (a.n < 0 || a.n >= ((int64_t)1 << 31) || a.n_head < 0 || a.n_tail < 0 || a.n_head > HITE_HELITRON_MAX_PATTERNS ||
        a.n_tail > HITE_HELITRON_MAX_PATTERNS || (a.n > 0 && !a.seq_off) || (a.n_head > 0 && !a.head) || (a.n_tail > 0 && !a.tail))
        return HITE_EINVAL;
    rel.assign((size_t)a.n + 1, 0);
    for (int64_t q = 0; q < a.n; q++) {
        const int64_t l = a.seq_off[q + 1] - a.seq_off[q];
        if (l < 0 || l >= ((int64_t)1 << 31)) return HITE_EINVAL;
        rel[q + 1] = rel[q] + l;
    }
    hp.resize((size_t)a.n_head); tp.resize((size_t)a.n_tail);
    for (int32_t k = 0; k < a.n_head; k++) if (!heli_compile(a.head[k], false, &hp[k])) return HITE_EINVAL;
    for (int32_t k = 0; k < a.n_tail; k++) if (!heli_compile(a.tail[k], true, &tp[k])) return HITE_EINVAL;
    return HITE_OK;
}

struct HeliScored { int64_t *d_off, *d_key; int32_t *d_seq, *d_score; int64_t n_anchor; };

// anchors + scores of the nb bytes at d_s (sequence q = bytes rel[q] .. rel[q + 1]); nb > 0
static int heli_score(hite_ctx *ctx, DevPool &B, const uint8_t *d_s, const std::vector<int64_t> &rel, int64_t n, int64_t nb,
                      const std::vector<HeliPat> &hp, const std::vector<HeliPat> &tp, hipStream_t st, HeliScored *S) {
    int32_t *d_cnt; int64_t *d_pos, *d_bs; HeliPat *d_hp, *d_tp;
    HELI_ALLOC(S->d_off, (n + 1) * 8);
    HELI_ALLOC(d_cnt, nb * 4);
    HELI_ALLOC(d_pos, (nb + 1) * 8);
    HELI_ALLOC(d_bs, scan_tmp_elems(nb) * 8);
    HELI_ALLOC(d_hp, hp.size() * sizeof(HeliPat));
    HELI_ALLOC(d_tp, tp.size() * sizeof(HeliPat));
    HITE_CHECK(ctx, hipMemcpyAsync(S->d_off, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    if (!hp.empty()) HITE_CHECK(ctx, hipMemcpyAsync(d_hp, hp.data(), hp.size() * sizeof(HeliPat), hipMemcpyHostToDevice, st));
    if (!tp.empty()) HITE_CHECK(ctx, hipMemcpyAsync(d_tp, tp.data(), tp.size() * sizeof(HeliPat), hipMemcpyHostToDevice, st));
    int tk = hite_prof_begin(ctx, "heli_anchor_kernels", st);
    hipLaunchKernelGGL(heli_anchor_count_kernel, dim3(grid256(nb)), dim3(256), 0, st, d_s, S->d_off, n, nb, d_cnt);
    HITE_CHECK(ctx, hipGetLastError());
    int rc = scan_excl_buf<int32_t>(ctx, d_bs, d_cnt, nb, d_pos, st);
    if (rc) return rc;
    HITE_CHECK(ctx, hipMemcpyAsync(&S->n_anchor, d_pos + nb, 8, hipMemcpyDeviceToHost, st));
    HITE_CHECK(ctx, hipStreamSynchronize(st));
    const int64_t A = S->n_anchor;
    if (A >= ((int64_t)1 << 31)) { hite_prof_end(ctx, tk, st); return HITE_EINVAL; }      // (the lists count in packed 32-bit halves)
    HELI_ALLOC(S->d_key, A * 8);
    HELI_ALLOC(S->d_seq, A * 4);
    HELI_ALLOC(S->d_score, A * 4);
    if (A == 0) { hite_prof_end(ctx, tk, st); return HITE_OK; }
    hipLaunchKernelGGL(heli_anchor_fill_kernel, dim3(grid256(nb)), dim3(256), 0, st, d_s, S->d_off, n, nb, d_pos, S->d_key, S->d_seq);
    hite_prof_end(ctx, tk, st);
    int64_t blocks = (A + HELI_WAVES - 1) / HELI_WAVES;
    if (blocks > 256 * 8) blocks = 256 * 8;
    tk = hite_prof_begin(ctx, "heli_score_kernel", st);
    hipLaunchKernelGGL(heli_score_kernel, dim3((unsigned)blocks), dim3(HELI_WAVES * 64), 0, st, d_s, S->d_off, S->d_key, S->d_seq, A, d_hp,
                       (int32_t)hp.size(), d_tp, (int32_t)tp.size(), S->d_score);
    hite_prof_end(ctx, tk, st);
    HITE_CHECK(ctx, hipGetLastError());
    return HITE_OK;
}

static int heli_list_alloc(hite_ctx *ctx, DevPool &B, int64_t n, HeliList *L) {
    HELI_ALLOC(L->pos, n * 8);
    HELI_ALLOC(L->score, n * 4);
    HELI_ALLOC(L->seq, n * 4);
    return HITE_OK;
}

extern "C" int hite_helitron_scan_dev(hite_ctx *ctx, int64_t n, const uint8_t *d_seqs, const int64_t *seq_off, int32_t n_head,
                                      const hite_lcv *head, int32_t n_tail, const hite_lcv *tail, int32_t head_threshold,
                                      int32_t tail_threshold, int32_t len_min, int32_t len_max, int64_t cap, int32_t *seq_out,
                                      int32_t *start_out, int32_t *end_out, uint8_t *strand_out, int32_t *hscore_out, int32_t *tscore_out,
                                      int64_t *n_out, int64_t *stats, void *stream) {
    if (!ctx || !n_out || cap < 0 || head_threshold < 1 || tail_threshold < 1 || len_min < 1 || len_min > len_max) return HITE_EINVAL;
    if (cap > 0 && (!seq_out || !start_out || !end_out || !strand_out || !hscore_out || !tscore_out)) return HITE_EINVAL;
    *n_out = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    hipStream_t st = (hipStream_t)stream;
    try {
        std::vector<HeliPat> hpat, tpat;
        std::vector<int64_t> rel;
        const HeliArgs a = {n, seq_off, n_head, n_tail, head, tail};
        int rc = heli_check(a, hpat, tpat, rel);
        if (rc) return rc;
        const int64_t nb = rel[(size_t)n];
        if (nb == 0) return HITE_OK;
        if (!d_seqs) return HITE_EINVAL;
        HITE_CHECK(ctx, hipSetDevice(ctx->device));
        DevPool B;
        HeliScored S;
        if ((rc = heli_score(ctx, B, d_seqs, rel, n, nb, hpat, tpat, st, &S))) return rc;
        const int64_t A = S.n_anchor;
        if (stats) stats[0] = A;
        if (A == 0) { hite_prof_resolve(ctx); return HITE_OK; }

        // the four lists
        int64_t *d_val, *d_pre, *d_bs;
        HELI_ALLOC(d_val, A * 8);
        HELI_ALLOC(d_pre, (A + 1) * 8);
        HELI_ALLOC(d_bs, scan_tmp_elems(A) * 8);
        HeliList L[4];          // plus heads, minus heads, plus tails, minus tails
        int64_t cnt[4];
        int tk = hite_prof_begin(ctx, "heli_list_kernels", st);
        for (int pass = 0; pass < 2; pass++) {
            const int32_t thr = pass ? tail_threshold : head_threshold;
            hipLaunchKernelGGL(heli_flag_kernel, dim3(grid256(A)), dim3(256), 0, st, S.d_key, S.d_score, A, pass, thr, d_val);
            if ((rc = scan_excl_buf<int64_t>(ctx, d_bs, d_val, A, d_pre, st))) return rc;
            int64_t tot = 0;
            HITE_CHECK(ctx, hipMemcpyAsync(&tot, d_pre + A, 8, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipStreamSynchronize(st));
            cnt[2 * pass] = tot & 0xFFFFFFFFll; cnt[2 * pass + 1] = tot >> 32;
            if ((rc = heli_list_alloc(ctx, B, cnt[2 * pass], &L[2 * pass]))) return rc;
            if ((rc = heli_list_alloc(ctx, B, cnt[2 * pass + 1], &L[2 * pass + 1]))) return rc;
            hipLaunchKernelGGL(heli_list_kernel, dim3(grid256(A)), dim3(256), 0, st, S.d_key, S.d_score, S.d_seq, A, pass, thr, d_pre,
                               L[2 * pass], L[2 * pass + 1]);
            HITE_CHECK(ctx, hipGetLastError());
        }
        hite_prof_end(ctx, tk, st);
        const int64_t n_hp = cnt[0], n_hm = cnt[1], n_tp = cnt[2], n_tm = cnt[3], nh = n_hp + n_hm;
        if (stats) { stats[1] = nh; stats[2] = n_tp + n_tm; }
        if (nh == 0 || n_tp + n_tm == 0) { HITE_CHECK(ctx, hipStreamSynchronize(st)); hite_prof_resolve(ctx); return HITE_OK; }

        // pairs
        int64_t *d_partner, *d_pre_p, *d_pre_m, *d_bs2; int32_t *d_fp, *d_fm;
        HELI_ALLOC(d_partner, nh * 8);
        HELI_ALLOC(d_fp, n_hp * 4);
        HELI_ALLOC(d_fm, n_hm * 4);
        HELI_ALLOC(d_pre_p, (n_hp + 1) * 8);
        HELI_ALLOC(d_pre_m, (n_hm + 1) * 8);
        HELI_ALLOC(d_bs2, scan_tmp_elems(nh) * 8);
        tk = hite_prof_begin(ctx, "heli_pair_kernels", st);
        hipLaunchKernelGGL(heli_pair_kernel, dim3(grid256(nh)), dim3(256), 0, st, L[0], n_hp, L[1], n_hm, L[2], n_tp, L[3], n_tm, S.d_off,
                           len_min, len_max, d_partner, d_fp, d_fm);
        HITE_CHECK(ctx, hipGetLastError());
        if ((rc = scan_excl_buf<int32_t>(ctx, d_bs2, d_fp, n_hp, d_pre_p, st))) return rc;
        if ((rc = scan_excl_buf<int32_t>(ctx, d_bs2, d_fm, n_hm, d_pre_m, st))) return rc;
        int64_t np = 0, nm = 0;
        HITE_CHECK(ctx, hipMemcpyAsync(&np, d_pre_p + n_hp, 8, hipMemcpyDeviceToHost, st));
        HITE_CHECK(ctx, hipMemcpyAsync(&nm, d_pre_m + n_hm, 8, hipMemcpyDeviceToHost, st));
        HITE_CHECK(ctx, hipStreamSynchronize(st));
        const int64_t total = np + nm, w = total < cap ? total : cap;
        *n_out = total;
        if (stats) stats[3] = total;
        if (w > 0) {
            HeliOut o;
            HELI_ALLOC(o.seq, w * 4); HELI_ALLOC(o.start, w * 4); HELI_ALLOC(o.end, w * 4);
            HELI_ALLOC(o.hscore, w * 4); HELI_ALLOC(o.tscore, w * 4); HELI_ALLOC(o.strand, w);
            hipLaunchKernelGGL(heli_place_kernel, dim3(grid256(nh)), dim3(256), 0, st, L[0], n_hp, L[1], n_hm, L[2], L[3], S.d_off, d_partner,
                               d_pre_p, d_pre_m, w, o);
            HITE_CHECK(ctx, hipGetLastError());
            HITE_CHECK(ctx, hipMemcpyAsync(seq_out, o.seq, (size_t)w * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipMemcpyAsync(start_out, o.start, (size_t)w * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipMemcpyAsync(end_out, o.end, (size_t)w * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipMemcpyAsync(hscore_out, o.hscore, (size_t)w * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipMemcpyAsync(tscore_out, o.tscore, (size_t)w * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipMemcpyAsync(strand_out, o.strand, (size_t)w, hipMemcpyDeviceToHost, st));
        }
        hite_prof_end(ctx, tk, st);
        HITE_CHECK(ctx, hipStreamSynchronize(st));
        hite_prof_resolve(ctx);
        return total > cap ? HITE_ECAP : HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

// host sequences -> device, then the device form
static int heli_upload(hite_ctx *ctx, DevPool &B, int64_t n, const uint8_t *seqs, const int64_t *seq_off, const uint8_t **d_s) {
    *d_s = nullptr;
    if (n <= 0 || !seq_off) return HITE_OK;
    if (!csr_sorted(seq_off, n)) return HITE_EINVAL;
    const int64_t nb = seq_off[n] - seq_off[0];
    if (nb == 0) return HITE_OK;
    if (!seqs) return HITE_EINVAL;
    HITE_CHECK(ctx, hipSetDevice(ctx->device));
    uint8_t *d;
    HELI_ALLOC(d, nb + 16);
    HITE_CHECK(ctx, hipMemcpy(d, seqs + seq_off[0], (size_t)nb, hipMemcpyHostToDevice));
    *d_s = d;
    return HITE_OK;
}

extern "C" int hite_helitron_scan(hite_ctx *ctx, int64_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t n_head,
                                  const hite_lcv *head, int32_t n_tail, const hite_lcv *tail, int32_t head_threshold,
                                  int32_t tail_threshold, int32_t len_min, int32_t len_max, int64_t cap, int32_t *seq_out,
                                  int32_t *start_out, int32_t *end_out, uint8_t *strand_out, int32_t *hscore_out, int32_t *tscore_out,
                                  int64_t *n_out, int64_t *stats) {
    if (!ctx || n < 0) return HITE_EINVAL;
    DevPool B;
    const uint8_t *d_s;
    const int rc = heli_upload(ctx, B, n, seqs, seq_off, &d_s);
    if (rc) return rc;
    return hite_helitron_scan_dev(ctx, n, d_s, seq_off, n_head, head, n_tail, tail, head_threshold, tail_threshold, len_min, len_max, cap,
                                  seq_out, start_out, end_out, strand_out, hscore_out, tscore_out, n_out, stats, nullptr);
}

extern "C" int hite_helitron_scores(hite_ctx *ctx, int64_t n, const uint8_t *seqs, const int64_t *seq_off, int32_t n_head,
                                    const hite_lcv *head, int32_t n_tail, const hite_lcv *tail, int32_t *scores_out) {
    if (!ctx || n < 0) return HITE_EINVAL;
    try {
        std::vector<HeliPat> hpat, tpat;
        std::vector<int64_t> rel;
        const HeliArgs a = {n, seq_off, n_head, n_tail, head, tail};
        int rc = heli_check(a, hpat, tpat, rel);
        if (rc) return rc;
        const int64_t nb = rel[(size_t)n];
        if (nb == 0) return HITE_OK;
        if (!scores_out) return HITE_EINVAL;
        DevPool B;
        const uint8_t *d_s;
        if ((rc = heli_upload(ctx, B, n, seqs, seq_off, &d_s))) return rc;
        HeliScored S;
        hipStream_t st = nullptr;
        if ((rc = heli_score(ctx, B, d_s, rel, n, nb, hpat, tpat, st, &S))) return rc;
        int32_t *d_dense;
        HELI_ALLOC(d_dense, nb * 16);
        HITE_CHECK(ctx, hipMemsetAsync(d_dense, 0, (size_t)nb * 16, st));
        if (S.n_anchor > 0)
            hipLaunchKernelGGL(heli_dense_kernel, dim3(grid256(S.n_anchor)), dim3(256), 0, st, S.d_key, S.d_seq, S.d_score, S.n_anchor,
                               S.d_off, nb, d_dense);
        HITE_CHECK(ctx, hipGetLastError());
        HITE_CHECK(ctx, hipMemcpy(scores_out, d_dense, (size_t)nb * 16, hipMemcpyDeviceToHost));
        hite_prof_resolve(ctx);
        return HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

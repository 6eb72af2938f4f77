// hite_pairhsp.hip -- the high-scoring local alignments (HSPs) of pairs of sequence intervals: the arithmetic under the one
// `blastn -query .. -subject .. -outfmt 6` process FiLTR starts per candidate line in its steps 1 and 2 (is_recombination,
// get_ltr_from_line, judge_scn_line_by_flank_seq_v2: bin/FiLTR-main/src/Util.py:5923, :11149, :10759).  The tool is not pinned (no
// machine of the project has it): parity is the written definition in include/hite_gpu.h ("local alignments of pairs of intervals"),
// its CPU twin tests/pairhsp_twin.py + tests/pairhsp_twin.c, HIP == twin record for record.
//
// ph_pair_kernel: ONE WORKGROUP PER PAIR (Q, S), four wavefronts, in three steps --
//   1. votes: the 12-base words of Q go into an open-addressing table in the workgroup's own slice of global scratch (word -> count and
//      a chain of positions; integer atomics, the counts do not depend on the order); every position of S looks its word up, passes the
//      frequency cap and adds one to a bin of diagonals in LDS per occurrence;
//   2. windows: wavefront 0 picks up to four bins (a wavefront maximum over packed (votes, lowest bin) keys per pick);
//   3. alignment: WAVEFRONT w TAKES BAND w.  hsp_align (hite_hsp.h: the cell, the recurrence and the strip routine) runs the recurrence
//      of the header inside the band and a rectangle.  The wavefront then runs the rectangle before and the one after its first HSP
//      through the same routine.
// The raw HSPs (at most 12 per pair) leave by ordinary vector stores; the host orders them and applies the containment rule.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include "hite_hsp.h"
#include <algorithm>
#include <new>
#include <vector>

#define PH_WAVES HITE_PAIRHSP_MAX_WINDOWS          // wavefront w aligns band w
static_assert(HITE_PAIRHSP_BAND_BELOW + HITE_PAIRHSP_BAND_ABOVE == HSP_BAND, "the band of a window is the band of hsp_align");
#define PH_MAX_BINS (((2 * HITE_PAIRHSP_MAX_LEN - 2) >> HITE_PAIRHSP_BIN_SHIFT) + 2)
#define PH_BATCH_PAIRS 8192                        // pairs per launch ($HITE_PAIRHSP_BATCH_PAIRS overrides: the tests run several batches)
#define PH_BATCH_BYTES ((int64_t)64 << 20)         // interval bytes per launch
#define PH_MAX_BLOCKS 512
#define PH_TABLE_BYTES ((size_t)256 << 20)         // all word tables of a launch together
#define PH_OUT_WORDS (7 * HITE_PAIRHSP_MAX_HSPS)   // per pair: 4 bands x (first, before, after) x 7; score 0: no HSP there

struct PhTask { int64_t q0, s0; int32_t m, n; };      // byte offsets of the two intervals in the batch's bytes

// the word that begins at position i of the len bytes at p, or -1 (past the end, or a byte outside ACGT)
__device__ __forceinline__ int ph_word(const uint8_t *p, int len, int i) {
    if (i + HITE_PAIRHSP_WORD > len) return -1;
    int w = 0;
#pragma unroll
    for (int k = 0; k < HITE_PAIRHSP_WORD; k++) {
        const int c = hsp_code(p[i + k]);
        if (c > 3) return -1;
        w = w * 4 + c;
    }
    return w;
}
__device__ __forceinline__ uint32_t ph_hash(int w) { return ((uint32_t)w * 2654435761u) >> 8; }

__device__ __forceinline__ void ph_store(int32_t *o, const HspBest &h) {
    const int score = hsp_score(h.a);
    if (score < HITE_PAIRHSP_MIN_SCORE) {
        for (int k = 0; k < 7; k++) o[k] = 0;
        return;
    }
    o[0] = hsp_q_start(h.b); o[1] = hsp_q_end(h.e); o[2] = hsp_s_start(h.b); o[3] = hsp_s_end(h.e);
    o[4] = score; o[5] = hsp_matches(h.a); o[6] = hsp_columns(h.a);
}

// tables: per workgroup table_words 32-bit words -- keys[slots] (word + 1; 0: free), count[slots], head[slots] (position + 1; 0: end),
// next[m] (position + 1 of the next occurrence), slots = the power of two >= max(64, 2 m) of the pair at hand
__global__ __launch_bounds__(PH_WAVES * 64) void ph_pair_kernel(const PhTask *__restrict__ tasks, int n_tasks, const uint8_t *__restrict__ seqs,
                                                                int diag_min, uint32_t *__restrict__ tables, size_t table_words,
                                                                int32_t *__restrict__ out) {
    __shared__ int s_vote[PH_MAX_BINS];
    __shared__ int s_band[PH_WAVES], s_nband;
    __shared__ long long s_bnd_a[PH_WAVES][2 * HSP_BAND];
    __shared__ uint32_t s_bnd_b[PH_WAVES][2 * HSP_BAND];
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    uint32_t *tb = tables + (size_t)blockIdx.x * table_words;
    for (int k = blockIdx.x; k < n_tasks; k += gridDim.x) {
        const PhTask T = tasks[k];
        const int m = T.m, n = T.n;
        const uint8_t *q = seqs + T.q0, *s = seqs + T.s0;
        int slots = 64;
        while (slots < 2 * m) slots <<= 1;
        uint32_t *keys = tb, *cnt = tb + slots, *head = tb + 2 * slots, *next = tb + 3 * slots;
        const int nbins = ((m + n - 2) >> HITE_PAIRHSP_BIN_SHIFT) + 1;      // bins 0 .. nbins - 1 can hold a hit; w(b) reads bin nbins
        for (int x = tid; x < 3 * slots; x += PH_WAVES * 64) tb[x] = 0;
        for (int x = tid; x <= nbins; x += PH_WAVES * 64) s_vote[x] = 0;
        __syncthreads();
        for (int i = tid; i + HITE_PAIRHSP_WORD <= m; i += PH_WAVES * 64) {
            const int wd = ph_word(q, m, i);
            if (wd < 0) continue;
            uint32_t slot = ph_hash(wd) & (uint32_t)(slots - 1);
            bool mine = false;
            for (int t = 0; t < slots && !mine; t++) {      // at most m of the >= 2 m slots are ever taken: a free one comes up
                const uint32_t was = atomicCAS(&keys[slot], 0u, (uint32_t)wd + 1u);
                mine = was == 0u || was == (uint32_t)wd + 1u;
                if (!mine) slot = (slot + 1) & (uint32_t)(slots - 1);
            }
            if (!mine) continue;
            atomicAdd(&cnt[slot], 1u);
            next[i] = atomicExch(&head[slot], (uint32_t)i + 1u);
        }
        __syncthreads();
        for (int j = tid; j + HITE_PAIRHSP_WORD <= n; j += PH_WAVES * 64) {
            const int wd = ph_word(s, n, j);
            if (wd < 0) continue;
            uint32_t slot = ph_hash(wd) & (uint32_t)(slots - 1);
            bool found = false;
            for (int t = 0; t < slots; t++) {
                const uint32_t key = keys[slot];
                if (key == 0u) break;
                if (key == (uint32_t)wd + 1u) { found = true; break; }
                slot = (slot + 1) & (uint32_t)(slots - 1);
            }
            if (!found || cnt[slot] > HITE_PAIRHSP_MAX_OCC) continue;
            uint32_t p = head[slot];
            for (int t = 0; t < HITE_PAIRHSP_MAX_OCC && p != 0u; t++) {      // the chain holds count <= MAX_OCC positions
                const int d = j - (int)(p - 1);
                if (d >= diag_min) atomicAdd(&s_vote[(d + m - 1) >> HITE_PAIRHSP_BIN_SHIFT], 1);
                p = next[p - 1];
            }
        }
        __syncthreads();
        if (w == 0) {       // up to four windows: the largest w(b) >= MIN_VOTES, the lowest b on ties, none next to a chosen one
            int chosen[PH_WAVES], nc = 0;
#pragma unroll
            for (int t = 0; t < PH_WAVES; t++) chosen[t] = -4;
#pragma unroll
            for (int t = 0; t < PH_WAVES; t++) {
                uint32_t key = 0;      // votes * 2^11 + (2047 - b): votes <= 2 * 8 * 32 768 = 2^19
                for (int b = lane; b < nbins; b += 64) {
                    bool near = false;
#pragma unroll
                    for (int c = 0; c < PH_WAVES; c++) near = near || abs(b - chosen[c]) < 2;
                    const int wv = s_vote[b] + s_vote[b + 1];
                    if (!near && wv >= HITE_PAIRHSP_MIN_VOTES) key = max(key, (uint32_t)wv << 11 | (uint32_t)(2047 - b));
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) key = max(key, (uint32_t)__shfl_xor(key, d, 64));
                if (key != 0u && nc == t) {
                    chosen[t] = 2047 - (int)(key & 2047u);
                    nc = t + 1;
                    if (lane == 0) s_band[t] = chosen[t];
                }
            }
            if (lane == 0) s_nband = nc;
        }
        __syncthreads();
        int32_t *o = out + (size_t)k * PH_OUT_WORDS + w * 21;
        HspBest h = {0, 0, 0}, before = {0, 0, 0}, after = {0, 0, 0};
        if (w < s_nband) {
            const int b = s_band[w];
            const int dlo = max((b << HITE_PAIRHSP_BIN_SHIFT) - HITE_PAIRHSP_BAND_BELOW - (m - 1), diag_min);
            const int dhi = (b << HITE_PAIRHSP_BIN_SHIFT) + HITE_PAIRHSP_BAND_ABOVE - 1 - (m - 1);
            h = hsp_align(q, m, s, dlo, dhi, 1, m, 1, n, s_bnd_a[w], s_bnd_b[w]);
            if (hsp_score(h.a) >= HITE_PAIRHSP_MIN_SCORE) {
                const int qs = hsp_q_start(h.b), ss = hsp_s_start(h.b), qe = hsp_q_end(h.e), se = hsp_s_end(h.e);
                if (qs - 1 >= HITE_PAIRHSP_MIN_RECT && ss - 1 >= HITE_PAIRHSP_MIN_RECT)
                    before = hsp_align(q, m, s, dlo, dhi, 1, qs - 1, 1, ss - 1, s_bnd_a[w], s_bnd_b[w]);
                if (m - qe >= HITE_PAIRHSP_MIN_RECT && n - se >= HITE_PAIRHSP_MIN_RECT)
                    after = hsp_align(q, m, s, dlo, dhi, qe + 1, m, se + 1, n, s_bnd_a[w], s_bnd_b[w]);
            }
        }
        if (lane == 0) {
            ph_store(o, h);
            ph_store(o + 7, before);
            ph_store(o + 14, after);
        }
        __syncthreads();          // the next pair overwrites the votes, the bands and the table
    }
}

struct PhHsp { int32_t f[7]; };      // q_start, q_end, s_start, s_end, score, matches, columns

extern "C" int hite_pair_hsps(hite_ctx *ctx, int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int64_t n_pair, const int32_t *a_id,
                              const int64_t *a_start, const int64_t *a_end, const int32_t *b_id, const int64_t *b_start, const int64_t *b_end,
                              int32_t diag_min, int64_t cap, int32_t *status, int64_t *first, int32_t *recs, int64_t *n_out) {
    if (!ctx || n_seq < 0 || n_pair < 0 || cap < 0 || (n_seq > 0 && !seq_off)) return HITE_EINVAL;
    if (n_out) *n_out = 0;
    if (n_pair == 0) {
        if (first) first[0] = 0;
        return HITE_OK;
    }
    if (!a_id || !a_start || !a_end || !b_id || !b_start || !b_end || !status || !first || !n_out || (cap > 0 && !recs)) return HITE_EINVAL;
    if (!csr_sorted(seq_off, n_seq)) return HITE_EINVAL;
    if (n_seq > 0 && seq_off[n_seq] > seq_off[0] && !seqs) return HITE_EINVAL;
    const int64_t batch_pairs = ctx->pairhsp_batch_pairs > 0 ? ctx->pairhsp_batch_pairs : PH_BATCH_PAIRS;
    try {
        // the pairs that pass the limits, in batches of bounded pairs and bytes; the bytes of a pair's two intervals go up side by side
        struct Src { int64_t pair, a0, b0; };
        struct Batch { size_t t0, t1; int64_t bytes; int32_t max_m; };
        std::vector<PhTask> tasks;
        std::vector<Src> src;
        std::vector<Batch> batches;
        for (int64_t p = 0; p < n_pair; p++) {
            status[p] = -1;
            int64_t m, n;
            if (!interval_pair_ok(n_seq, seq_off, a_id[p], a_start[p], a_end[p], b_id[p], b_start[p], b_end[p], 1, HITE_PAIRHSP_MAX_LEN, &m, &n)) continue;
            status[p] = 0;
            if (batches.empty() || (int64_t)(batches.back().t1 - batches.back().t0) >= batch_pairs || batches.back().bytes + m + n > PH_BATCH_BYTES)
                batches.push_back(Batch{tasks.size(), tasks.size(), 0, 0});
            Batch &b = batches.back();
            tasks.push_back(PhTask{b.bytes, b.bytes + m, (int32_t)m, (int32_t)n});
            src.push_back(Src{p, seq_off[a_id[p]] + a_start[p], seq_off[b_id[p]] + b_start[p]});
            b.t1 = tasks.size();
            b.bytes += m + n;
            b.max_m = std::max(b.max_m, (int32_t)m);
        }
        std::vector<std::vector<PhHsp>> found((size_t)n_pair);
        if (!batches.empty()) {
            struct Plan { size_t table_words; unsigned blocks; };
            // the device memory of a batch: the bytes of its pairs, its tasks, its records, the tables of its blocks
            auto layout = [](const Batch &b, const Plan &pl) {
                const size_t nt = b.t1 - b.t0;
                return ScratchPlan({{1, (size_t)b.bytes, 16}, {sizeof(PhTask), nt, 0}, {4, nt * PH_OUT_WORDS, 0}, {4, pl.blocks * pl.table_words, 0}});
            };
            std::vector<Plan> plans;
            size_t need = 0;
            for (const Batch &b : batches) {
                size_t slots = 64;
                while (slots < 2 * (size_t)b.max_m) slots <<= 1;
                Plan pl;
                pl.table_words = 3 * slots + (((size_t)b.max_m + 63) & ~(size_t)63);
                const size_t nt = b.t1 - b.t0;
                pl.blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(nt, PH_MAX_BLOCKS), PH_TABLE_BYTES / (pl.table_words * 4)));
                need = std::max(need, layout(b, pl).total);
                plans.push_back(pl);
            }
            HITE_CHECK(ctx, hipSetDevice(ctx->device));
            void *scr = nullptr;
            const int rc = hite_scratch_reserve(ctx, need + 256, &scr);
            if (rc) return rc;
            hipStream_t st = nullptr;
            std::vector<uint8_t> stage;
            std::vector<int32_t> h_out;
            for (size_t bi = 0; bi < batches.size(); bi++) {
                const Batch &b = batches[bi];
                const Plan &pl = plans[bi];
                const size_t nt = b.t1 - b.t0;
                const ScratchPlan lay = layout(b, pl);
                uint8_t *d_seq = lay.at<uint8_t>(scr, 0);
                PhTask *d_tasks = lay.at<PhTask>(scr, 1);
                int32_t *d_out = lay.at<int32_t>(scr, 2);
                uint32_t *d_tables = lay.at<uint32_t>(scr, 3);
                stage.resize((size_t)b.bytes);
                for (size_t t = b.t0; t < b.t1; t++) {
                    memcpy(stage.data() + tasks[t].q0, seqs + src[t].a0, (size_t)tasks[t].m);
                    memcpy(stage.data() + tasks[t].s0, seqs + src[t].b0, (size_t)tasks[t].n);
                }
                HITE_CHECK(ctx, hipMemcpyAsync(d_seq, stage.data(), (size_t)b.bytes, hipMemcpyHostToDevice, st));
                HITE_CHECK(ctx, hipMemcpyAsync(d_tasks, tasks.data() + b.t0, nt * sizeof(PhTask), hipMemcpyHostToDevice, st));
                const int tk = hite_prof_begin(ctx, "pairhsp_pair", st);
                hipLaunchKernelGGL(ph_pair_kernel, dim3(pl.blocks), dim3(PH_WAVES * 64), 0, st, d_tasks, (int)nt, d_seq, (int)diag_min, d_tables,
                                   pl.table_words, d_out);
                hite_prof_end(ctx, tk, st);
                HITE_CHECK(ctx, hipGetLastError());
                h_out.resize(nt * PH_OUT_WORDS);
                HITE_CHECK(ctx, hipMemcpyAsync(h_out.data(), d_out, nt * PH_OUT_WORDS * 4, hipMemcpyDeviceToHost, st));
                HITE_CHECK(ctx, hipStreamSynchronize(st));      // the next batch overwrites the scratch
                for (size_t t = 0; t < nt; t++) {
                    std::vector<PhHsp> raw, &kept = found[(size_t)src[b.t0 + t].pair];
                    for (int k = 0; k < HITE_PAIRHSP_MAX_HSPS; k++) {
                        PhHsp h;
                        memcpy(h.f, h_out.data() + t * PH_OUT_WORDS + 7 * k, sizeof(h.f));
                        if (h.f[4] >= HITE_PAIRHSP_MIN_SCORE) raw.push_back(h);
                    }
                    // score descending, then q_start, s_start, q_end, s_end; equal keys keep the order they were found in
                    std::stable_sort(raw.begin(), raw.end(), [](const PhHsp &x, const PhHsp &y) {
                        if (x.f[4] != y.f[4]) return x.f[4] > y.f[4];
                        if (x.f[0] != y.f[0]) return x.f[0] < y.f[0];
                        if (x.f[2] != y.f[2]) return x.f[2] < y.f[2];
                        if (x.f[1] != y.f[1]) return x.f[1] < y.f[1];
                        return x.f[3] < y.f[3];
                    });
                    for (const PhHsp &h : raw) {
                        bool inside = false;
                        for (const PhHsp &g : kept) inside = inside || (g.f[0] <= h.f[0] && h.f[1] <= g.f[1] && g.f[2] <= h.f[2] && h.f[3] <= g.f[3]);
                        if (!inside) kept.push_back(h);
                    }
                }
            }
            hite_prof_resolve(ctx);
        }
        int64_t total = 0;
        for (int64_t p = 0; p < n_pair; p++) {
            first[p] = total;
            if (status[p] < 0) continue;
            status[p] = (int32_t)found[(size_t)p].size();
            for (const PhHsp &h : found[(size_t)p]) {
                if (total < cap) memcpy(recs + 7 * total, h.f, sizeof(h.f));
                total++;
            }
        }
        first[n_pair] = total;
        *n_out = total;
        return total > cap ? HITE_ECAP : HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

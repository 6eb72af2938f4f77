// hite_ident.hip -- pairwise identity of sequence intervals: the primitive under the `-c` / `-A` of the build's cd-hit-est stand-in
// (util.remove_redundant_sequences; the reference runs `cd-hit-est -aS 0.95 -aL 0.95 -c <c> -G 0 -g 1 -A 80`, judge_TIR_transposons.py:87,
// Util.py:12330).  The tool is not pinned (no machine of the project has it): parity is the written definition in include/hite_gpu.h
// ("pairwise identity"), its CPU twin tests/identity_twin.py + tests/identity_twin.c, HIP == twin on (cost, matches) for every pair.
//
// ident_pair_kernel: ONE WAVEFRONT PER PAIR.  The band's diagonals d = j - i = lo .. hi are the columns x = d - lo of a row of cell
// states in LDS (one row per wavefront, HITE_IDENT_MAX_WIDTH + 64 words); rows i = 1 .. m go in sequence, a row in strips of 64 columns,
// lane l of strip s owning x = 64 s + l.  In these coordinates the diagonal predecessor (i-1, j-1) is the same x of the row before,
// the cell above (i-1, j) is x + 1 of the row before, and the cell to the left (i, j-1) is x - 1 of the same row: the in-row gap
// chain new[x] = min over x' <= x of (t[x'] + (x - x')) is a wavefront prefix-minimum (six shift-and-add steps), carried from strip to
// strip through lane 63.  A cell state is cost << 16 | (0xFFFF - matches): one unsigned minimum is the lexicographic rule; 0xFFFFFFFF
// is "no such cell" and additions saturate there (an existing cell's cost is at most m + n <= 65 534).
// The host entry point checks every pair (ids, intervals, limits), turns it into a task (byte offsets + lengths) and launches the
// pairs in batches of IDENT_BATCH, so device memory is the sequences plus one batch whatever n_pair is.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include <vector>
#include <new>

#define IDENT_WAVES 4
#define IDENT_MAX_LEN 32767        // STAR_MAX_LEN: the aligner's window limit
#define IDENT_BATCH 65536          // pairs per launch ($HITE_IDENT_BATCH overrides: the tests run several batches of a few hundred)

// >>> ident_cell
#define IDENT_INF 0xFFFFFFFFu      // no such cell
#define IDENT_ONE 0x00010000u      // one edit: cost + 1
#define IDENT_ZERO 0x0000FFFFu     // cost 0, matches 0
// a byte (either case) as a base code A 0 / C 1 / G 2 / T 3 / anything else 4 (N); comp: of the complementary base
__device__ __forceinline__ int ident_code(uint8_t c, bool comp) {
    int b;
    switch (c & 0xDF) {      // letters to upper case
        case 'A': b = 0; break;
        case 'C': b = 1; break;
        case 'G': b = 2; break;
        case 'T': b = 3; break;
        default: return 4;
    }
    return comp ? 3 - b : b;
}
// v + x, staying at "no such cell" on overflow
__device__ __forceinline__ uint32_t ident_add(uint32_t v, uint32_t x) {
    const uint32_t s = v + x;
    return s < v ? IDENT_INF : s;
}
// the cell before its in-row chain: the better of the diagonal step from `diag` = (i-1, j-1) and the step down from `up` = (i-1, j);
// N (code 4) matches nothing.  A match costs nothing and adds one to matches: state - 1.
__device__ __forceinline__ uint32_t ident_cell(uint32_t diag, uint32_t up, int ca, int cb) {
    const uint32_t d = diag == IDENT_INF ? IDENT_INF : ((ca == cb && ca < 4) ? diag - 1u : ident_add(diag, IDENT_ONE));
    const uint32_t u = ident_add(up, IDENT_ONE);
    return d < u ? d : u;
}
// the step right over `dist` columns from the state `left`
__device__ __forceinline__ uint32_t ident_chain(uint32_t t, uint32_t left, int dist) {
    const uint32_t c = ident_add(left, (uint32_t)dist * IDENT_ONE);
    return c < t ? c : t;
}
// <<< ident_cell

struct IdentTask { int64_t a0, b0; int32_t m, n, strand, pad; };   // byte offsets of the two intervals; m < 0: the pair is refused

__global__ __launch_bounds__(IDENT_WAVES * 64) void ident_pair_kernel(const IdentTask *__restrict__ tasks, int64_t n_tasks,
                                                                      const uint8_t *__restrict__ seqs, int32_t band,
                                                                      int32_t *__restrict__ out) {
    __shared__ uint32_t rows[IDENT_WAVES][HITE_IDENT_MAX_WIDTH + 64];
    const int lane = lane_id(), w = wave_id();
    uint32_t *row = rows[w];
    for (int64_t k = (int64_t)blockIdx.x * IDENT_WAVES + w; k < n_tasks; k += (int64_t)gridDim.x * IDENT_WAVES) {
        const IdentTask T = tasks[k];
        const int m = T.m, n = T.n;
        int32_t *o = out + 2 * k;
        if (m < 0) {         // refused by the host: a limit, an id or an interval
            if (lane == 0) { o[0] = -1; o[1] = 0; }
            continue;
        }
        const int lo = min(0, n - m) - band, hi = max(0, n - m) + band;
        const int W = hi - lo + 1;
        const int ns = (W + 63) >> 6;
        const uint8_t *a = seqs + T.a0, *b = seqs + T.b0;
        const bool rev = T.strand != 0;
        // row 0: (0, j) costs j; the columns from W on stay "no such cell" for good (the cell above the last column reads one of them)
        for (int x = lane; x < ns * 64 + 64; x += 64) {
            const int j = lo + x;
            row[x] = (x < W && j >= 0 && j <= n) ? IDENT_ZERO + (uint32_t)j * IDENT_ONE : IDENT_INF;
        }
        __threadfence_block();
        for (int i = 1; i <= m; i++) {
            const int ca = ident_code(a[i - 1], false);
            uint32_t carry = IDENT_INF;
            for (int s = 0; s < ns; s++) {
                const int x = s * 64 + lane, j = i + lo + x;
                const bool exists = x < W && j >= 0 && j <= n;
                const uint32_t diag = row[x], up = row[x + 1];
                uint32_t t = IDENT_INF;
                if (exists) {
                    const int cb = j >= 1 ? ident_code(rev ? b[n - j] : b[j - 1], rev) : 4;
                    t = ident_cell(j >= 1 ? diag : IDENT_INF, up, ca, cb);
                }
                if (lane == 0) t = ident_chain(t, carry, 1);
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t y = __shfl_up(t, d, 64);
                    if (lane >= d) t = ident_chain(t, y, d);
                }
                if (!exists) t = IDENT_INF;
                carry = __shfl(t, 63, 64);
                row[x] = t;
            }
            __threadfence_block();      // the next row reads what other lanes wrote
        }
        if (lane == 0) {
            const uint32_t v = row[n - m - lo];
            o[0] = (int32_t)(v >> 16);
            o[1] = (int32_t)(0xFFFFu - (v & 0xFFFFu));
        }
        __threadfence_block();          // ... and the next pair's row 0 overwrites it
    }
}

static int ident_batch_size() {
    const char *e = getenv("HITE_IDENT_BATCH");
    if (e && *e) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= (1 << 24)) return (int)v;
    }
    return IDENT_BATCH;
}

static int ident_run(hite_ctx *ctx, const uint8_t *seqs, int64_t n_bytes, const std::vector<IdentTask> &tasks, int32_t band,
                     int32_t *cost_out, int32_t *match_out) {
    hipStream_t st = nullptr;
    const int64_t n_pair = (int64_t)tasks.size();
    const int64_t batch = std::min<int64_t>(ident_batch_size(), n_pair);
    const ScratchPlan plan({{1, (size_t)n_bytes, 16}, {sizeof(IdentTask), (size_t)batch, 0}, {8, (size_t)batch, 0}});
    void *p = nullptr;
    int rc = hite_scratch_reserve(ctx, plan.total + 256, &p);
    if (rc) return rc;
    uint8_t *d_seq = plan.at<uint8_t>(p, 0);
    IdentTask *d_tasks = plan.at<IdentTask>(p, 1);
    int32_t *d_out = plan.at<int32_t>(p, 2);
    if (n_bytes > 0) HITE_CHECK(ctx, hipMemcpyAsync(d_seq, seqs, (size_t)n_bytes, hipMemcpyHostToDevice, st));
    std::vector<int32_t> res((size_t)batch * 2);
    for (int64_t at = 0; at < n_pair; at += batch) {
        const int64_t nb = std::min(batch, n_pair - at);
        HITE_CHECK(ctx, hipMemcpyAsync(d_tasks, tasks.data() + at, (size_t)nb * sizeof(IdentTask), hipMemcpyHostToDevice, st));
        int64_t blocks = (nb + IDENT_WAVES - 1) / IDENT_WAVES;
        if (blocks > 256 * 16) blocks = 256 * 16;
        const int tk = hite_prof_begin(ctx, "ident_pair_kernel", st);
        hipLaunchKernelGGL(ident_pair_kernel, dim3((unsigned)blocks), dim3(IDENT_WAVES * 64), 0, st, d_tasks, nb, d_seq, band, d_out);
        hite_prof_end(ctx, tk, st);
        HITE_CHECK(ctx, hipGetLastError());
        HITE_CHECK(ctx, hipMemcpyAsync(res.data(), d_out, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
        HITE_CHECK(ctx, hipStreamSynchronize(st));
        for (int64_t k = 0; k < nb; k++) { cost_out[at + k] = res[2 * k]; match_out[at + k] = res[2 * k + 1]; }
    }
    hite_prof_resolve(ctx);
    return HITE_OK;
}

extern "C" int hite_pair_identity(hite_ctx *ctx, int64_t n_seq, const uint8_t *seqs, const int64_t *seq_off, int64_t n_pair,
                                  const int32_t *a_id, const int64_t *a_start, const int64_t *a_end, const int32_t *b_id,
                                  const int64_t *b_start, const int64_t *b_end, const uint8_t *strand, int32_t band, int32_t *cost_out,
                                  int32_t *match_out) {
    if (!ctx || n_seq < 0 || n_pair < 0 || band < 0 || (n_seq > 0 && !seq_off)) return HITE_EINVAL;
    if (n_pair == 0) return HITE_OK;
    if (!a_id || !a_start || !a_end || !b_id || !b_start || !b_end || !strand || !cost_out || !match_out) return HITE_EINVAL;
    if (!csr_sorted(seq_off, n_seq)) return HITE_EINVAL;
    const int64_t base = n_seq > 0 ? seq_off[0] : 0, n_bytes = n_seq > 0 ? seq_off[n_seq] - seq_off[0] : 0;
    if (n_bytes > 0 && !seqs) return HITE_EINVAL;
    HITE_CHECK(ctx, hipSetDevice(ctx->device));
    try {
        std::vector<IdentTask> tasks((size_t)n_pair);
        for (int64_t p = 0; p < n_pair; p++) {
            IdentTask &t = tasks[p];
            t.a0 = t.b0 = 0; t.m = -1; t.n = 0; t.strand = strand[p] ? 1 : 0; t.pad = 0;
            int64_t m, n;
            if (!interval_pair_ok(n_seq, seq_off, a_id[p], a_start[p], a_end[p], b_id[p], b_start[p], b_end[p], 0, IDENT_MAX_LEN, &m, &n)) continue;
            const int64_t diff = n > m ? n - m : m - n;
            if (diff + 2 * (int64_t)band + 1 > HITE_IDENT_MAX_WIDTH) continue;
            t.a0 = seq_off[a_id[p]] - base + a_start[p];
            t.b0 = seq_off[b_id[p]] - base + b_start[p];
            t.m = (int32_t)m; t.n = (int32_t)n;
        }
        return ident_run(ctx, seqs ? seqs + base : nullptr, n_bytes, tasks, band, cost_out, match_out);
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

// hite_framecluster.hip -- greedy clustering of small groups of short sequences: the arithmetic under the three `cd-hit-est` calls
// FiLTR makes per LTR candidate on the gap-free flank frames of its copies (sort_frame, bin/FiLTR-main/utils/data_util.py:2872-2920,
// and filter_ltr_by_flanking_cluster_sub, bin/FiLTR-main/src/Util.py:10938-10983).  The tool is not pinned (no machine of the
// project has it): parity is the written definition in include/hite_gpu.h ("clusters of a group of frames"), its CPU twin
// tests/framecluster_twin.py + tests/framecluster_twin.c, HIP == twin on every row.
//
// The host orders the kept rows of every group (length descending, then row index), lays consecutive groups side by side into UNITS of
// at most HITE_FRAMECLUSTER_MAX_ROWS rows (a group never spans two units: a unit is one large group or many small ones) and sends the
// units up in batches of bounded bytes.  fc_unit_kernel: ONE WORKGROUP PER UNIT, in three steps --
//   1. the unit's bytes become base codes in LDS;
//   2. every pair (later row i, earlier row j of the same group) of the unit is one task of the workgroup's wavefronts: ONE WAVEFRONT
//      PER PAIR, so the pairs of many small groups fill the wavefronts that one small group would leave idle.  The pair value is the
//      recurrence of the header over packed 64-bit cells: the lanes are 64 columns of the later (shorter) row, lane l on row d - l at
//      step d, so that the cell above is the lane's own last value, the cell to the left the last value of lane l - 1 and the diagonal
//      cell what lane l - 1 handed over one step earlier (two data-parallel moves per step, no LDS).  A row of more than 64 bases goes in strips;
//      the last column of a strip stays in LDS (one value per row of the matrix) and is what lane 0 of the next strip reads.
//      Similar(j, i) sets bit j of row i in an LDS bit matrix (128 x 128 bits);
//   3. the ordered leader pass, one THREAD per group of the unit: a row joins the lowest representative whose bit it has.
// Nothing leaves the workgroup but one cluster index per row (vector stores); there is no global atomic.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include <algorithm>
#include <new>
#include <vector>

#define FC_WAVES 8
#define FC_MAX_ROWS HITE_FRAMECLUSTER_MAX_ROWS
#define FC_MAX_LEN HITE_FRAMECLUSTER_MAX_LEN
#define FC_BATCH_BYTES ((int64_t)64 << 20)     // sequence bytes per upload ($HITE_FRAMECLUSTER_BATCH_BYTES overrides: the tests run several)
#define FC_MAX_BLOCKS (256 * 8)

// >>> framecluster_cell
// A cell value (score, matches, columns, bases of A, bases of B) is ONE signed 64-bit integer, score * 2^37 + matches * 2^28 +
// columns * 2^18 + a * 2^9 + b: the four lower fields are never negative and stay below their radix (matches, a, b <= 256 < 2^9,
// columns <= 512 < 2^10), so the integer order is the lexicographic order and a step is one addition.
#define FC_SCORE_ONE ((int64_t)1 << 37)
#define FC_STEP_MATCH (2 * FC_SCORE_ONE + ((int64_t)1 << 28) + ((int64_t)1 << 18) + ((int64_t)1 << 9) + 1)      // (+2, 1, 1, 1, 1)
#define FC_STEP_MISMATCH (-2 * FC_SCORE_ONE + ((int64_t)1 << 18) + ((int64_t)1 << 9) + 1)                       // (-2, 0, 1, 1, 1)
#define FC_STEP_GAP_A (-3 * FC_SCORE_ONE + ((int64_t)1 << 18) + ((int64_t)1 << 9))                              // (-3, 0, 1, 1, 0)
#define FC_STEP_GAP_B (-3 * FC_SCORE_ONE + ((int64_t)1 << 18) + 1)                                              // (-3, 0, 1, 0, 1)
// a byte (either case) as a base code A 0 / C 1 / G 2 / T 3 / anything else 4 (N); comp: of the complementary base
__device__ __forceinline__ int fc_code(uint8_t c, bool comp) {
    int b;
    switch (c) {
        case 'A': case 'a': b = 0; break;
        case 'C': case 'c': b = 1; break;
        case 'G': case 'g': b = 2; break;
        case 'T': case 't': b = 3; break;
        default: return 4;
    }
    return comp ? 3 - b : b;
}
__device__ __forceinline__ int fc_comp(int code) { return code < 4 ? 3 - code : 4; }
// V(i, j) from diag = V(i-1, j-1), up = V(i-1, j), left = V(i, j-1); N (code 4) matches nothing; a score <= 0 gives E = 0
__device__ __forceinline__ int64_t fc_cell(int64_t diag, int64_t up, int64_t left, int ca, int cb) {
    int64_t v = diag + ((ca == cb && ca < 4) ? FC_STEP_MATCH : FC_STEP_MISMATCH);
    const int64_t u = up + FC_STEP_GAP_A, l = left + FC_STEP_GAP_B;
    if (u > v) v = u;
    if (l > v) v = l;
    return v < FC_SCORE_ONE ? 0 : v;
}
// Similar(A, B) from the pair value r, A (la bases) the earlier row: every compare in binary64, in the order of the header
__device__ __forceinline__ bool fc_similar(int64_t r, int la, int lb, double ident, double cov_short, double cov_long, int min_cov) {
    const int k = (int)((r >> 28) & 511), c = (int)((r >> 18) & 1023), a = (int)((r >> 9) & 511), b = (int)(r & 511);
    if (!(c > 0)) return false;
    if (!((double)k >= ident * (double)c)) return false;
    if (!(a >= min_cov && b >= min_cov)) return false;
    if (!((double)a >= cov_long * (double)la)) return false;
    return (double)b >= cov_short * (double)lb;
}
// <<< framecluster_cell

struct FcUnit { int64_t off; int32_t row0, n_rows, n_pairs, bytes; };      // bytes at off of the batch, rows [row0, row0 + n_rows) of the batch
struct FcRow { uint32_t loc, pre; uint16_t len, first; };                  // bytes at loc of the unit; pairs of the unit before this row's; first row of its group

__device__ __forceinline__ int64_t fc_wave_max(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t y = __shfl_xor((long long)v, d, 64);
        if (y > v) v = y;
    }
    return v;
}

// lane l takes the value of lane l - 1: one wave_shr1 per 32-bit half.  Lane 0 gets 0; the caller puts its own value there.
__device__ __forceinline__ int64_t fc_up1(int64_t v) {
    const uint32_t lo = (uint32_t)wave_shr1((int)(uint32_t)v), hi = (uint32_t)wave_shr1((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)((uint64_t)hi << 32 | lo);
}

// R(A, B) (rev: R(A, revcomp(B))) by one wavefront; a / b: base codes in LDS, m, n >= 1 bases; bnd: m + 1 words of the wavefront.
// The step of a lane depends on the step before it of its neighbour, so what a step costs is its latency: the cell values and the
// base codes of A travel from lane to lane by data-parallel moves (lane 0 takes the next code from a register that holds 64 of
// them), and the word of the strip before is read one step ahead.  All lanes return the same value.
__device__ __forceinline__ int64_t fc_pair(const uint8_t *a, int m, const uint8_t *b, int n, bool rev, long long *bnd) {
    const int lane = lane_id();
    int64_t best = 0;
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int nl = min(64, n - s0);
        const bool more = s0 + 64 < n;
        int cb = 4;
        if (lane < nl) cb = rev ? fc_comp(b[n - 1 - (s0 + lane)]) : b[s0 + lane];
        int64_t cur = 0, diag = 0;       // V(0, j) = V(0, j - 1) = E
        int ca = 4, a64 = 4;             // the lane's base of A; a[64 k + lane] of the current 64 rows
        int64_t ahead = s0 > 0 ? (int64_t)bnd[1] : 0;      // V(d, s0) of the next step: the strip before, or column 0
        const int steps = m + nl - 1;
        for (int d = 1; d <= steps; d++) {
            const int i = d - lane;
            if (((d - 1) & 63) == 0) a64 = d - 1 + lane < m ? a[d - 1 + lane] : 4;
            const int a_new = __builtin_amdgcn_readlane(a64, (d - 1) & 63);        // a[d - 1], or N past the end
            ca = wave_shr1(ca);
            int64_t left = fc_up1(cur);
            if (lane == 0) { ca = a_new; left = ahead; }
            if (s0 > 0) ahead = d + 1 <= m ? (int64_t)bnd[d + 1] : 0;
            const bool on = lane < nl && i >= 1 && i <= m;
            const int64_t v = fc_cell(diag, cur, left, ca, cb);
            diag = left;
            if (on) {
                cur = v;
                if (v > best) best = v;
                if (more && lane == 63) bnd[i] = v;
            }
        }
        __threadfence_block();          // the next strip (and the next pair) reads what lane 63 wrote
    }
    return fc_wave_max(best);
}

__global__ __launch_bounds__(FC_WAVES * 64) void fc_unit_kernel(const FcUnit *__restrict__ units, int n_units, const FcRow *__restrict__ rows,
                                                                const uint8_t *__restrict__ seqs, double ident, double cov_short,
                                                                double cov_long, int min_cov, int both, int32_t *__restrict__ cl_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_code[];      // the unit's base codes
    __shared__ unsigned long long s_bits[FC_MAX_ROWS][2];                 // bit j of row i: Similar(row first + j, row i)
    __shared__ long long s_bnd[FC_WAVES][FC_MAX_LEN + 1];
    __shared__ uint32_t s_loc[FC_MAX_ROWS], s_pre[FC_MAX_ROWS];
    __shared__ uint16_t s_len[FC_MAX_ROWS], s_first[FC_MAX_ROWS];
    __shared__ int32_t s_cl[FC_MAX_ROWS];
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
        const FcUnit U = units[u];
        const int R = U.n_rows;
        if (tid < R) {
            const FcRow r = rows[U.row0 + tid];
            s_loc[tid] = r.loc; s_pre[tid] = r.pre; s_len[tid] = r.len; s_first[tid] = r.first;
            s_bits[tid][0] = 0; s_bits[tid][1] = 0;
        }
        for (int x = tid; x < U.bytes; x += FC_WAVES * 64) s_code[x] = (uint8_t)fc_code(seqs[U.off + x], false);
        __syncthreads();
        for (int p = w; p < U.n_pairs; p += FC_WAVES) {
            int lo = 0, hi = R - 1;          // the last row whose pairs begin at or before p
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((int)s_pre[mid] <= p) lo = mid; else hi = mid - 1;
            }
            const int i = lo, jl = p - (int)s_pre[i], j = (int)s_first[i] + jl;
            const int la = s_len[j], lb = s_len[i];
            int64_t r = 0;
            if (la > 0 && lb > 0) {
                r = fc_pair(s_code + s_loc[j], la, s_code + s_loc[i], lb, false, s_bnd[w]);
                if (both) {
                    const int64_t r2 = fc_pair(s_code + s_loc[j], la, s_code + s_loc[i], lb, true, s_bnd[w]);
                    if (r2 > r) r = r2;
                }
            }
            if (lane == 0 && fc_similar(r, la, lb, ident, cov_short, cov_long, min_cov)) atomicOr(&s_bits[i][jl >> 6], 1ull << (jl & 63));
        }
        __syncthreads();
        if (tid < R && (int)s_first[tid] == tid) {       // the ordered pass over the group that begins at this row
            unsigned long long rep0 = 0, rep1 = 0;
            int n_cl = 0;
            for (int r = tid; r < R && (int)s_first[r] == tid; r++) {
                const int k = r - tid;
                const unsigned long long m0 = s_bits[r][0] & rep0, m1 = s_bits[r][1] & rep1;
                int cl;
                if (m0 | m1) {
                    cl = s_cl[tid + (m0 ? __ffsll(m0) - 1 : 64 + __ffsll(m1) - 1)];
                } else {
                    cl = n_cl++;
                    if (k < 64) rep0 |= 1ull << k; else rep1 |= 1ull << (k - 64);
                }
                s_cl[r] = cl;
            }
        }
        __syncthreads();
        if (tid < R) cl_out[U.row0 + tid] = s_cl[tid];
        __syncthreads();          // the next unit overwrites the tables
    }
}

struct FcGroup { int64_t g, row0; int32_t n; };        // group g: its kept rows are the entries [row0, row0 + n) of `order`

extern "C" int hite_frame_cluster(hite_ctx *ctx, int64_t n_group, const int64_t *row_off, const uint8_t *seqs, const int64_t *seq_off,
                                  double ident, double cov_short, double cov_long, int32_t min_cov, int32_t min_len, int32_t both_strands,
                                  int32_t *cluster_of_row, int32_t *n_cluster) {
    if (!ctx || n_group < 0 || min_cov < 0 || min_len < 0) return HITE_EINVAL;
    if (!(ident >= 0.0 && ident <= 1.0) || !(cov_short >= 0.0 && cov_short <= 1.0) || !(cov_long >= 0.0 && cov_long <= 1.0))
        return HITE_EINVAL;                                                 // (NaN fails both compares)
    if (n_group == 0) return HITE_OK;
    if (!row_off || !n_cluster || !csr_ok(row_off, n_group)) return HITE_EINVAL;
    const int64_t r_lo = row_off[0], r_hi = row_off[n_group];
    if (r_hi > r_lo) {
        if (!seq_off || !cluster_of_row || !csr_ok(seq_off + r_lo, r_hi - r_lo)) return HITE_EINVAL;
        if (seq_off[r_hi] > seq_off[r_lo] && !seqs) return HITE_EINVAL;
    }
    const int64_t limit = ctx->framecluster_batch_bytes > 0 ? ctx->framecluster_batch_bytes : FC_BATCH_BYTES;
    try {
        // the kept rows of every group in cluster order, group after group; a group beyond a limit or without a kept row ends here
        std::vector<int64_t> order;             // source row (absolute index) of every unit row
        std::vector<FcGroup> groups;
        std::vector<FcUnit> units;
        std::vector<FcRow> rows;
        for (int64_t g = 0; g < n_group; g++) {
            const int64_t r0 = row_off[g], r1 = row_off[g + 1];
            bool beyond = r1 - r0 > FC_MAX_ROWS;
            for (int64_t r = r0; r < r1 && !beyond; r++) beyond = seq_off[r + 1] - seq_off[r] > FC_MAX_LEN;
            for (int64_t r = r0; r < r1; r++) cluster_of_row[r] = -1;
            n_cluster[g] = beyond ? -1 : 0;
            if (beyond) continue;
            const size_t at = order.size();
            for (int64_t r = r0; r < r1; r++)
                if (seq_off[r + 1] - seq_off[r] > min_len) order.push_back(r);
            const int n = (int)(order.size() - at);
            if (n == 0) continue;
            std::stable_sort(order.begin() + at, order.end(),
                             [&](int64_t x, int64_t y) { return seq_off[x + 1] - seq_off[x] > seq_off[y + 1] - seq_off[y]; });
            if (units.empty() || units.back().n_rows + n > FC_MAX_ROWS) units.push_back(FcUnit{0, (int32_t)0, 0, 0, 0});
            FcUnit &U = units.back();
            groups.push_back(FcGroup{g, (int64_t)at, n});
            for (int k = 0; k < n; k++) {
                const int64_t r = order[at + k];
                const int len = (int)(seq_off[r + 1] - seq_off[r]);
                rows.push_back(FcRow{(uint32_t)U.bytes, (uint32_t)U.n_pairs, (uint16_t)len, (uint16_t)U.n_rows});
                U.bytes += len;
                U.n_pairs += k;
            }
            U.n_rows += n;
        }
        if (units.empty()) return HITE_OK;
        // units -> batches of at most `limit` sequence bytes (one unit larger than that runs alone)
        struct Batch { size_t u0, u1; int64_t bytes, rows; int32_t max_bytes; };
        std::vector<Batch> batches;
        {
            int32_t row0 = 0;
            for (size_t u = 0; u < units.size(); u++) {
                if (batches.empty() || batches.back().bytes + units[u].bytes > limit) {
                    batches.push_back(Batch{u, u, 0, 0, 0});
                    row0 = 0;
                }
                Batch &b = batches.back();
                units[u].off = b.bytes;
                units[u].row0 = row0;
                row0 += units[u].n_rows;
                b.u1 = u + 1;
                b.bytes += units[u].bytes;
                b.rows += units[u].n_rows;
                b.max_bytes = std::max(b.max_bytes, units[u].bytes);
                if (b.rows > (int64_t)1 << 30) return HITE_EINVAL;
            }
        }
        // the device memory of a batch: the bytes of its rows, its units, its rows, the cluster of every row
        auto layout = [](const Batch &b) {
            return ScratchPlan({{1, (size_t)b.bytes, 16}, {sizeof(FcUnit), b.u1 - b.u0, 0}, {sizeof(FcRow), (size_t)b.rows, 0}, {4, (size_t)b.rows, 0}});
        };
        size_t need = 0;
        for (const Batch &b : batches) need = std::max(need, layout(b).total);
        HITE_CHECK(ctx, hipSetDevice(ctx->device));
        void *scr = nullptr;
        const int rc = hite_scratch_reserve(ctx, need + 256, &scr);
        if (rc) return rc;
        hipStream_t st = nullptr;
        std::vector<uint8_t> stage;
        std::vector<int32_t> h_cl;
        size_t row_at = 0;        // unit rows before the batch
        for (const Batch &b : batches) {
            const ScratchPlan lay = layout(b);
            uint8_t *d_seq = lay.at<uint8_t>(scr, 0);
            FcUnit *d_units = lay.at<FcUnit>(scr, 1);
            FcRow *d_rows = lay.at<FcRow>(scr, 2);
            int32_t *d_cl = lay.at<int32_t>(scr, 3);
            stage.resize((size_t)b.bytes);
            size_t at = 0;
            for (int64_t k = 0; k < b.rows; k++) {
                const int64_t r = order[row_at + k];
                const size_t len = (size_t)(seq_off[r + 1] - seq_off[r]);
                memcpy(stage.data() + at, seqs + seq_off[r], len);
                at += len;
            }
            HITE_CHECK(ctx, hipMemcpyAsync(d_seq, stage.data(), (size_t)b.bytes, hipMemcpyHostToDevice, st));
            HITE_CHECK(ctx, hipMemcpyAsync(d_units, units.data() + b.u0, (b.u1 - b.u0) * sizeof(FcUnit), hipMemcpyHostToDevice, st));
            HITE_CHECK(ctx, hipMemcpyAsync(d_rows, rows.data() + row_at, (size_t)b.rows * sizeof(FcRow), hipMemcpyHostToDevice, st));
            const int tk = hite_prof_begin(ctx, "framecluster_unit", st);
            hipLaunchKernelGGL(fc_unit_kernel, dim3((unsigned)std::min<size_t>(b.u1 - b.u0, FC_MAX_BLOCKS)), dim3(FC_WAVES * 64),
                               ((size_t)b.max_bytes + 15) & ~(size_t)15, st, d_units, (int)(b.u1 - b.u0), d_rows, d_seq, ident, cov_short, cov_long,
                               min_cov, both_strands ? 1 : 0, d_cl);
            hite_prof_end(ctx, tk, st);
            HITE_CHECK(ctx, hipGetLastError());
            h_cl.resize((size_t)b.rows);
            HITE_CHECK(ctx, hipMemcpyAsync(h_cl.data(), d_cl, (size_t)b.rows * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipStreamSynchronize(st));      // the next batch overwrites the scratch
            for (int64_t k = 0; k < b.rows; k++) cluster_of_row[order[row_at + k]] = h_cl[k];
            row_at += (size_t)b.rows;
        }
        for (const FcGroup &G : groups) {
            int32_t top = -1;
            for (int k = 0; k < G.n; k++) top = std::max(top, cluster_of_row[order[G.row0 + k]]);
            n_cluster[G.g] = top + 1;
        }
        hite_prof_resolve(ctx);
        return HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

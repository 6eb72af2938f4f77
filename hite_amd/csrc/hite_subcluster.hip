// hite_subcluster.hip -- sub-clusters of an aligned cluster: the stage between the first and the second alignment of generate_cons_v1
// (Util.py:12467-12476, where the reference runs `Ninja --corr_type m --cluster_cutoff 0.2`).  The tool is not pinned (no machine of
// the project has it): parity is the written definition in include/hite_gpu.h ("sub-clusters of an alignment"), the leader
// clustering that util.ninja_stand_in states, its CPU twin tests/subcluster_twin.py, HIP == twin on every row.
//
// The definition is sequential (a row joins the FIRST leader it matches, else it becomes the next leader); what runs here is its
// exactly equal chunked form.  Rows go in chunks of B = HITE_SUBCLUSTER_CHUNK (<= 64: the rows of a chunk are the lanes of a wavefront):
//   phase A  sub_phase_a_kernel   every (row of the chunk, leader born before the chunk), one wavefront per pair, across the grid:
//                                 the lowest matching leader index of a row by atomicMin.  Old leaders rank before leaders born in
//                                 the chunk, so a match here is final.
//   phase B  sub_phase_b_kernel   the match bits (row i, row j < i) inside the chunk for the rows phase A left open, one wavefront
//                                 per pair, one 64-bit word of bits per row;
//            sub_resolve_kernel   ONE wavefront, lane = row of the chunk: the ordered pass over the open rows -- a row joins the first
//                                 leader born in the chunk before it whose bit it has, else it becomes a leader.
// The phases hand their results on at kernel boundaries only.  An alignment of R <= B rows is phase B alone and takes ONE workgroup
// (sub_small_kernel: bits in LDS, then the ordered pass by its first wavefront), so a batch of small clusters is one launch.
// A pair is decided by integer counts (diff, n) and one binary64 compare; the counts go over 16-byte words (byte-wise compare inside
// 32-bit words, population count) with the bytes before the first and after the last whole word taken one by one.  A wavefront
// leaves a pair once diff > cutoff * C: n <= C, so the pair cannot match any more.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include <vector>
#include <new>

#define SUB_WAVES 4
#define SUB_NONE 0x7FFFFFFF        // phase A: the row matched no old leader
#define SUB_MAX_COLS 65535
#define SUB_BATCH_BYTES ((int64_t)256 << 20)   // alignment bytes per upload ($HITE_SUBCLUSTER_BATCH_BYTES overrides: the tests run several)
#define SUB_MAX_BLOCKS (256 * 8)

// >>> subcluster_pair
#define SUB_GAP4 0x2D2D2D2Du       // '-' in every byte
// 0x80 in every byte of v that is not zero
__device__ __forceinline__ uint32_t sub_nonzero_bytes(uint32_t v) { return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u; }
// four columns: diff += columns where the rows differ, n += columns where either is not a gap
__device__ __forceinline__ void sub_count4(uint32_t x, uint32_t y, int &diff, int &n) {
    diff += __builtin_popcount(sub_nonzero_bytes(x ^ y));
    n += __builtin_popcount(sub_nonzero_bytes(x ^ SUB_GAP4) | sub_nonzero_bytes(y ^ SUB_GAP4));
}
__device__ __forceinline__ void sub_count1(uint8_t x, uint8_t y, int &diff, int &n) {
    diff += x != y;
    n += (x != 45) | (y != 45);
}
// sixteen columns; x is 16-byte aligned, y is not
__device__ __forceinline__ void sub_count16(const uint8_t *x, const uint8_t *y, int &diff, int &n) {
    uint32_t a[4], b[4];
    __builtin_memcpy(a, __builtin_assume_aligned(x, 16), 16);
    __builtin_memcpy(b, y, 16);
    sub_count4(a[0], b[0], diff, n); sub_count4(a[1], b[1], diff, n);
    sub_count4(a[2], b[2], diff, n); sub_count4(a[3], b[3], diff, n);
}
// the C columns of a pair: `head` bytes until x is 16-byte aligned, `nw` whole words, the rest one by one
__device__ __forceinline__ void sub_split(const uint8_t *x, int C, int &head, int &nw) {
    head = (int)((16u - (unsigned)((uintptr_t)x & 15u)) & 15u);
    if (head > C) head = C;
    nw = (C - head) >> 4;
}
// worker `lane` of `lanes`: its share of the bytes outside the whole words
__device__ __forceinline__ void sub_count_ends(const uint8_t *x, const uint8_t *y, int C, int head, int nw, int lane, int lanes,
                                               int &diff, int &n) {
    for (int c = lane; c < head; c += lanes) sub_count1(x[c], y[c], diff, n);
    for (int c = head + 16 * nw + lane; c < C; c += lanes) sub_count1(x[c], y[c], diff, n);
}
// the match test, in binary64 exactly as written
__device__ __forceinline__ bool sub_match(int diff, int n, double cutoff) { return n > 0 && (double)diff <= cutoff * (double)n; }
// <<< subcluster_pair

__device__ __forceinline__ int sub_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// one wavefront decides one pair (all lanes return the same value)
__device__ __forceinline__ bool sub_pair_match(const uint8_t *x, const uint8_t *y, int C, double cutoff) {
    const int lane = lane_id();
    int head, nw, diff = 0, n = 0;
    sub_split(x, C, head, nw);
    sub_count_ends(x, y, C, head, nw, lane, 64, diff, n);
    const double stop = cutoff * (double)C;
    const uint8_t *xw = x + head, *yw = y + head;
    for (int w0 = 0; w0 < nw; w0 += 256) {       // 4 words per lane and round: 4 096 columns
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int w = w0 + u * 64 + lane;
            if (w < nw) sub_count16(xw + (size_t)w * 16, yw + (size_t)w * 16, diff, n);
        }
        if (w0 + 256 < nw && (double)sub_wave_sum(diff) > stop) return false;
    }
    return sub_match(sub_wave_sum(diff), sub_wave_sum(n), cutoff);
}

// The ordered pass over one chunk by ONE wavefront, lane = row of the chunk (nb <= 64 rows).  best: the lane's phase-A result
// (SUB_NONE: open), bits: bit j = the lane's row matches row j < lane of the chunk, L: leaders before the chunk.
// -> the lane's sub-cluster index; *is_new: the lane's row became a leader; returns the leaders after the chunk.
__device__ __forceinline__ int sub_resolve_wave(int best, uint64_t bits, int nb, int L, int *sub_out, bool *is_new) {
    const int lane = lane_id();
    uint64_t born = 0;            // rows of the chunk that became leaders
    int mine = best;
    bool fresh = false;
    for (int i = 0; i < nb; i++) {
        const int b = __shfl(best, i, 64);
        if (b != SUB_NONE) continue;
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)bits, i, 64), hi = (uint32_t)__shfl((int)(uint32_t)(bits >> 32), i, 64);
        const uint64_t m = ((uint64_t)hi << 32 | lo) & born;
        if (m) {
            const int first = __shfl(mine, __ffsll((unsigned long long)m) - 1, 64);
            if (lane == i) mine = first;
        } else {
            if (lane == i) { mine = L; fresh = true; }
            born |= 1ull << i;
            L++;
        }
    }
    *sub_out = mine;
    *is_new = fresh;
    return L;
}

struct SubTask { int64_t off; int64_t row_base; int32_t rows, cols, slot, pad; };   // an alignment of the batch: bytes at off, results at row_base

// an alignment of R <= 64 rows per workgroup
__global__ __launch_bounds__(SUB_WAVES * 64) void sub_small_kernel(const SubTask *__restrict__ tasks, int n_tasks, const uint8_t *__restrict__ mats,
                                                                   double cutoff, int32_t *__restrict__ sub, int32_t *__restrict__ n_sub) {
    __shared__ unsigned long long s_bits[64];
    const int lane = lane_id(), w = wave_id();
    for (int t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const SubTask T = tasks[t];
        const int R = T.rows, C = T.cols;
        const uint8_t *mat = mats + T.off;
        if (threadIdx.x < 64) s_bits[threadIdx.x] = 0;
        __syncthreads();
        for (int p = w; p < R * R; p += SUB_WAVES) {
            const int i = p / R, j = p - i * R;
            if (j >= i) continue;
            if (sub_pair_match(mat + (size_t)i * C, mat + (size_t)j * C, C, cutoff) && lane == 0) atomicOr(&s_bits[i], 1ull << j);
        }
        __syncthreads();
        if (w == 0) {
            int mine;
            bool fresh;
            const int L = sub_resolve_wave(SUB_NONE, (uint64_t)s_bits[lane], R, 0, &mine, &fresh);
            if (lane < R) sub[T.row_base + lane] = mine;
            if (lane == 0) n_sub[T.slot] = L;
        }
        __syncthreads();          // the next alignment clears the bits
    }
}

// ---- the chunked form: state of ONE alignment (n_lead is its slot of n_sub) -------------------------------------------------------
__global__ void sub_init_kernel(int32_t *__restrict__ best, unsigned long long *__restrict__ bits, int32_t *__restrict__ n_lead) {
    if (threadIdx.x < 64) { best[threadIdx.x] = SUB_NONE; bits[threadIdx.x] = 0; }
    if (threadIdx.x == 0) *n_lead = 0;
}

// pairs p = leader * nb + row: the low leaders first, and a pair whose row already has a lower match is left out
__global__ __launch_bounds__(SUB_WAVES * 64) void sub_phase_a_kernel(const uint8_t *__restrict__ mat, int C, int r0, int nb,
                                                                     const int32_t *__restrict__ leaders, const int32_t *__restrict__ n_lead,
                                                                     double cutoff, int32_t *best) {
    const int lane = lane_id();
    const int64_t n_pair = (int64_t)*n_lead * nb;
    for (int64_t p = (int64_t)blockIdx.x * SUB_WAVES + wave_id(); p < n_pair; p += (int64_t)gridDim.x * SUB_WAVES) {
        const int l = (int)(p / nb), i = (int)(p - (int64_t)l * nb);
        if (__atomic_load_n(&best[i], __ATOMIC_RELAXED) < l) continue;      // (uniform over the wavefront: one address)
        if (sub_pair_match(mat + (size_t)(r0 + i) * C, mat + (size_t)leaders[l] * C, C, cutoff) && lane == 0) atomicMin(&best[i], l);
    }
}

__global__ __launch_bounds__(SUB_WAVES * 64) void sub_phase_b_kernel(const uint8_t *__restrict__ mat, int C, int r0, int nb,
                                                                     const int32_t *__restrict__ best, double cutoff,
                                                                     unsigned long long *__restrict__ bits) {
    const int lane = lane_id();
    for (int p = blockIdx.x * SUB_WAVES + wave_id(); p < nb * nb; p += gridDim.x * SUB_WAVES) {
        const int i = p / nb, j = p - i * nb;
        if (j >= i || best[i] != SUB_NONE || best[j] != SUB_NONE) continue;   // a row with an old leader neither leads nor asks
        if (sub_pair_match(mat + (size_t)(r0 + i) * C, mat + (size_t)(r0 + j) * C, C, cutoff) && lane == 0) atomicOr(&bits[i], 1ull << j);
    }
}

// one wavefront; leaves best / bits cleared for the next chunk
__global__ __launch_bounds__(64) void sub_resolve_kernel(int r0, int nb, int32_t *__restrict__ best, unsigned long long *__restrict__ bits,
                                                         int32_t *__restrict__ leaders, int32_t *__restrict__ n_lead, int32_t *__restrict__ sub) {
    const int lane = lane_id();
    const int b = lane < nb ? best[lane] : SUB_NONE;
    const uint64_t m = lane < nb ? (uint64_t)bits[lane] : 0;
    int mine;
    bool fresh;
    const int L = sub_resolve_wave(b, m, nb, *n_lead, &mine, &fresh);
    if (lane < nb) {
        sub[r0 + lane] = mine;
        if (fresh) leaders[mine] = r0 + lane;
    }
    best[lane] = SUB_NONE;
    bits[lane] = 0;
    if (lane == 0) *n_lead = L;
}

struct SubBatch { int a0, a1; int64_t bytes, rows, max_rows; };     // alignments [a0, a1) go up together

// device memory of a batch, carved from the context's scratch: the alignments, the tasks, the sub-cluster of every row, the count of every
// alignment, the leaders of a chunked alignment, and the best pair / the bit rows of a chunk
static ScratchPlan sub_layout(const SubBatch &b) {
    const size_t na = (size_t)(b.a1 - b.a0);
    return ScratchPlan({{1, (size_t)b.bytes, 32}, {sizeof(SubTask), na, 0}, {4, (size_t)b.rows, 4}, {4, na, 0}, {4, (size_t)b.max_rows, 4}, {4, 64, 0}, {8, 64, 0}});
}

extern "C" int hite_msa_subcluster(hite_ctx *ctx, int32_t nmat, const int32_t *rows, const int64_t *cols, const int64_t *mat_off,
                                   const uint8_t *mats, double cutoff, const int64_t *row_off, int32_t *sub_of_row, int32_t *n_sub) {
    if (!ctx || nmat < 0 || !(cutoff >= 0.0 && cutoff <= 1.0)) return HITE_EINVAL;      // (NaN fails both compares)
    if (nmat == 0) return HITE_OK;
    if (!rows || !cols || !mat_off || !row_off || !n_sub) return HITE_EINVAL;
    if (mat_off[0] < 0 || row_off[0] < 0) return HITE_EINVAL;
    for (int a = 0; a < nmat; a++) {
        if (rows[a] < 0 || cols[a] < 0 || cols[a] > SUB_MAX_COLS) return HITE_EINVAL;
        if (mat_off[a + 1] - mat_off[a] < (int64_t)rows[a] * cols[a] || row_off[a + 1] - row_off[a] < rows[a]) return HITE_EINVAL;
        if (rows[a] > 0 && !sub_of_row) return HITE_EINVAL;
        if ((int64_t)rows[a] * cols[a] > 0 && !mats) return HITE_EINVAL;
    }
    const int B = ctx->subcluster_chunk;
    const int64_t limit = ctx->subcluster_batch_bytes > 0 ? ctx->subcluster_batch_bytes : SUB_BATCH_BYTES;
    try {
        // what needs no device: an alignment without rows has no sub-cluster, one without columns has n = 0 on every pair
        std::vector<SubBatch> batches;
        for (int a = 0; a < nmat; a++) {
            const int64_t sz = (int64_t)rows[a] * cols[a];
            if (sz == 0) {
                for (int r = 0; r < rows[a]; r++) sub_of_row[row_off[a] + r] = r;
                n_sub[a] = rows[a];
                continue;
            }
            // a batch spans mat_off[a0] .. the end of its last alignment, gaps between the alignments included
            if (batches.empty() || mat_off[a] + sz - mat_off[batches.back().a0] > limit) batches.push_back(SubBatch{a, a, 0, 0, 0});
            SubBatch &b = batches.back();
            b.a1 = a + 1;
            b.bytes = mat_off[a] + sz - mat_off[b.a0];
            b.rows += rows[a];
            if (rows[a] > B && rows[a] > b.max_rows) b.max_rows = rows[a];
        }
        if (batches.empty()) return HITE_OK;
        size_t need = 0;
        for (const SubBatch &b : batches) need = std::max(need, sub_layout(b).total);
        HITE_CHECK(ctx, hipSetDevice(ctx->device));
        void *scr = nullptr;
        const int rc = hite_scratch_reserve(ctx, need + 256, &scr);
        if (rc) return rc;
        hipStream_t st = nullptr;
        std::vector<SubTask> tasks, small;
        std::vector<int32_t> h_sub, h_nsub;
        for (const SubBatch &b : batches) {
            const ScratchPlan lay = sub_layout(b);
            uint8_t *d_mats = lay.at<uint8_t>(scr, 0);
            SubTask *d_tasks = lay.at<SubTask>(scr, 1);
            int32_t *d_sub = lay.at<int32_t>(scr, 2), *d_nsub = lay.at<int32_t>(scr, 3), *d_leaders = lay.at<int32_t>(scr, 4);
            int32_t *d_best = lay.at<int32_t>(scr, 5);
            unsigned long long *d_bits = lay.at<unsigned long long>(scr, 6);
            tasks.clear(); small.clear();
            int64_t row_base = 0;
            for (int a = b.a0; a < b.a1; a++) {
                if ((int64_t)rows[a] * cols[a] == 0) continue;
                SubTask t{mat_off[a] - mat_off[b.a0], row_base, rows[a], (int32_t)cols[a], (int32_t)tasks.size(), 0};
                tasks.push_back(t);
                if (rows[a] <= B) small.push_back(t);
                row_base += rows[a];
            }
            HITE_CHECK(ctx, hipMemcpyAsync(d_mats, mats + mat_off[b.a0], (size_t)b.bytes, hipMemcpyHostToDevice, st));
            if (!small.empty()) {
                HITE_CHECK(ctx, hipMemcpyAsync(d_tasks, small.data(), small.size() * sizeof(SubTask), hipMemcpyHostToDevice, st));
                const int tk = hite_prof_begin(ctx, "subcluster_small", st);
                hipLaunchKernelGGL(sub_small_kernel, dim3((unsigned)std::min<size_t>(small.size(), 65536)), dim3(SUB_WAVES * 64), 0, st, d_tasks,
                                   (int)small.size(), d_mats, cutoff, d_sub, d_nsub);
                hite_prof_end(ctx, tk, st);
                HITE_CHECK(ctx, hipGetLastError());
            }
            for (const SubTask &t : tasks) {
                if (t.rows <= B) continue;
                const uint8_t *mat = d_mats + t.off;
                int32_t *n_lead = d_nsub + t.slot, *sub = d_sub + t.row_base;
                hipLaunchKernelGGL(sub_init_kernel, dim3(1), dim3(64), 0, st, d_best, d_bits, n_lead);
                const int tk = hite_prof_begin(ctx, "subcluster_chunked", st);
                for (int r0 = 0; r0 < t.rows; r0 += B) {
                    const int nb = std::min(B, t.rows - r0);
                    if (r0 > 0) {       // at most r0 leaders so far
                        const int64_t blocks = std::min<int64_t>(((int64_t)r0 * nb + SUB_WAVES - 1) / SUB_WAVES, SUB_MAX_BLOCKS);
                        hipLaunchKernelGGL(sub_phase_a_kernel, dim3((unsigned)blocks), dim3(SUB_WAVES * 64), 0, st, mat, t.cols, r0, nb, d_leaders,
                                           n_lead, cutoff, d_best);
                    }
                    hipLaunchKernelGGL(sub_phase_b_kernel, dim3((unsigned)((nb * nb + SUB_WAVES - 1) / SUB_WAVES)), dim3(SUB_WAVES * 64), 0, st, mat,
                                       t.cols, r0, nb, d_best, cutoff, d_bits);
                    hipLaunchKernelGGL(sub_resolve_kernel, dim3(1), dim3(64), 0, st, r0, nb, d_best, d_bits, d_leaders, n_lead, sub);
                }
                hite_prof_end(ctx, tk, st);
                HITE_CHECK(ctx, hipGetLastError());
            }
            h_sub.resize((size_t)b.rows);
            h_nsub.resize(tasks.size());
            HITE_CHECK(ctx, hipMemcpyAsync(h_sub.data(), d_sub, (size_t)b.rows * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipMemcpyAsync(h_nsub.data(), d_nsub, tasks.size() * 4, hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipStreamSynchronize(st));      // the next batch overwrites the scratch
            size_t k = 0;
            for (int a = b.a0; a < b.a1; a++) {
                if ((int64_t)rows[a] * cols[a] == 0) continue;
                const SubTask &t = tasks[k];
                memcpy(sub_of_row + row_off[a], h_sub.data() + t.row_base, (size_t)t.rows * 4);
                n_sub[a] = h_nsub[k++];
            }
        }
        hite_prof_resolve(ctx);
        return HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

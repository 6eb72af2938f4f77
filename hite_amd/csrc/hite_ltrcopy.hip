// hite_ltrcopy.hip -- full-length copy support of the confident intact LTR elements: FiLTR's step 4, where the reference runs
// `minimap2 -ax asm20 -N 100 -p 0.2` of every element against the genome, keeps the alignments that cover element and target
// (get_copies_minimap2, bin/FiLTR-main/src/Util.py:6509-6556) and then only those that coincide with a candidate line, without the
// shorter of two that overlap (get_intact_ltr_copies, :11022-11147).  The rules are in hite_ltrcopy.h, written once for the host and the
// device; the definition is in include/hite_gpu.h ("full-length copy support") and its CPU twin is tests/ltrcopy_twin.py.
//
// The copy table stays on the device: hite_ltr_copy_support runs the copy finder (hite_find_copies_dev, aligned intervals, with the
// clip words of hite_copy_clips_dev for what pysam calls query_alignment_length) and hands its arrays to the two kernels below;
// hite_ltr_copy_support_records uploads a table the caller has.  Only the kept copies come down.
//   lc_match_kernel: ONE THREAD PER RECORD -- the coverage rule, then the look-up of the record's own bucket of candidate lines
//     (binary search over the sorted bucket keys, scan of the bucket).  The candidate table is small (one entry per line) and is
//     built by the entry point in host C++: the greedy pass over a bucket is sequential by definition.
//   lc_element_kernel: ONE WAVEFRONT PER ELEMENT -- the matched records of the element (<= 300) in LDS, their stable order by
//     length as a rank per record, the redundancy rule on the sorted records, and the kept ones out with one atomic per wavefront.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include "hite_ltrcopy.h"

#define LC_FLAG_COVER 1
#define LC_FLAG_MATCH 2
#define LC_MAX_BLOCKS (256 * 16)

// the element that holds record r: the last el with copy_first[el] <= r (empty elements share an offset with their successor)
__device__ __forceinline__ int64_t lc_element_of(const int32_t *__restrict__ copy_first, int64_t n_el, int64_t r) {
    int64_t lo = 0, hi = n_el;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)copy_first[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// counters: [0] records that pass the coverage rule, [1] that also coincide with a candidate line, [2] kept copies
__global__ __launch_bounds__(256) void lc_match_kernel(int64_t n_rec, int64_t n_el, const int64_t *__restrict__ el_len,
                                                       const int32_t *__restrict__ copy_first, const int32_t *__restrict__ contig,
                                                       const int64_t *__restrict__ start1, const int64_t *__restrict__ end1,
                                                       const uint32_t *__restrict__ clip, int32_t n_contig, const uint64_t *__restrict__ bkeys,
                                                       const int64_t *__restrict__ bfirst, int64_t nb, const int64_t *__restrict__ fs,
                                                       const int64_t *__restrict__ fe, double cover, double thr, int64_t segment_len,
                                                       uint8_t *__restrict__ flag, uint32_t *__restrict__ contig_first,
                                                       unsigned long long *__restrict__ counters) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool cov = false, hit = false;
    if (r < n_rec) {
        const int64_t el = lc_element_of(copy_first, n_el, r);
        const int32_t c = contig[r];
        const int64_t s = start1[r], e = end1[r];
        cov = c >= 0 && c < n_contig && lc_cover_ok(el_len[el], clip ? clip[r] : 0u, s, e, cover);
        if (cov) {
            atomicMin(&contig_first[c], (uint32_t)r);       // the order in which the reference meets the contigs
            hit = lc_match(bkeys, bfirst, nb, fs, fe, c, s, e, thr, segment_len);
        }
        flag[r] = (uint8_t)((cov ? LC_FLAG_COVER : 0) | (hit ? LC_FLAG_MATCH : 0));
    }
    const unsigned long long m_cov = __ballot(cov), m_hit = __ballot(hit);
    if (lane_id() == 0) {
        if (m_cov) atomicAdd(&counters[0], (unsigned long long)__popcll(m_cov));
        if (m_hit) atomicAdd(&counters[1], (unsigned long long)__popcll(m_hit));
    }
}

// Blocks of ONE wavefront, an element per trip.  o_*: room for every record; el_base / el_cnt: where the copies of the element begin
// in o_* and how many there are (the wavefronts take their room in the order they finish: the entry point puts the elements in order).
__global__ __launch_bounds__(64) void lc_element_kernel(int64_t n_el, const int32_t *__restrict__ copy_first, const int32_t *__restrict__ contig,
                                                        const int64_t *__restrict__ start1, const int64_t *__restrict__ end1,
                                                        const uint8_t *__restrict__ flag, const uint32_t *__restrict__ contig_first,
                                                        int32_t *__restrict__ o_contig, int64_t *__restrict__ o_start1, int64_t *__restrict__ o_end1,
                                                        int64_t *__restrict__ el_base, int32_t *__restrict__ el_cnt,
                                                        unsigned long long *__restrict__ counters) {
    __shared__ long long s_s[LC_MAX_RECORDS], s_e[LC_MAX_RECORDS], t_s[LC_MAX_RECORDS], t_e[LC_MAX_RECORDS];
    __shared__ int32_t s_c[LC_MAX_RECORDS], t_c[LC_MAX_RECORDS];
    __shared__ uint32_t s_cf[LC_MAX_RECORDS];
    __shared__ uint8_t t_keep[LC_MAX_RECORDS + 4];
    const int lane = lane_id();
    for (int64_t el = blockIdx.x; el < n_el; el += gridDim.x) {
        const int64_t r0 = copy_first[el];
        const int n = min((int)(copy_first[el + 1] - r0), LC_MAX_RECORDS);
        // the matched records of the element, in input order
        int m = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool on = k < n && (flag[r0 + k] & LC_FLAG_MATCH);
            const unsigned long long mask = __ballot(on);
            if (on) {
                const int at = m + __popcll(mask & (((unsigned long long)1 << lane) - 1));
                const int32_t c = contig[r0 + k];
                s_s[at] = start1[r0 + k]; s_e[at] = end1[r0 + k]; s_c[at] = c; s_cf[at] = contig_first[c];
            }
            m += __popcll(mask);
        }
        __syncthreads();
        for (int i = lane; i < m; i += 64) {
            const int rk = lc_rank(i, m, s_s, s_e, s_cf);
            t_s[rk] = s_s[i]; t_e[rk] = s_e[i]; t_c[rk] = s_c[i];
        }
        __syncthreads();
        for (int i = lane; i < m; i += 64) t_keep[i] = !lc_redundant(i, m, t_s, t_e, t_c);
        __syncthreads();
        int kept = 0;
        for (int i0 = 0; i0 < m; i0 += 64) kept += __popcll(__ballot(i0 + lane < m && t_keep[i0 + lane]));
        unsigned long long base = 0;
        if (lane == 0 && kept) base = atomicAdd(&counters[2], (unsigned long long)kept);
        base = (unsigned long long)__shfl((long long)base, 0, 64);
        if (lane == 0) { el_base[el] = (int64_t)base; el_cnt[el] = kept; }
        int done = 0;
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < m && t_keep[i];
            const unsigned long long mask = __ballot(on);
            if (on) {
                const int64_t at = (int64_t)base + done + __popcll(mask & (((unsigned long long)1 << lane) - 1));
                o_contig[at] = t_c[i]; o_start1[at] = t_s[i]; o_end1[at] = t_e[i];
            }
            done += __popcll(mask);
        }
        __syncthreads();          // the next element overwrites the tables
    }
}

// the kernels on a table in device memory, the kept copies down into the caller's arrays
static int lc_run(hite_ctx *ctx, hipStream_t st, int64_t n_el, const int64_t *h_el_len, const int32_t *d_copy_first, int64_t n_rec,
                  const int32_t *d_contig, const int64_t *d_start1, const int64_t *d_end1, const uint32_t *d_clip, int32_t n_contig,
                  const LcBuckets &B, double cover, double thr, int64_t segment_len, int64_t cap, int32_t *out_first, int32_t *out_contig,
                  int64_t *out_start1, int64_t *out_end1, int64_t *n_out, int64_t *stats) {
    *n_out = 0;
    if (stats) { stats[0] = n_rec; stats[1] = stats[2] = stats[3] = 0; }
    for (int64_t k = 0; k <= n_el; k++) out_first[k] = 0;
    if (n_el == 0 || n_rec == 0) return HITE_OK;
    const int64_t nb = (int64_t)B.keys.size(), nf = (int64_t)B.fs.size();
    DevBuf b_len, b_keys, b_first, b_fs, b_fe, b_flag, b_cfirst, b_cnt, b_oc, b_os, b_oe, b_base, b_ecnt;
    HITE_CHECK(ctx, b_len.up(h_el_len, (size_t)n_el * 8));
    HITE_CHECK(ctx, b_keys.up(B.keys.data(), (size_t)nb * 8));
    HITE_CHECK(ctx, b_first.up(B.first.data(), (size_t)(nb + 1) * 8));
    HITE_CHECK(ctx, b_fs.up(B.fs.data(), (size_t)nf * 8));
    HITE_CHECK(ctx, b_fe.up(B.fe.data(), (size_t)nf * 8));
    HITE_CHECK(ctx, b_flag.alloc((size_t)n_rec));
    HITE_CHECK(ctx, b_cfirst.alloc((size_t)n_contig * 4));
    HITE_CHECK(ctx, b_cnt.alloc(4 * 8));
    HITE_CHECK(ctx, b_oc.alloc((size_t)n_rec * 4));
    HITE_CHECK(ctx, b_os.alloc((size_t)n_rec * 8));
    HITE_CHECK(ctx, b_oe.alloc((size_t)n_rec * 8));
    HITE_CHECK(ctx, b_base.alloc((size_t)n_el * 8));
    HITE_CHECK(ctx, b_ecnt.alloc((size_t)n_el * 4));
    HITE_CHECK(ctx, hipMemsetAsync(b_cfirst.p, 0xff, (size_t)n_contig * 4, st));
    HITE_CHECK(ctx, hipMemsetAsync(b_cnt.p, 0, 4 * 8, st));
    unsigned long long *d_cnt = b_cnt.as<unsigned long long>();
    int tk = hite_prof_begin(ctx, "ltrcopy_match", st);
    hipLaunchKernelGGL(lc_match_kernel, dim3(grid256(n_rec)), dim3(256), 0, st, n_rec, n_el, b_len.as<int64_t>(), d_copy_first, d_contig, d_start1,
                       d_end1, d_clip, n_contig, b_keys.as<uint64_t>(), b_first.as<int64_t>(), nb, b_fs.as<int64_t>(), b_fe.as<int64_t>(), cover,
                       thr, segment_len, b_flag.as<uint8_t>(), b_cfirst.as<uint32_t>(), d_cnt);
    hite_prof_end(ctx, tk, st);
    HITE_CHECK(ctx, hipGetLastError());
    tk = hite_prof_begin(ctx, "ltrcopy_element", st);
    hipLaunchKernelGGL(lc_element_kernel, dim3((unsigned)std::min<int64_t>(n_el, LC_MAX_BLOCKS)), dim3(64), 0, st, n_el, d_copy_first, d_contig,
                       d_start1, d_end1, b_flag.as<uint8_t>(), b_cfirst.as<uint32_t>(), b_oc.as<int32_t>(), b_os.as<int64_t>(), b_oe.as<int64_t>(),
                       b_base.as<int64_t>(), b_ecnt.as<int32_t>(), d_cnt);
    hite_prof_end(ctx, tk, st);
    HITE_CHECK(ctx, hipGetLastError());
    unsigned long long h_cnt[4];
    HITE_CHECK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    HITE_CHECK(ctx, hipStreamSynchronize(st));
    hite_prof_resolve(ctx);
    const int64_t total = (int64_t)h_cnt[2];
    *n_out = total;
    if (stats) { stats[1] = (int64_t)h_cnt[0]; stats[2] = (int64_t)h_cnt[1]; stats[3] = total; }
    if (total > n_rec) return HITE_EHIP;
    if (total > cap) return HITE_ECAP;
    std::vector<int64_t> h_base((size_t)n_el), h_s((size_t)total), h_e((size_t)total);
    std::vector<int32_t> h_ecnt((size_t)n_el), h_c((size_t)total);
    HITE_CHECK(ctx, hipMemcpyAsync(h_base.data(), b_base.p, (size_t)n_el * 8, hipMemcpyDeviceToHost, st));
    HITE_CHECK(ctx, hipMemcpyAsync(h_ecnt.data(), b_ecnt.p, (size_t)n_el * 4, hipMemcpyDeviceToHost, st));
    if (total > 0) {
        HITE_CHECK(ctx, hipMemcpyAsync(h_c.data(), b_oc.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HITE_CHECK(ctx, hipMemcpyAsync(h_s.data(), b_os.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
        HITE_CHECK(ctx, hipMemcpyAsync(h_e.data(), b_oe.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    }
    HITE_CHECK(ctx, hipStreamSynchronize(st));
    int64_t at = 0;
    for (int64_t el = 0; el < n_el; el++) {
        out_first[el] = (int32_t)at;
        const int64_t b = h_base[(size_t)el];
        const int32_t c = h_ecnt[(size_t)el];
        if (c < 0 || b < 0 || b + c > total || at + c > total) return HITE_EHIP;
        for (int32_t k = 0; k < c; k++, at++) {
            out_contig[at] = h_c[(size_t)(b + k)]; out_start1[at] = h_s[(size_t)(b + k)]; out_end1[at] = h_e[(size_t)(b + k)];
        }
    }
    out_first[n_el] = (int32_t)at;
    return HITE_OK;
}

static bool lc_params_ok(double cover, double thr, int64_t segment_len) {
    return cover >= 0.0 && cover <= 1.0 && thr >= 0.0 && thr <= 1.0 && segment_len > 0;       // (NaN fails the compares)
}

extern "C" int hite_ltr_copy_support_records(hite_ctx *ctx, int64_t n_el, const int64_t *el_len, const int32_t *copy_first, const int32_t *contig,
                                             const int64_t *start1, const int64_t *end1, const uint32_t *clip, int64_t n_std,
                                             const int32_t *std_contig, const int64_t *std_start, const int64_t *std_end, int32_t n_contig,
                                             const int64_t *contig_len, double full_length_coverage, double overlap_threshold,
                                             int64_t segment_len, int64_t cap, int32_t *out_first, int32_t *out_contig, int64_t *out_start1,
                                             int64_t *out_end1, int64_t *n_out, int64_t *stats) {
    if (!ctx || n_el < 0 || n_std < 0 || n_contig < 0 || cap < 0 || !n_out || !out_first) return HITE_EINVAL;
    if (!lc_params_ok(full_length_coverage, overlap_threshold, segment_len)) return HITE_EINVAL;
    if ((n_el > 0 && (!el_len || !copy_first)) || (n_std > 0 && (!std_contig || !std_start || !std_end)) || (n_contig > 0 && !contig_len))
        return HITE_EINVAL;
    if (cap > 0 && (!out_contig || !out_start1 || !out_end1)) return HITE_EINVAL;
    int64_t n_rec = 0;
    if (n_el > 0) {
        if (copy_first[0] != 0) return HITE_EINVAL;
        for (int64_t k = 0; k < n_el; k++) {
            const int64_t n = (int64_t)copy_first[k + 1] - copy_first[k];
            if (n < 0 || n > LC_MAX_RECORDS) return HITE_EINVAL;
        }
        n_rec = copy_first[n_el];
    }
    if (n_rec > 0 && (!contig || !start1 || !end1)) return HITE_EINVAL;
    for (int64_t r = 0; r < n_rec; r++)
        if (contig[r] < 0 || contig[r] >= n_contig) return HITE_EINVAL;
    try {
        LcBuckets B;
        if (!lc_build_buckets(n_std, std_contig, std_start, std_end, n_contig, contig_len, overlap_threshold, segment_len, &B)) return HITE_EINVAL;
        HITE_CHECK(ctx, hipSetDevice(ctx->device));
        DevBuf b_cf, b_ct, b_s, b_e, b_cl;
        if (n_rec > 0) {
            HITE_CHECK(ctx, b_cf.up(copy_first, (size_t)(n_el + 1) * 4));
            HITE_CHECK(ctx, b_ct.up(contig, (size_t)n_rec * 4));
            HITE_CHECK(ctx, b_s.up(start1, (size_t)n_rec * 8));
            HITE_CHECK(ctx, b_e.up(end1, (size_t)n_rec * 8));
            if (clip) HITE_CHECK(ctx, b_cl.up(clip, (size_t)n_rec * 4));
        }
        return lc_run(ctx, nullptr, n_el, el_len, b_cf.as<int32_t>(), n_rec, b_ct.as<int32_t>(), b_s.as<int64_t>(), b_e.as<int64_t>(),
                      clip ? b_cl.as<uint32_t>() : nullptr, n_contig, B, full_length_coverage, overlap_threshold, segment_len, cap, out_first,
                      out_contig, out_start1, out_end1, n_out, stats);
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

// the finder on the elements, its table handed to lc_run where it lies
static int lc_fused(hite_ctx *ctx, void **state_io, int32_t n_el, const uint8_t *el, const int64_t *el_off, const LcBuckets &B, double cover,
                    double thr, int64_t segment_len, int64_t cap, int32_t *out_first, int32_t *out_contig, int64_t *out_start1, int64_t *out_end1,
                    int64_t *n_out, int64_t *stats) {
    if (!*state_io) {
        const int rc = hite_copy_index_build(ctx, state_io, nullptr);
        if (rc) return rc;
    }
    const int64_t bytes = el_off[n_el];
    DevBuf b_el, b_off;
    HITE_CHECK(ctx, b_el.alloc((size_t)bytes + 64));
    HITE_CHECK(ctx, b_off.alloc((size_t)(n_el + 1) * 8));
    if (bytes > 0) HITE_CHECK(ctx, hipMemcpy(b_el.p, el, (size_t)bytes, hipMemcpyHostToDevice));
    HITE_CHECK(ctx, hipMemcpy(b_off.p, el_off, (size_t)(n_el + 1) * 8, hipMemcpyHostToDevice));
    int32_t *d_cf = nullptr, *d_ct = nullptr, *d_an = nullptr;
    int64_t *d_s = nullptr, *d_e = nullptr, n_rec = 0;
    uint8_t *d_mn = nullptr;
    int rc = hite_find_copies_dev(ctx, *state_io, n_el, b_el.as<uint8_t>(), b_off.as<int64_t>(), bytes, &d_cf, &n_rec, &d_ct, &d_s, &d_e, &d_mn, &d_an,
                                  nullptr);
    if (rc) return rc;
    const uint32_t *d_clip = nullptr;
    int64_t n_clip = 0;
    rc = hite_copy_clips_dev(*state_io, &d_clip, &n_clip);
    if (rc) return rc;
    if (n_rec > 0 && (!d_clip || n_clip != n_rec)) return HITE_EHIP;
    HITE_CHECK(ctx, hipDeviceSynchronize());
    std::vector<int64_t> el_len((size_t)n_el);
    for (int32_t k = 0; k < n_el; k++) el_len[(size_t)k] = el_off[k + 1] - el_off[k];
    return lc_run(ctx, nullptr, n_el, el_len.data(), d_cf, n_rec, d_ct, d_s, d_e, d_clip, ctx->n_contigs, B, cover, thr, segment_len, cap, out_first,
                  out_contig, out_start1, out_end1, n_out, stats);
}

extern "C" int hite_ltr_copy_support(hite_ctx *ctx, void **state_io, int32_t n_el, const uint8_t *el, const int64_t *el_off, int64_t n_std,
                                     const int32_t *std_contig, const int64_t *std_start, const int64_t *std_end, double full_length_coverage,
                                     double overlap_threshold, int64_t segment_len, int64_t cap, int32_t *out_first, int32_t *out_contig,
                                     int64_t *out_start1, int64_t *out_end1, int64_t *n_out, int64_t *stats) {
    if (!ctx || !ctx->d_bases || !ctx->h_contig_off || !state_io || n_el < 0 || n_el >= (1 << 19) || n_std < 0 || cap < 0 || !n_out || !out_first)
        return HITE_EINVAL;
    if (!lc_params_ok(full_length_coverage, overlap_threshold, segment_len)) return HITE_EINVAL;
    if (!el_off || !csr_ok(el_off, n_el) || (el_off[n_el] > el_off[0] && !el) || el_off[0] != 0) return HITE_EINVAL;
    if (n_std > 0 && (!std_contig || !std_start || !std_end)) return HITE_EINVAL;
    if (cap > 0 && (!out_contig || !out_start1 || !out_end1)) return HITE_EINVAL;
    if (n_el == 0) {
        *n_out = 0;
        out_first[0] = 0;
        if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
        return HITE_OK;
    }
    try {
        std::vector<int64_t> contig_len((size_t)ctx->n_contigs);
        for (int32_t c = 0; c < ctx->n_contigs; c++) contig_len[(size_t)c] = ctx->h_contig_off[c + 1] - ctx->h_contig_off[c];
        LcBuckets B;
        if (!lc_build_buckets(n_std, std_contig, std_start, std_end, ctx->n_contigs, contig_len.data(), overlap_threshold, segment_len, &B))
            return HITE_EINVAL;
        HITE_CHECK(ctx, hipSetDevice(ctx->device));
        const int32_t mode = ctx->sw[HITE_SW_COPY_INTERVAL];       // the rule reads aligned intervals and their clips, whatever the context is set to
        ctx->sw[HITE_SW_COPY_INTERVAL] = 1;
        int rc;
        try {
            rc = lc_fused(ctx, state_io, n_el, el, el_off, B, full_length_coverage, overlap_threshold, segment_len, cap, out_first, out_contig,
                          out_start1, out_end1, n_out, stats);
        } catch (...) {
            ctx->sw[HITE_SW_COPY_INTERVAL] = mode;
            throw;
        }
        ctx->sw[HITE_SW_COPY_INTERVAL] = mode;
        return rc;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

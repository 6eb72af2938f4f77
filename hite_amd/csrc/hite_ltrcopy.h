// hite_ltrcopy.h -- the rules of FiLTR's step 4 on one copy record and on the records of one element, as plain C++ for the host and
// the device: what turns the copy table of the confident intact LTR elements into their full-length copies (get_copies_minimap2,
// bin/FiLTR-main/src/Util.py:6509-6556, and get_intact_ltr_copies, :11022-11147).  hite_ltrcopy.hip runs them in its kernels,
// tests/test_host_compiled_ltrcopy.py compiles this file for the host and holds it against tests/ltrcopy_twin.py.
// Every compare of the reference that is made in floating point is made here in binary64 with the same operations in the same order:
// one division or one multiplication of two exactly converted integers, then the compare.  A zero denominator (the reference raises
// ZeroDivisionError) answers false.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define __forceinline__ inline
#endif

#define LC_MAX_RECORDS 300      // records of one element: the cap of the copy finder

// map_fragment (Util.py:4837): the segment of chunk bases that takes the interval; start, end >= 0, chunk > 0
__host__ __device__ __forceinline__ int64_t lc_map_fragment(int64_t start, int64_t end, int64_t chunk) {
    const int64_t sc = start / chunk, ec = end / chunk;
    if (sc == ec) return sc;
    int64_t a = ec * chunk - start, b = end - ec * chunk;
    if (a < 0) a = -a;
    if (b < 0) b = -b;
    return a < b ? ec : sc;
}
// the key of a bucket of candidate lines: (contig, segment), ascending
__host__ __device__ __forceinline__ uint64_t lc_bucket_key(int32_t contig, int64_t seg) { return (uint64_t)(uint32_t)contig << 32 | (uint64_t)(uint32_t)seg; }

// get_copies_minimap2: a record of an element of L bases whose ends lost clip = left | right << 16 bases and that lies on
// start1 .. end1 of the genome is a full-length copy when aligned / L >= c and aligned / (end1 - start1 + 1) >= c
__host__ __device__ __forceinline__ bool lc_cover_ok(int64_t L, uint32_t clip, int64_t start1, int64_t end1, double c) {
    const int64_t aligned = L - (int64_t)(clip & 0xffffu) - (int64_t)(clip >> 16), target = end1 - start1 + 1;
    if (L <= 0 || target <= 0) return false;
    return (double)aligned / (double)L >= c && (double)aligned / (double)target >= c;
}
// the two-sided test of get_intact_ltr_copies on a stored fragment (ps, pe) and a fragment (s, e): get_overlap_len (:4200) over
// |pe - ps| and over |e - s|, both >= thr
__host__ __device__ __forceinline__ bool lc_overlap_ok(int64_t ps, int64_t pe, int64_t s, int64_t e, double thr) {
    int64_t ov = (pe < e ? pe : e) - (ps > s ? ps : s);
    if (ov < 0) ov = 0;
    int64_t dp = pe - ps, dc = e - s;
    if (dp < 0) dp = -dp;
    if (dc < 0) dc = -dc;
    if (dp == 0 || dc == 0) return false;
    return (double)ov / (double)dp >= thr && (double)ov / (double)dc >= thr;
}
// the bucket with this key among nb ascending keys, or -1
__host__ __device__ __forceinline__ int64_t lc_bucket_find(const uint64_t *keys, int64_t nb, uint64_t key) {
    int64_t lo = 0, hi = nb;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < nb && keys[lo] == key ? lo : -1;
}
// does the record (contig, start1, end1) coincide with a candidate line?  Its own bucket alone is searched (:11108)
__host__ __device__ __forceinline__ bool lc_match(const uint64_t *keys, const int64_t *first, int64_t nb, const int64_t *fs, const int64_t *fe,
                                                  int32_t contig, int64_t start1, int64_t end1, double thr, int64_t segment_len) {
    if (contig < 0 || start1 < 0 || end1 < 0) return false;
    const int64_t seg = lc_map_fragment(start1, end1, segment_len);
    if (seg >= ((int64_t)1 << 32)) return false;
    const int64_t b = lc_bucket_find(keys, nb, lc_bucket_key(contig, seg));
    if (b < 0) return false;
    for (int64_t k = first[b]; k < first[b + 1]; k++)
        if (lc_overlap_ok(fs[k], fe[k], start1, end1, thr)) return true;
    return false;
}

// The copies of one element that coincide with a candidate line, in the order the reference holds them before it sorts: by the
// first appearance of their contig among ALL full-length records of the call (the reference collects them contig by contig,
// :11039-11049, 11100), then in input order.  cf[k]: that first appearance (a record index) of the contig of copy k.
// rank of copy i in the stable ascending order by end - start (:11127): the copies that are shorter, or as long and before it
template <class I64, class U32>
__host__ __device__ __forceinline__ int lc_rank(int i, int m, const I64 *s, const I64 *e, const U32 *cf) {
    const int64_t len = (int64_t)e[i] - (int64_t)s[i];
    const uint32_t c = cf[i];
    int r = 0;
    for (int j = 0; j < m; j++) {
        const int64_t lj = (int64_t)e[j] - (int64_t)s[j];
        r += lj < len || (lj == len && (cf[j] < c || (cf[j] == c && j < i)));
    }
    return r;
}
// is copy i of the sorted copies redundant (:11129-11143)?  Some later copy of the same contig overlaps it by >= 0.95 of its length
template <class I64, class I32>
__host__ __device__ __forceinline__ bool lc_redundant(int i, int m, const I64 *s, const I64 *e, const I32 *contig) {
    const int64_t si = s[i], ei = e[i];
    const double need = 0.95 * (double)(ei - si + 1);
    for (int j = i + 1; j < m; j++) {
        if (contig[j] != contig[i]) continue;
        const int64_t sj = s[j], ej = e[j];
        const int64_t ov = (ei < ej ? ei : ej) - (si > sj ? si : sj) + 1;
        if ((double)ov >= need) return true;
    }
    return false;
}

// The table of candidate lines (:11023-11034, 11077-11095): line k lies on std_start[k] .. std_end[k] (0-based start, end) of
// std_contig[k].  In input order a line goes into the bucket (contig, map_fragment) unless a line stored there before passes the
// two-sided test with it.  Out: the buckets ascending by key as a CSR over (fs, fe).  A line outside the segments of its contig
// (the reference raises KeyError) is not stored.  false: a line with a contig outside 0 .. n_contig - 1 or a negative coordinate.
struct LcBuckets {
    std::vector<uint64_t> keys;
    std::vector<int64_t> first, fs, fe;
};
static inline bool lc_build_buckets(int64_t n_std, const int32_t *std_contig, const int64_t *std_start, const int64_t *std_end, int32_t n_contig,
                                    const int64_t *contig_len, double thr, int64_t segment_len, LcBuckets *out) {
    struct Frag { uint64_t key; int64_t s, e; };
    std::vector<Frag> fr;
    fr.reserve((size_t)n_std);
    for (int64_t k = 0; k < n_std; k++) {
        const int32_t c = std_contig[k];
        const int64_t s = std_start[k], e = std_end[k];
        if (c < 0 || c >= n_contig || s < 0 || e < 0) return false;
        const int64_t seg = lc_map_fragment(s, e, segment_len);
        const int64_t n_seg = contig_len[c] / segment_len + (contig_len[c] % segment_len != 0);
        if (seg >= n_seg || seg >= ((int64_t)1 << 32)) continue;
        fr.push_back(Frag{lc_bucket_key(c, seg), s, e});
    }
    std::stable_sort(fr.begin(), fr.end(), [](const Frag &a, const Frag &b) { return a.key < b.key; });
    out->keys.clear(); out->first.clear(); out->fs.clear(); out->fe.clear();
    for (size_t a = 0; a < fr.size();) {
        size_t b = a;
        const size_t at = out->fs.size();
        for (; b < fr.size() && fr[b].key == fr[a].key; b++) {
            bool found = false;
            for (size_t p = at; p < out->fs.size() && !found; p++) found = lc_overlap_ok(out->fs[p], out->fe[p], fr[b].s, fr[b].e, thr);
            if (!found) { out->fs.push_back(fr[b].s); out->fe.push_back(fr[b].e); }
        }
        out->keys.push_back(fr[a].key);
        out->first.push_back((int64_t)at);
        a = b;
    }
    out->first.push_back((int64_t)out->fs.size());
    return true;
}

// hite_hostbuf.h -- what the host wrappers share: the owner of a call's temporary device buffers, the layout of a block carved from
// the context's scratch, the pinned scalars of a driver, and the checks of offset tables and of pairs of intervals.
#pragma once
#include "hite_common.h"
#include <initializer_list>
#include <new>
#include <vector>

// A temporary device buffer of one call, freed on every return path.  Kernels read 16 bytes at a time: what goes up is padded.
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 256); }
    hipError_t up(const void *h, size_t n) {
        hipError_t e = alloc(n + 16);
        if (e != hipSuccess) return e;
        return n ? hipMemcpy(p, h, n, hipMemcpyHostToDevice) : hipSuccess;
    }
    template <class T> T *as() const { return (T *)p; }
};

// As many of them as a call turns out to need, freed first to last.
struct DevPool {
    std::vector<DevBuf> bufs;
    template <class T> hipError_t alloc(T *&out, size_t bytes) {
        bufs.emplace_back();
        const hipError_t e = bufs.back().alloc(bytes);
        out = bufs.back().as<T>();
        return e;
    }
};

// The scalars a driver reads back: SCAL_WORDS words on the device (`d`), where scans and kernels leave totals and counters, and
// their pinned mirror (`h`).  The owner gives the words their meaning (CopySlot in hite_copies.hip, the pipeline's numbers).
#define SCAL_WORDS 64
template <typename TIn> static int scan_excl_buf(hite_ctx *, int64_t *, const TIn *, int64_t, int64_t *, hipStream_t);      // (hite_scan.h)
struct ScalPin {
    int64_t *h = nullptr, *d = nullptr;
    hipError_t alloc() {
        const hipError_t e = hipHostMalloc((void **)&h, SCAL_WORDS * sizeof(int64_t));
        return e != hipSuccess ? e : hipMalloc((void **)&d, SCAL_WORDS * sizeof(int64_t));
    }
    void release() { if (h) (void)hipHostFree(h); if (d) (void)hipFree(d); h = d = nullptr; }
    // words [0, count) to the host; synchronises the stream
    int read_back(hite_ctx *ctx, hipStream_t st, int count) {
        HITE_CHECK(ctx, hipMemcpyAsync(h, d, sizeof(int64_t) * count, hipMemcpyDeviceToHost, st));
        HITE_CHECK(ctx, hipStreamSynchronize(st));
        return HITE_OK;
    }
    // exclusive scan of n counters into out[n + 1] (bs: scan_tmp_elems(n) words; a caller includes hite_scan.h); the total goes to word `slot`
    template <class TIn>
    int scan_total(hite_ctx *ctx, hipStream_t st, int64_t *bs, const TIn *in, int64_t n, int64_t *out, int slot) {
        HITE_TRY(scan_excl_buf<TIn>(ctx, bs, in, n, out, st));
        HITE_CHECK(ctx, hipMemcpyAsync(d + slot, out + n, 8, hipMemcpyDeviceToDevice, st));
        return HITE_OK;
    }
};

// >>> host_plan
// The buffers of one block of device memory: listed once as (element size, count, extra bytes), each starts at a multiple of 256
// and owns at least 256 bytes.  The one list gives the size of the block and every pointer into it.
struct BufSpec { size_t elem, count, extra; };
struct ScratchPlan {
    std::vector<size_t> off;
    size_t total = 0;
    ScratchPlan(std::initializer_list<BufSpec> bufs) : ScratchPlan(bufs.begin(), bufs.size()) {}
    ScratchPlan(const BufSpec *bufs, size_t n) {
        for (size_t i = 0; i < n; i++) {
            const size_t bytes = bufs[i].elem * bufs[i].count + bufs[i].extra;
            off.push_back(total);
            total += bytes ? (bytes + 255) & ~(size_t)255 : 256;
        }
    }
    template <class T> T *at(void *base, size_t i) const { return (T *)((uintptr_t)base + off[i]); }
};

// n + 1 offsets of n consecutive pieces: none of negative length ...
static inline bool csr_sorted(const int64_t *off, int64_t n) {
    for (int64_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return true;
}
// ... and the first at or after 0
static inline bool csr_ok(const int64_t *off, int64_t n) { return n == 0 || (off[0] >= 0 && csr_sorted(off, n)); }

// [start, end) of sequence `id` (its bases: seq_off[id] .. seq_off[id + 1]): inside the sequence and of min_len .. max_len bases?
static inline bool interval_ok(int64_t id, int64_t start, int64_t end, int64_t n_seq, const int64_t *seq_off, int64_t min_len,
                               int64_t max_len, int64_t *len) {
    if (id < 0 || id >= n_seq) return false;
    if (start < 0 || end < start || end > seq_off[id + 1] - seq_off[id]) return false;
    *len = end - start;
    return *len >= min_len && *len <= max_len;
}
// both intervals of a pair: their lengths m and n, or false
static inline bool interval_pair_ok(int64_t n_seq, const int64_t *seq_off, int64_t a_id, int64_t a_start, int64_t a_end, int64_t b_id,
                                    int64_t b_start, int64_t b_end, int64_t min_len, int64_t max_len, int64_t *m, int64_t *n) {
    return interval_ok(a_id, a_start, a_end, n_seq, seq_off, min_len, max_len, m) &&
           interval_ok(b_id, b_start, b_end, n_seq, seq_off, min_len, max_len, n);
}
// <<< host_plan

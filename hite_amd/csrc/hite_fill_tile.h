// hite_fill_tile.h -- the tile form of the sparse fill: a wavefront builds FT_T consecutive centre positions of one row in LDS and
// moves them with wide loads and stores (star_fill_tile_kernel, hite_msa.hip).  The ops of a row are monotone, so for a tile
//   * the window bytes it needs are ONE range of the window: from the end of the op before the tile to the end of its last op
//     (or to the row's end behind the last position) -- loaded into an LDS slot in 16-byte chunks;
//   * the output columns are ONE range of the output row: from the first column of the tile's first position to that of the next
//     tile's (the layout words) -- built as an LDS image and stored in 16-byte chunks;
//   * the layout words are those of every row of the candidate: a lane keeps the words of its positions in registers over the rows.
// One dependent level per (row, tile) -- ops, then the window range -- instead of three per cell (hite_fill.h).
#pragma once
#include "hite_fill.h"

// >>> fill_tile_row (tests/test_host_fill_tiles.py compiles this block for the host, behind the fill_sparse_row block of hite_fill.h:
// the phases below, run lane by lane over a tile, must write what fill_sparse_row writes)
#ifndef FT_NP
#define FT_NP 8                         // consecutive positions of a lane: one 2 * FT_NP-byte load brings their ops
#endif
#define FT_T (64 * FT_NP)               // positions of a tile
#define FT_CH (FT_NP / 8)               // 16-byte chunks of a lane in the window slot and in the image
#define FT_LDS (1024 * FT_CH)           // bytes of the window slot, and of the image, of a wavefront
#define FT_SLOT (FT_LDS - 16)           // longest window range / widest image that fits behind any 16-byte misalignment
#ifndef FT_ROWS
#define FT_ROWS 1                       // rows a workgroup takes per trip, one per wavefront: ONE wavefront walks all rows of a tile
#endif

typedef uint32_t FtV16 __attribute__((vector_size(16)));      // a 16-byte chunk: one load, one store

// the ops a lane holds for one row, as loaded (what they mean at and behind position m is decided in ft_op)
struct FtOps {
    uint32_t o2[FT_NP / 2];             // ops of the positions p0 .. p0 + FT_NP - 1, two per word
    uint32_t oprev;                     // the op in front of p0
};
// the op of the lane's position p0 + u as loaded; u need not be a constant (the words are picked with constant indices: an index that
// is a variable would move them out of the registers)
__device__ __forceinline__ unsigned ft_lane_op(const FtOps &L, int u) {
    uint32_t o = L.o2[0] & 0xffffu;
#pragma unroll
    for (int x = 1; x < FT_NP; x++)
        if (u == x) o = (L.o2[x >> 1] >> (16 * (x & 1))) & 0xffffu;
    return o;
}
__device__ __forceinline__ int ft_end(unsigned o) { return (int)(o & 0x7fffu) + ((o >> 15) ? 0 : 1); }
// the op of position p <= m as the fill reads it: behind the last position the row's end, as a gap; the centre faces itself
__device__ __forceinline__ unsigned ft_op(unsigned raw, int p, int m, int nrow, bool centre) {
    if (p >= m) return 0x8000u | (unsigned)nrow;
    return centre ? (unsigned)p : raw;
}
__device__ __forceinline__ unsigned ft_prev(unsigned raw, int p, bool centre) {     // the op in front of position p
    return centre ? (p == 0 ? 0x8000u : (unsigned)(p - 1)) : raw;
}
// phase 1: the loads of a lane for (row, tile); p0 = its first position, first = the row is row 0 of its candidate.  Every address
// stays inside the row's ops and the spare entries around it but for the 2 * FT_NP - 2 bytes behind position m that the wide load
// may take from the ops row below (the candidate's extra row)
__device__ __forceinline__ FtOps ft_ops_load(const uint16_t *__restrict__ rop, int p0, int m, bool centre, bool first) {
    FtOps L;
#pragma unroll
    for (int i = 0; i < FT_NP / 2; i++) L.o2[i] = 0;
    L.oprev = 0;
    if (centre) return L;
    const int pc = p0 < m ? p0 : m;
    uint32_t t[FT_NP / 2];
    __builtin_memcpy(t, rop + pc, 2 * FT_NP);                  // (ops rows are 2-byte aligned: one unaligned wide load)
#pragma unroll
    for (int i = 0; i < FT_NP / 2; i++) L.o2[i] = t[i];
    // (p == 0: the spare entry of the ops row above, row_ins.  Row 0 of a candidate has no row above -- in front of the first
    // candidate's lies the start of the buffer -- and no ops of its own: where its slot is loaded at all, entry 0 stands in)
    L.oprev = rop[first && pc == 0 ? 0 : pc - 1];
    return L;
}
// the window range of (row, tile): [*qa, *qa + *len); false = it does not fit the slot (or is no range of this row at all): the
// (row, tile) goes through ft_cells_direct.  tprev = the op in front of the tile (oprev of the tile's first lane), tlast = the op of
// its last position pl (ft_lane_op(L, (pl - P0) % FT_NP) of lane (pl - P0) / FT_NP): taken from these lanes, not loaded once more --
// a load from an address that all lanes share is waited for where it is issued
__device__ __forceinline__ bool ft_row_plan(unsigned tprev, unsigned tlast, int P0, int pl, int m, int nrow, bool centre, int *qa, int *len) {
    const int a = ft_end(ft_prev(tprev, P0, centre));
    const int end = ft_end(ft_op(tlast, pl, m, nrow, centre));      // (pl == m: the row's end)
    *qa = a; *len = end - a;
    return a >= 0 && end >= a && end <= nrow && end - a <= FT_SLOT;
}
// the output columns of the tile: [*c0, *c0 + *W) of every row, from the layout words of its first position and of the position
// behind it (wnext; C = the row's columns where the tile is the candidate's last); false = wider than the image
__device__ __forceinline__ bool ft_tile_plan(unsigned wfirst, unsigned wnext, bool last_tile, int C, int *c0, int *W) {
    *c0 = (int)(wfirst >> 16);
    *W = (last_tile ? C : (int)(wnext >> 16)) - *c0;
    return *W >= 0 && *W <= FT_SLOT;
}
// phase 2: the window range into the slot, chunk by chunk: the chunks are those of the ADDRESS (16-byte aligned whatever the
// window's own start), so byte q of the row lies at slot[sh + q - qa], sh = address of byte qa mod 16
__device__ __forceinline__ int ft_win_shift(const uint8_t *b, int qa) { return (int)((uintptr_t)(b + qa) & 15u); }
__device__ __forceinline__ int ft_win_chunks(int sh, int len) { return (sh + len + 15) >> 4; }
// (every lane loads, a lane without a chunk of its own the first one once more: a load that only some lanes -- or only some rows --
// issue makes the waits of everything behind it count as if it had not been issued)
__device__ __forceinline__ void ft_win_load(FtV16 *v, const uint8_t *__restrict__ b, int qa, int len, int lane) {
    const int sh = ft_win_shift(b, qa);
    const FtV16 *src = (const FtV16 *)(b + qa - sh);
    const int nch = ft_win_chunks(sh, len);
#pragma unroll
    for (int k = 0; k < FT_CH; k++) v[k] = src[lane + 64 * k < nch ? lane + 64 * k : 0];
}
template <class Lds>
__device__ __forceinline__ void ft_win_put(Lds slot, const FtV16 *v, int nch, int lane) {
#pragma unroll
    for (int k = 0; k < FT_CH; k++)
        if (lane + 64 * k < nch) ((FtV16 *)slot)[lane + 64 * k] = v[k];
}
// phase 3: the cells of a lane from the slot into the image; w = the layout words of its positions (0 behind m), bias = where
// output column 0 would lie in the image (image offset of column c0 minus c0), wb = sh - qa likewise for the slot
template <class Lds>
__device__ __forceinline__ void ft_cells(Lds img, Lds slot, const FtOps &L, const uint32_t *w, int p0, int m, int nrow, int le, bool centre,
                                         int wb, int bias) {
    unsigned rare = 0;
#pragma unroll
    for (int u = 0; u < FT_NP; u++) {
        const int p = p0 + u;
        const unsigned o = ft_op((L.o2[u >> 1] >> (16 * (u & 1))) & 0xffffu, p, m, nrow, centre);
        const unsigned kw = w[u] & 0x7fffu;
        const bool keep = (w[u] >> 15) & 1u, base = keep && !(o >> 15);
        const uint8_t cb = slot[base ? wb + (int)(o & 0x7fffu) : 0];
        if (keep) img[bias + (int)(w[u] >> 16) + (int)kw] = base ? cb : (uint8_t)'-';
        if (p <= m && (kw != 0u || (p == m && le >= 0))) rare |= 1u << u;
    }
    // kept insertion columns and the extra last column (fill_sparse_block): rare, one trip per such position of the lane.  Its
    // words are picked with constant indices: an index that is a variable would move w and the ops out of the registers
    while (rare) {
        const int u = __builtin_ctz(rare);
        rare &= rare - 1;
        uint32_t wu = w[0], ou = L.o2[0] & 0xffffu, pu = L.oprev;
#pragma unroll
        for (int x = 1; x < FT_NP; x++)
            if (u == x) { wu = w[x]; ou = (L.o2[x >> 1] >> (16 * (x & 1))) & 0xffffu; pu = (L.o2[(x - 1) >> 1] >> (16 * ((x - 1) & 1))) & 0xffffu; }
        const int p = p0 + u;
        const unsigned o = ft_op(ou, p, m, nrow, centre), op = ft_prev(pu, p, centre);
        const int kw = (int)(wu & 0x7fffu), bs = bias + (int)(wu >> 16);
        const int rp = ft_end(op), ins = (int)(o & 0x7fffu) - rp;
        for (int k = 0; k < kw; k++) img[bs + k] = k < ins ? slot[wb + rp + k] : (uint8_t)'-';
        if (p == m && le >= 0) img[bs + kw] = le < ins ? slot[wb + rp + le] : (uint8_t)'-';
    }
}
// phase 4: the image to the output row.  The image begins at the offset the destination has within 16 bytes, so the chunks of
// both are aligned: a head of single bytes up to the first 16-byte boundary, 16-byte stores, a tail of single bytes
__device__ __forceinline__ int ft_img_shift(const uint8_t *dst) { return (int)((uintptr_t)dst & 15u); }
template <class Lds>
__device__ __forceinline__ void ft_store(uint8_t *__restrict__ dst, Lds img, int W, int lane) {
    const int a = ft_img_shift(dst);
    const int head = min(W, (16 - a) & 15), nmid = (W - head) >> 4, tail = W - head - 16 * nmid;
    if (lane < head) dst[lane] = img[a + lane];
    FtV16 *d16 = (FtV16 *)(dst + head);
#pragma unroll
    for (int k = 0; k < FT_CH; k++)
        if (lane + 64 * k < nmid) d16[lane + 64 * k] = ((const FtV16 *)(img + a + head))[lane + 64 * k];
    if (lane < tail) dst[head + 16 * nmid + lane] = img[a + head + 16 * nmid + lane];
}
// a (row, tile) that does not fit: the positions pa .. pb - 1 of the row cell by cell, as fill_sparse_row does them
__device__ __forceinline__ void ft_cells_direct(uint8_t *row, const uint8_t *__restrict__ b, int nrow, const uint16_t *__restrict__ rop,
                                                const uint32_t *__restrict__ lay, int m, int le, bool centre, int pa, int pb, int lane) {
    for (int p = pa + lane; p < pb; p += 64) {
        const unsigned w = lay[p];
        const unsigned oc = centre ? (unsigned)p : (p < m ? (unsigned)rop[p] : 0x8000u);
        if ((w >> 15) & 1u) row[(w >> 16) + (w & 0x7fffu)] = (oc >> 15) ? (uint8_t)'-' : b[oc & 0x7fffu];
        fill_sparse_block<uint8_t *>(row, b, nrow, rop, m, le, centre, p, w, oc);
    }
}
// <<< fill_tile_row

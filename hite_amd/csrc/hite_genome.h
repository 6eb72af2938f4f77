// hite_genome.h -- device helpers over the resident 2-bit genome (shared by hite_ctx.hip and
// hite_pipeline.hip).
#pragma once
#include "hite_common.h"

// window length rules  Util.py:8102-8109, 8117
__device__ __forceinline__ void window_rule(const int64_t *__restrict__ coff, int32_t ncontig, int32_t c, int64_t s1,
                                            int64_t e1, int32_t flank, int64_t &len, int64_t &tlen, int64_t &g_lo) {
    len = 0; tlen = 0; g_lo = 0;
    if (c < 0 || c >= ncontig) return;
    int64_t clen = coff[c + 1] - coff[c];
    if (s1 - 1 - flank < 0 || e1 + flank > clen) return;
    int64_t lo = s1 - 1 - flank, hi = e1 + flank;
    if (hi < lo) hi = lo;
    int64_t n = hi - lo;
    if (n < 100) return;
    len = n;
    tlen = n > 1000 ? 1000 : 0;
    g_lo = coff[c] + lo;
}

// >>> genome_decode (tests/test_host_compiled.py compiles this block for the host and compares it with plain slicing)
// 4 consecutive bases starting at packed index g -> 4 ASCII bytes (little endian in a u32)
__device__ __forceinline__ uint32_t fetch4(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask,
                                           int64_t g) {
    int64_t w = g >> 4;
    int sh = (int)(g & 15) * 2;
    uint64_t two = (uint64_t)bases[w] | ((uint64_t)bases[w + 1] << 32);
    uint32_t bits = (uint32_t)(two >> sh) & 0xffu;
    int64_t mw = g >> 5;
    int msh = (int)(g & 31);
    uint64_t mtwo = (uint64_t)nmask[mw] | ((uint64_t)nmask[mw + 1] << 32);
    uint32_t m = (uint32_t)(mtwo >> msh) & 0xfu;
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t code = (bits >> (2 * i)) & 3u;
        uint32_t ch = (0x54474341u >> (8 * code)) & 0xffu;  // "ACGT"
        if ((m >> i) & 1u) ch = 'N';
        out |= ch << (8 * i);
    }
    return out;
}
// reverse-complement of 4 ASCII bytes packed in a u32 (byte order reversed, bases complemented)
__device__ __forceinline__ uint32_t revcomp4(uint32_t x) {
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t c = (x >> (8 * i)) & 0xffu;
        uint32_t r = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'N';
        out |= r << (8 * (3 - i));
    }
    return out;
}

// 16 consecutive bases starting at packed index g: their 2-bit codes (base i in bits 2i, 2i + 1) and their "not ACGT" bits
__device__ __forceinline__ void fetch16_codes(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask, int64_t g,
                                              uint32_t &codes, uint32_t &nbits) {
    const int64_t w = g >> 4;
    const uint64_t two = (uint64_t)bases[w] | ((uint64_t)bases[w + 1] << 32);
    codes = (uint32_t)(two >> ((int)(g & 15) * 2));
    const int64_t mw = g >> 5;
    const uint64_t mtwo = (uint64_t)nmask[mw] | ((uint64_t)nmask[mw + 1] << 32);
    nbits = (uint32_t)(mtwo >> (int)(g & 31)) & 0xffffu;
}
// the same 16 bases read backwards and complemented
__device__ __forceinline__ void revcomp16_codes(uint32_t &codes, uint32_t &nbits) {
    const uint32_t r = __builtin_bitreverse32(~codes);                       // groups reversed, the two bits of a group swapped
    codes = ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
    nbits = __builtin_bitreverse32(nbits) >> 16;
}
// four of them (8 code bits, 4 "not ACGT" bits) as ASCII
__device__ __forceinline__ uint32_t ascii4(uint32_t c8, uint32_t n4) {
    const uint32_t sel = (c8 | (c8 << 6) | (c8 << 12) | (c8 << 18)) & 0x03030303u;
    uint32_t v = __builtin_amdgcn_perm(0u, 0x54474341u, sel);               // "ACGT"[code] per byte
    if (n4) {
        const uint32_t full = (((n4 | (n4 << 7) | (n4 << 14) | (n4 << 21)) & 0x01010101u)) * 0xffu;
        v = (v & ~full) | (0x4e4e4e4eu & full);
    }
    return v;
}

// write window[ws .. ws+cnt) to dst using the lanes of one wave, four bases per lane and turn (any alignment of dst)
__device__ __forceinline__ void emit_span4(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask,
                                           int64_t g_lo, int64_t wlen, bool minus, int64_t ws, int64_t cnt,
                                           uint8_t *__restrict__ dst, int lane) {
    int64_t groups = (cnt + 3) >> 2;
    bool aligned = (((uintptr_t)dst) & 3) == 0;
    for (int64_t j = lane; j < groups; j += 64) {
        int64_t p = ws + 4 * j;  // window position of the first byte of this group
        int rem = (int)((cnt - 4 * j) < 4 ? (cnt - 4 * j) : 4);
        uint32_t v;
        if (!minus) {
            v = fetch4(bases, nmask, g_lo + p);
        } else {
            // window[p+i] = comp(genome[g_lo + wlen-1-p-i]); fetch ascending from g_lo + wlen - 4 - p
            int64_t g = g_lo + wlen - 4 - p;
            if (g >= 0) v = revcomp4(fetch4(bases, nmask, g));
            else {  // only possible in a partial tail group at the very start of the genome
                v = 0;
                for (int i = 0; i < rem; i++) {
                    uint32_t c = fetch4(bases, nmask, g_lo + wlen - 1 - p - i) & 0xffu;
                    uint32_t r = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'N';
                    v |= r << (8 * i);
                }
            }
        }
        if (rem == 4 && aligned) *reinterpret_cast<uint32_t *>(dst + 4 * j) = v;
        else for (int i = 0; i < rem; i++) dst[4 * j + i] = (uint8_t)(v >> (8 * i));
    }
}
// the same, 16 bases per lane and turn wherever dst allows 16-byte stores (a window is 1-30 kB: with 4-byte stores a wavefront
// wrote 256 B per turn and spent ~40 instructions and 4 loads on every 4 bases); head and tail of the span go four at a time
__device__ __forceinline__ void emit_span(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask,
                                          int64_t g_lo, int64_t wlen, bool minus, int64_t ws, int64_t cnt,
                                          uint8_t *__restrict__ dst, int lane) {
    const int lead = (int)((0 - (uintptr_t)dst) & 15);
    if ((((uintptr_t)dst) & 3) != 0 || cnt < lead + 16) { emit_span4(bases, nmask, g_lo, wlen, minus, ws, cnt, dst, lane); return; }
    if (lead) emit_span4(bases, nmask, g_lo, wlen, minus, ws, lead, dst, lane);
    const int64_t n16 = (cnt - lead) >> 4;
    uint8_t *d16 = dst + lead;
    for (int64_t j = lane; j < n16; j += 64) {
        const int64_t p = ws + lead + 16 * j;
        uint32_t codes, nb;
        if (!minus) fetch16_codes(bases, nmask, g_lo + p, codes, nb);
        else { fetch16_codes(bases, nmask, g_lo + wlen - 16 - p, codes, nb); revcomp16_codes(codes, nb); }   // >= g_lo: p + 16 <= wlen
        uint4 v;
        v.x = ascii4(codes & 0xffu, nb & 0xfu);
        v.y = ascii4((codes >> 8) & 0xffu, (nb >> 4) & 0xfu);
        v.z = ascii4((codes >> 16) & 0xffu, (nb >> 8) & 0xfu);
        v.w = ascii4(codes >> 24, nb >> 12);
        *reinterpret_cast<uint4 *>(d16 + 16 * j) = v;
    }
    const int64_t done = lead + 16 * n16;
    if (done < cnt) emit_span4(bases, nmask, g_lo, wlen, minus, ws + done, cnt - done, dst + done, lane);
}


// <<< genome_decode

// >>> gather_chunk (tests/test_host_gather_chunk.py compiles this block for the host, behind genome_decode, and compares it chunk by
// chunk with plain slicing + pads)
// What the window gather needs to know about a row (row_meta_kernel writes one per row; the gather reads nothing else about it but
// where its slot lies).  The row as it is written: `a` pad bytes, the window [g_lo, g_lo + len) read on its strand, `b` pad bytes;
// under GR_TRUNC the first 500 and the last 500 bytes of that.  A pad byte is the centre's base it faces in lower case -- front pad
// byte i = centre base i, back pad byte j = centre base c_len - b + j -- or HITE_ROW_PAD where the centre has no such base.
struct __attribute__((aligned(16))) GatherRow {
    int64_t g_lo, c_g_lo;      // first base of the window / of the centre's window in the packed genome
    int32_t len, c_len;        // their lengths (0: no window; else >= 100, window_rule)
    uint16_t a, b;             // pad bytes in front / behind (pad_lengths)
    uint32_t flags;
};
#define GR_MINUS 1u            // the window is read reverse-complemented
#define GR_TRUNC 2u            // the first500 + last500 form
#define GR_CMINUS 4u           // the centre's window is read reverse-complemented
#define GR_ITEM_CHUNKS 256     // chunks (of 16 bytes) of a row that one wavefront takes at a time

__device__ __forceinline__ int gather_row_len(const GatherRow &R) {
    if (R.len <= 0) return 0;
    return (R.flags & GR_TRUNC) ? 1000 : (int)R.a + R.len + (int)R.b;
}
// the 16 packed bases that hold positions p .. p + 15 of a window (len >= 16), never leaving the window: the fetch is moved inside
// and gather_align shifts it back, so that nothing in front of g_lo or behind the window's last base is ever asked for
__device__ __forceinline__ int gather_clamp(int len, int p) { return p < 0 ? 0 : (p > len - 16 ? len - 16 : p); }
__device__ __forceinline__ int64_t gather_fetch_pos(int64_t g_lo, int len, bool minus, int p) {
    if (len < 16) return g_lo;                                         // (no window: nothing of the fetch is used)
    const int pf = gather_clamp(len, p);
    return minus ? g_lo + len - 16 - pf : g_lo + pf;
}
// what fetch16_codes read at gather_fetch_pos -> base i = position p + i of the window (whatever lies outside it is not defined)
__device__ __forceinline__ void gather_align(int len, bool minus, int p, uint32_t &codes, uint32_t &nb) {
    if (minus) revcomp16_codes(codes, nb);
    int s = p - gather_clamp(len, p);
    s = s < -15 ? -15 : (s > 15 ? 15 : s);
    if (s > 0) { codes >>= 2 * s; nb >>= s; }
    else if (s < 0) { codes <<= -2 * s; nb = (nb << -s) & 0xffffu; }
}
__device__ __forceinline__ uint4 gather_ascii16(uint32_t codes, uint32_t nb) {
    uint4 v;
    v.x = ascii4(codes & 0xffu, nb & 0xfu);
    v.y = ascii4((codes >> 8) & 0xffu, (nb >> 4) & 0xfu);
    v.z = ascii4((codes >> 16) & 0xffu, (nb >> 8) & 0xfu);
    v.w = ascii4(codes >> 24, (nb >> 12) & 0xfu);
    return v;
}
// bits lo .. hi - 1 of a 16-bit mask (any lo, hi)
__device__ __forceinline__ uint32_t gather_bits(int lo, int hi) {
    lo = lo < 0 ? 0 : (lo > 16 ? 16 : lo);
    hi = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
    return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}
__device__ __forceinline__ uint32_t gather_bytes4(uint32_t m4) {     // bit i -> byte i all ones
    return (((m4 | (m4 << 7) | (m4 << 14) | (m4 << 21)) & 0x01010101u)) * 0xffu;
}
// v where the mask has a bit, else w
__device__ __forceinline__ uint4 gather_select(uint32_t m16, const uint4 &v, const uint4 &w) {
    const uint32_t fx = gather_bytes4(m16 & 0xfu), fy = gather_bytes4((m16 >> 4) & 0xfu), fz = gather_bytes4((m16 >> 8) & 0xfu),
                   fw = gather_bytes4((m16 >> 12) & 0xfu);
    uint4 o;
    o.x = (v.x & fx) | (w.x & ~fx); o.y = (v.y & fy) | (w.y & ~fy); o.z = (v.z & fz) | (w.z & ~fz); o.w = (v.w & fw) | (w.w & ~fw);
    return o;
}
// 16 pad bytes that face the centre's positions pc .. pc + 15
__device__ __forceinline__ uint4 gather_pad16(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask, const GatherRow &R,
                                              int pc) {
    uint4 pad;
    pad.x = pad.y = pad.z = pad.w = 0x01010101u * (uint32_t)HITE_ROW_PAD;
    const uint32_t have = gather_bits(-pc, R.c_len - pc);
    if (!have) return pad;
    const bool cm = (R.flags & GR_CMINUS) != 0;
    uint32_t codes, nb;
    fetch16_codes(bases, nmask, gather_fetch_pos(R.c_g_lo, R.c_len, cm, pc), codes, nb);
    gather_align(R.c_len, cm, pc, codes, nb);
    uint4 v = gather_ascii16(codes, nb);
    v.x |= 0x20202020u; v.y |= 0x20202020u; v.z |= 0x20202020u; v.w |= 0x20202020u;
    return gather_select(have, v, pad);
}
// bytes i0 .. i1 - 1 of a chunk whose byte i is position P + i of the PADDED window (the rest zero); codes / nb: what fetch16_codes
// read at gather_fetch_pos(R.g_lo, R.len, minus, P - a)
__device__ __forceinline__ uint4 gather_seg(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask, const GatherRow &R,
                                            int P, int i0, int i1, uint32_t codes, uint32_t nb) {
    uint4 out;
    out.x = out.y = out.z = out.w = 0u;
    const uint32_t mr = gather_bits(i0, i1);
    const int a = R.a, e = a + R.len;                                  // the window's bases: padded positions a .. e - 1
    const uint32_t mw = mr & gather_bits(a - P, e - P), mf = mr & gather_bits(0, a - P), mb = mr & gather_bits(e - P, 16);
    if (mw) {
        gather_align(R.len, (R.flags & GR_MINUS) != 0, P - a, codes, nb);
        out = gather_select(mw, gather_ascii16(codes, nb), out);
    }
    if (mf) out = gather_select(mf, gather_pad16(bases, nmask, R, P), out);
    if (mb) out = gather_select(mb, gather_pad16(bases, nmask, R, P - e + R.c_len - (int)R.b), out);
    return out;
}
// chunk q of a row (bytes 16 q .. 16 q + 15 of its slot) is bytes 0 .. nA - 1 at padded position PA + i and, only in the chunk that
// holds the seam of the first500 + last500 form (nA < 16), bytes nA .. 15 at padded position PB + i
__device__ __forceinline__ void gather_chunk_plan(const GatherRow &R, int q, int &PA, int &nA, int &PB) {
    const int o0 = 16 * q;
    PA = o0; nA = 16; PB = 0;
    if (R.flags & GR_TRUNC) {
        const int shift = (int)R.a + R.len + (int)R.b - 1000;          // output offset o >= 500 is padded position o + shift
        if (o0 >= 500) PA = o0 + shift;
        else if (o0 + 16 > 500) { nA = 500 - o0; PB = o0 + shift; }
    }
}
// where the chunk's first 16 bases are fetched (the one load every chunk needs; the kernel issues it for several chunks at once)
__device__ __forceinline__ int64_t gather_chunk_src(const GatherRow &R, int q) {
    int PA, nA, PB;
    gather_chunk_plan(R, q, PA, nA, PB);
    return gather_fetch_pos(R.g_lo, R.len, (R.flags & GR_MINUS) != 0, PA - (int)R.a);
}
// the common case: the chunk lies wholly in window bases ...
__device__ __forceinline__ bool gather_chunk_plain(const GatherRow &R, int q) {
    int PA, nA, PB;
    gather_chunk_plan(R, q, PA, nA, PB);
    return nA == 16 && PA >= (int)R.a && PA + 16 <= (int)R.a + R.len;
}
// ... and is one decode of what fetch16_codes read at gather_chunk_src
__device__ __forceinline__ uint4 gather_chunk_decode(const GatherRow &R, uint32_t codes, uint32_t nb) {
    if (R.flags & GR_MINUS) revcomp16_codes(codes, nb);
    return gather_ascii16(codes, nb);
}
// the 16 bytes of any chunk q from what fetch16_codes read at gather_chunk_src: a chunk that touches a pad, the seam or the row's end
// is put together in registers (a second fetch behind the seam, the centre's for a pad), and the bytes behind the row's length are zero
__device__ __forceinline__ uint4 gather_chunk_bytes(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask, const GatherRow &R,
                                                    int q, uint32_t codes, uint32_t nb) {
    if (gather_chunk_plain(R, q)) return gather_chunk_decode(R, codes, nb);
    int PA, nA, PB;
    gather_chunk_plan(R, q, PA, nA, PB);
    const int a = R.a;
    const bool minus = (R.flags & GR_MINUS) != 0;
    const int left = gather_row_len(R) - 16 * q;                       // bytes of the row from this chunk on
    uint4 out = gather_seg(bases, nmask, R, PA, 0, nA < left ? nA : left, codes, nb);
    if (nA < 16 && left > nA) {
        fetch16_codes(bases, nmask, gather_fetch_pos(R.g_lo, R.len, minus, PB - a), codes, nb);
        const uint4 o2 = gather_seg(bases, nmask, R, PB, nA, left < 16 ? left : 16, codes, nb);
        out.x |= o2.x; out.y |= o2.y; out.z |= o2.z; out.w |= o2.w;
    }
    return out;
}
// fetch16_codes in two halves, for a kernel that asks for the words of several chunks before it uses the first: the two words of
// `bases` and the two of `nmask` that hold the 16 bases from packed index g on (bases[g >> 4], the next; nmask[g >> 5], the next)
// -> their codes and "not ACGT" bits
__device__ __forceinline__ void gather_words16(uint32_t b0, uint32_t b1, uint32_t m0, uint32_t m1, int64_t g, uint32_t &codes, uint32_t &nb) {
    codes = (uint32_t)(((uint64_t)b0 | ((uint64_t)b1 << 32)) >> ((int)(g & 15) * 2));
    nb = (uint32_t)(((uint64_t)m0 | ((uint64_t)m1 << 32)) >> (int)(g & 31)) & 0xffffu;
}
__device__ __forceinline__ uint4 gather_chunk(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ nmask, const GatherRow &R, int q) {
    uint32_t codes, nb;
    const int64_t g = gather_chunk_src(R, q);
    gather_words16(bases[g >> 4], bases[(g >> 4) + 1], nmask[g >> 5], nmask[(g >> 5) + 1], g, codes, nb);
    return gather_chunk_bytes(bases, nmask, R, q, codes, nb);
}
// <<< gather_chunk

static __global__ void flank_sizes_kernel(const int64_t *__restrict__ coff, int32_t ncontig, int64_t n,
                                   const int32_t *__restrict__ contig, const int64_t *__restrict__ s1,
                                   const int64_t *__restrict__ e1, int32_t flank, int64_t *__restrict__ out_len,
                                   int64_t *__restrict__ trunc_len) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t len, tlen, g;
    window_rule(coff, ncontig, contig[i], s1[i], e1[i], flank, len, tlen, g);
    out_len[i] = len;
    if (trunc_len) trunc_len[i] = tlen;
}


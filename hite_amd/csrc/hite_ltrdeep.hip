// hite_ltrdeep.hip -- the high-copy LTR vote of FiLTR's hybrid CNN (bin/FiLTR-main/src/Deep_Learning: the feature extractor, class
// CNNCAT and the predictor), restated from the definition in include/hite_gpu.h ("high-copy LTR vote") and PINNED to the reference:
// tests/golden/ltr_deep.json.gz holds the reference's features, logits and decisions, tests/ltrdeep_twin.py is the numpy twin.
//
// Per batch of candidates, on the context's scratch:
//   ld_feature_kernel  ONE WORKGROUP PER CANDIDATE: the matrix becomes digit codes in LDS (A 0 G 1 C 2 T 3 '-' 4); a thread per
//                      column counts the four bases and writes the three planes of the image (the `support` plane through the
//                      101 x 101 table the host builds in binary64); the 2 x 3872 k-mer histogram is built in LDS with integer
//                      adds and written once.
//   ld_normalise_kernel  both feature tensors -> fp32, x / max(|x|_2, 1e-12) over the channel axis, in binary64 rounded once.
//   ld_conv_kernel<CIN, COUT, TH, TW, SC, POOL>  a direct fp32 3 x 3 convolution: a workgroup per tile of TH x TW = 256 pixels, a
//                      thread per pixel holding all COUT sums in registers; the input tile plus halo is staged in LDS 8 planes at a
//                      time, the weights lie as [plane][ky][kx][out] so that one pixel value meets COUT consecutive weights read
//                      through wave-uniform loads.  The sum runs over (plane, ky, kx) ascending in FMAs, so a pixel's value does
//                      not depend on the tile it is in.  Epilogue: scale, shift (the folded batch norm); with SC > 0 the block's
//                      shortcut -- the 1 x 1 convolution of the block's input, its folded batch norm -- is added; ReLU.  With POOL
//                      the planes are not stored: the pixels of the tile are summed per plane in a fixed tree (lanes by xor
//                      shuffles, then the four wavefronts in order) and the tile's 32 sums are written.
//                      The k-mer branch is the same template at H = 1 with tiles of 1 x 256.
//   ld_head_kernel     a wavefront per candidate: lane c sums the tile sums of plane c in ascending order and divides by H x W (the
//                      64 pooled values), then the three linear layers with their folded batch norms, each output one lane's FMAs
//                      in ascending order.
// No floating-point atomic, no sum whose order depends on the launch: the same bits at every batch size and place in a batch.
#include "hite_common.h"
#include "hite_hostbuf.h"
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#define LD_ROWS HITE_LTRDEEP_ROWS
#define LD_COLS HITE_LTRDEEP_COLS
#define LD_HALF (LD_COLS / 2)
#define LD_PIX (LD_ROWS * LD_COLS)
#define LD_KMER HITE_LTRDEEP_KMER
#define LD_K3 124                    // 5^3 - 1 slots of the 3-mers, then 5^4 - 1, then 5^5 - 1
#define LD_K4 624
#define LD_K5 3124
#define LD_TH HITE_LTRDEEP_TILE_H
#define LD_TW HITE_LTRDEEP_TILE_W
#define LD_KT HITE_LTRDEEP_KMER_TILE
#define LD_MIN_ROWS 5
#define LD_PLANES 32                 // planes of the last block of a branch
#define LD_CCH 8                     // input planes staged in LDS at a time
static_assert(LD_K3 + LD_K4 + LD_K5 == LD_KMER, "k-mer slots");
static_assert(LD_TH * LD_TW == 256 && LD_KT == 256, "a thread per pixel of a tile");

// ---- features -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ld_code(uint8_t c) { return c == 'A' ? 0 : c == 'G' ? 1 : c == 'C' ? 2 : c == 'T' ? 3 : 4; }

__global__ __launch_bounds__(256) void ld_feature_kernel(const uint8_t *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                         const uint8_t *__restrict__ support /* [count][total], 101 x 101 */,
                                                         uint8_t *__restrict__ img, int32_t *__restrict__ kmer) {
    __shared__ uint8_t s_code[LD_PIX];
    __shared__ int s_hist[2 * LD_KMER];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t r0 = row_off[b];
    const int nr = (int)(row_off[b + 1] - r0);          // LD_MIN_ROWS .. LD_ROWS: the host sends no other candidate
    const uint8_t *src = rows + r0 * LD_COLS;
    for (int x = tid; x < LD_PIX; x += 256) s_code[x] = (uint8_t)(x < nr * LD_COLS ? ld_code(src[x]) : 4);
    for (int x = tid; x < 2 * LD_KMER; x += 256) s_hist[x] = 0;
    __syncthreads();
    if (tid < LD_COLS) {
        int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        for (int r = 0; r < nr; r++) {
            const int c = s_code[r * LD_COLS + tid];
            n0 += c == 0; n1 += c == 1; n2 += c == 2; n3 += c == 3;
        }
        const int total = n0 + n1 + n2 + n3;
        const uint8_t s0 = support[n0 * 101 + total], s1 = support[n1 * 101 + total], s2 = support[n2 * 101 + total],
                      s3 = support[n3 * 101 + total];
        uint8_t *o = img + (size_t)b * 3 * LD_PIX + tid;
        for (int r = 0; r < LD_ROWS; r++) {
            const int c = s_code[r * LD_COLS + tid];
            o[r * LD_COLS] = c < 4 ? 100 : 0;
            o[LD_PIX + r * LD_COLS] = c == 0 ? s0 : c == 1 ? s1 : c == 2 ? s2 : c == 3 ? s3 : 0;
            o[2 * LD_PIX + r * LD_COLS] = c == 0 ? 50 : c == 1 ? 100 : c == 2 ? 75 : c == 3 ? 25 : 0;
        }
    }
    // every word of 3, 4 and 5 columns that starts at column i of row r of half h (the padding rows hold the all-gap word only)
    const int per_half = nr * (LD_HALF - 2);
    for (int item = tid; item < 2 * per_half; item += 256) {
        const int h = item / per_half, rem = item - h * per_half, r = rem / (LD_HALF - 2), i = rem - r * (LD_HALF - 2);
        const uint8_t *p = s_code + r * LD_COLS + h * LD_HALF + i;
        int *hist = s_hist + h * LD_KMER;
        const int w3 = p[0] * 25 + p[1] * 5 + p[2];
        if (w3 != LD_K3) atomicAdd(hist + w3, 1);
        if (i + 4 <= LD_HALF) {
            const int w4 = w3 * 5 + p[3];
            if (w4 != LD_K4) atomicAdd(hist + LD_K3 + w4, 1);
            if (i + 5 <= LD_HALF) {
                const int w5 = w4 * 5 + p[4];
                if (w5 != LD_K5) atomicAdd(hist + LD_K3 + LD_K4 + w5, 1);
            }
        }
    }
    __syncthreads();
    for (int x = tid; x < 2 * LD_KMER; x += 256) kmer[(size_t)b * 2 * LD_KMER + x] = s_hist[x];
}

// x / max(|x|_2, 1e-12) over the 3 planes of a pixel and the 2 halves of a slot
__global__ __launch_bounds__(256) void ld_normalise_kernel(int n, const uint8_t *__restrict__ img, const int32_t *__restrict__ kmer,
                                                           float *__restrict__ x_img, float *__restrict__ x_kmer) {
    const int64_t per = LD_PIX + LD_KMER, total = (int64_t)n * per;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t b = t / per;
        const int k = (int)(t - b * per);
        if (k < LD_PIX) {
            const uint8_t *p = img + b * 3 * LD_PIX + k;
            const double a0 = p[0], a1 = p[LD_PIX], a2 = p[2 * LD_PIX];
            const double d = fmax(sqrt(a0 * a0 + a1 * a1 + a2 * a2), 1e-12);
            float *o = x_img + b * 3 * LD_PIX + k;
            o[0] = (float)(a0 / d); o[LD_PIX] = (float)(a1 / d); o[2 * LD_PIX] = (float)(a2 / d);
        } else {
            const int s = k - LD_PIX;
            const int32_t *p = kmer + b * 2 * LD_KMER + s;
            const double a0 = p[0], a1 = p[LD_KMER];
            const double d = fmax(sqrt(a0 * a0 + a1 * a1), 1e-12);
            float *o = x_kmer + b * 2 * LD_KMER + s;
            o[0] = (float)(a0 / d); o[LD_KMER] = (float)(a1 / d);
        }
    }
}

// ---- convolutions ---------------------------------------------------------------------------------------------------------------
// in [n][CIN][H][W]; w [CIN][3][3][COUT]; scale, shift [COUT]; SC > 0: sc_in [n][SC][H][W], sc_w [SC][COUT], sc_scale, sc_shift.
// out [n][COUT][H][W], or with POOL [n][tiles][COUT] sums of the tile's pixels.  grid (tiles, n), tiles_x tiles across.
template <int CIN, int COUT, int TH, int TW, int SC, bool POOL>
__global__ __launch_bounds__(256) void ld_conv_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                      const float *__restrict__ scale, const float *__restrict__ shift,
                                                      const float *__restrict__ sc_in, const float *__restrict__ sc_w,
                                                      const float *__restrict__ sc_scale, const float *__restrict__ sc_shift,
                                                      float *__restrict__ out, int H, int W, int tiles_x) {
    constexpr int CCH = CIN < LD_CCH ? CIN : LD_CCH, LH = TH + 2, LW = TW + 2;
    static_assert(TH * TW == 256 && CIN % CCH == 0, "tile");
    __shared__ float s_in[CCH * LH * LW];
    __shared__ float s_red[POOL ? 4 * COUT : 1];
    const int cand = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int ty0 = (tile / tiles_x) * TH, tx0 = (tile % tiles_x) * TW, ty = tid / TW, tx = tid % TW;
    const size_t plane = (size_t)H * W;
    const float *src = in + (size_t)cand * CIN * plane;
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; co++) acc[co] = 0.f;
    for (int c0 = 0; c0 < CIN; c0 += CCH) {
        __syncthreads();          // the planes before have been read
        for (int x = tid; x < CCH * LH * LW; x += 256) {
            const int c = x / (LH * LW), rem = x - c * (LH * LW), yy = rem / LW, xx = rem - yy * LW;
            const int gy = ty0 + yy - 1, gx = tx0 + xx - 1;
            s_in[x] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(size_t)(c0 + c) * plane + (size_t)gy * W + gx] : 0.f;
        }
        __syncthreads();
        const float *wc = w + (size_t)c0 * 9 * COUT;
#pragma unroll
        for (int c = 0; c < CCH; c++)
#pragma unroll
            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++) {
                    const float v = s_in[(c * LH + ty + ky) * LW + tx + kx];
                    const float *wp = wc + ((c * 3 + ky) * 3 + kx) * COUT;
#pragma unroll
                    for (int co = 0; co < COUT; co++) acc[co] = fmaf(v, wp[co], acc[co]);
                }
    }
    const int gy = ty0 + ty, gx = tx0 + tx;
    const bool inside = gy < H && gx < W;
    const size_t pix = (size_t)gy * W + gx;
#pragma unroll
    for (int co = 0; co < COUT; co++) acc[co] = fmaf(acc[co], scale[co], shift[co]);
    if constexpr (SC > 0) {
        float xs[SC];
#pragma unroll
        for (int ci = 0; ci < SC; ci++) xs[ci] = inside ? sc_in[((size_t)cand * SC + ci) * plane + pix] : 0.f;
#pragma unroll
        for (int co = 0; co < COUT; co++) {
            float s = 0.f;
#pragma unroll
            for (int ci = 0; ci < SC; ci++) s = fmaf(xs[ci], sc_w[ci * COUT + co], s);
            acc[co] += fmaf(s, sc_scale[co], sc_shift[co]);
        }
    }
#pragma unroll
    for (int co = 0; co < COUT; co++) acc[co] = fmaxf(acc[co], 0.f);
    if constexpr (!POOL) {
        if (inside) {
#pragma unroll
            for (int co = 0; co < COUT; co++) out[((size_t)cand * COUT + co) * plane + pix] = acc[co];
        }
    } else {
        const int lane = lane_id(), wv = wave_id();
#pragma unroll
        for (int co = 0; co < COUT; co++) {
            float v = inside ? acc[co] : 0.f;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
            if (lane == 0) s_red[wv * COUT + co] = v;
        }
        __syncthreads();
        if (tid < COUT)
            out[((size_t)cand * gridDim.x + tile) * COUT + tid] = ((s_red[tid] + s_red[COUT + tid]) + s_red[2 * COUT + tid]) + s_red[3 * COUT + tid];
    }
}

// ---- pooling and head -----------------------------------------------------------------------------------------------------------
// fc: w1 [16][64], s1, t1 [16], w2 [8][16], s2, t2 [8], w3 [2][8], b3 [2]
#define LD_FC_W1 0
#define LD_FC_S1 (LD_FC_W1 + 16 * 64)
#define LD_FC_T1 (LD_FC_S1 + 16)
#define LD_FC_W2 (LD_FC_T1 + 16)
#define LD_FC_S2 (LD_FC_W2 + 8 * 16)
#define LD_FC_T2 (LD_FC_S2 + 8)
#define LD_FC_W3 (LD_FC_T2 + 8)
#define LD_FC_B3 (LD_FC_W3 + 2 * 8)
#define LD_FC_FLOATS (LD_FC_B3 + 2)
__global__ __launch_bounds__(64) void ld_head_kernel(const float *__restrict__ part_img, int tiles_img, const float *__restrict__ part_kmer,
                                                     int tiles_kmer, const float *__restrict__ fc, float *__restrict__ pooled,
                                                     float *__restrict__ logits) {
    __shared__ float s_x[64], s_h1[16], s_h2[8];
    const int b = blockIdx.x, lane = threadIdx.x;
    {
        const bool k = lane >= LD_PLANES;
        const int tiles = k ? tiles_kmer : tiles_img;
        const float *p = (k ? part_kmer : part_img) + (size_t)b * tiles * LD_PLANES + (lane & (LD_PLANES - 1));
        float s = 0.f;
        for (int t = 0; t < tiles; t++) s += p[(size_t)t * LD_PLANES];
        s = s / (k ? (float)LD_KMER : (float)LD_PIX);
        s_x[lane] = s;
        pooled[(size_t)b * 64 + lane] = s;
    }
    __syncthreads();
    if (lane < 16) {
        float a = 0.f;
        for (int i = 0; i < 64; i++) a = fmaf(fc[LD_FC_W1 + lane * 64 + i], s_x[i], a);
        s_h1[lane] = fmaxf(fmaf(a, fc[LD_FC_S1 + lane], fc[LD_FC_T1 + lane]), 0.f);
    }
    __syncthreads();
    if (lane < 8) {
        float a = 0.f;
        for (int i = 0; i < 16; i++) a = fmaf(fc[LD_FC_W2 + lane * 16 + i], s_h1[i], a);
        s_h2[lane] = fmaxf(fmaf(a, fc[LD_FC_S2 + lane], fc[LD_FC_T2 + lane]), 0.f);
    }
    __syncthreads();
    if (lane < 2) {
        float a = 0.f;
        for (int i = 0; i < 8; i++) a = fmaf(fc[LD_FC_W3 + lane * 8 + i], s_h2[i], a);
        logits[(size_t)b * 2 + lane] = a + fc[LD_FC_B3 + lane];
    }
}

// ---- the model on the device ----------------------------------------------------------------------------------------------------
struct LdConv { size_t w, scale, shift; };             // offsets (floats) into the model's buffer
struct LdBlock { LdConv c1, c2, sc; };
struct LdModel {
    int device;
    float *d;
    LdBlock blk[2][3];        // [img | kmer][block]
    size_t fc;
};

// one convolution of the canonical array: weight [cout][cin][k][k], then gamma, beta, mean, var -> [cin][k][k][cout], scale, shift
static const float *ld_fold_conv(const float *p, int cin, int cout, int k, std::vector<float> &buf, LdConv &at) {
    auto pad = [&]() { buf.resize((buf.size() + 63) & ~(size_t)63); };      // every tensor at a multiple of 256 bytes
    pad();
    at.w = buf.size();
    buf.resize(at.w + (size_t)cin * k * k * cout);
    for (int co = 0; co < cout; co++)
        for (int ci = 0; ci < cin; ci++)
            for (int q = 0; q < k * k; q++) buf[at.w + ((size_t)ci * k * k + q) * cout + co] = p[((size_t)co * cin + ci) * k * k + q];
    p += (size_t)cout * cin * k * k;
    pad();
    at.scale = buf.size();
    buf.resize(at.scale + cout);
    pad();
    at.shift = buf.size();
    buf.resize(at.shift + cout);
    for (int co = 0; co < cout; co++) {
        const double s = (double)p[co] / sqrt((double)p[3 * cout + co] + 1e-5);
        buf[at.scale + co] = (float)s;
        buf[at.shift + co] = (float)((double)p[cout + co] - (double)p[2 * cout + co] * s);
    }
    return p + 4 * (size_t)cout;
}

extern "C" int hite_ltr_model_build(hite_ctx *ctx, const float *params, int64_t n_params, void **model_out) {
    if (!ctx || !params || !model_out || n_params != HITE_LTRDEEP_PARAMS) return HITE_EINVAL;
    for (int64_t i = 0; i < n_params; i++)
        if (!std::isfinite(params[i])) return HITE_EINVAL;
    try {
        std::vector<float> buf;
        LdModel built{};
        LdModel *m = &built;          // (copied to the heap once nothing below can throw)
        m->device = ctx->device;
        m->d = nullptr;
        const float *p = params;
        static const int chan[4] = {0, 8, 16, 32};
        for (int br = 0; br < 2; br++)
            for (int k = 0; k < 3; k++) {
                const int cin = k == 0 ? (br == 0 ? 3 : 2) : chan[k], cout = chan[k + 1];
                p = ld_fold_conv(p, cin, cout, 3, buf, m->blk[br][k].c1);
                p = ld_fold_conv(p, cout, cout, 3, buf, m->blk[br][k].c2);
                p = ld_fold_conv(p, cin, cout, 1, buf, m->blk[br][k].sc);
            }
        // the head: y = ((W x + b) - mean) * s + beta = (W x) * s + ((b - mean) * s + beta)
        buf.resize((buf.size() + 63) & ~(size_t)63);
        m->fc = buf.size();
        buf.resize(m->fc + LD_FC_FLOATS);
        float *fc = buf.data() + m->fc;
        auto linear_bn = [&](int nin, int nout, int w_at, int s_at, int t_at) {
            const float *wt = p, *b = p + (size_t)nin * nout, *bn = b + nout;
            memcpy(fc + w_at, wt, sizeof(float) * nin * nout);
            for (int o = 0; o < nout; o++) {
                const double s = (double)bn[o] / sqrt((double)bn[3 * nout + o] + 1e-5);
                fc[s_at + o] = (float)s;
                fc[t_at + o] = (float)(((double)b[o] - (double)bn[2 * nout + o]) * s + (double)bn[nout + o]);
            }
            p = bn + 4 * (size_t)nout;
        };
        linear_bn(64, 16, LD_FC_W1, LD_FC_S1, LD_FC_T1);
        linear_bn(16, 8, LD_FC_W2, LD_FC_S2, LD_FC_T2);
        memcpy(fc + LD_FC_W3, p, sizeof(float) * 16);
        memcpy(fc + LD_FC_B3, p + 16, sizeof(float) * 2);
        p += 18;
        if (p - params != HITE_LTRDEEP_PARAMS) return HITE_EINVAL;
        LdModel *heap = new LdModel(built);
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipMalloc((void **)&heap->d, buf.size() * sizeof(float) + 256);
        if (e == hipSuccess) e = hipMemcpy(heap->d, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (heap->d) (void)hipFree(heap->d);
            delete heap;
            HITE_CHECK(ctx, e);
        }
        *model_out = heap;
        return HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

extern "C" void hite_ltr_model_release(void *model) {
    LdModel *m = (LdModel *)model;
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->d) (void)hipFree(m->d);
    delete m;
}

// ---- the host side of a call ----------------------------------------------------------------------------------------------------
template <int CIN, int COUT, int TH, int TW, int SC, bool POOL>
static void ld_launch(hipStream_t st, int n, int H, int W, const float *in, const float *P, const LdConv &c, const float *sc_in,
                      const LdConv &s, float *out) {
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    hipLaunchKernelGGL((ld_conv_kernel<CIN, COUT, TH, TW, SC, POOL>), dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(256), 0, st, in,
                       P + c.w, P + c.scale, P + c.shift, sc_in, P + s.w, P + s.scale, P + s.shift, out, H, W, tiles_x);
}
// the three blocks of a branch: x [n][C0] -> the tile sums of the 32 planes of the last block; t, y1, y2: planes of 32, 8, 16
template <int C0, int TH, int TW>
static void ld_branch(hipStream_t st, int n, int H, int W, const float *x, float *t, float *y1, float *y2, float *part, const float *P,
                      const LdBlock *b) {
    ld_launch<C0, 8, TH, TW, 0, false>(st, n, H, W, x, P, b[0].c1, nullptr, b[0].sc, t);
    ld_launch<8, 8, TH, TW, C0, false>(st, n, H, W, t, P, b[0].c2, x, b[0].sc, y1);
    ld_launch<8, 16, TH, TW, 0, false>(st, n, H, W, y1, P, b[1].c1, nullptr, b[1].sc, t);
    ld_launch<16, 16, TH, TW, 8, false>(st, n, H, W, t, P, b[1].c2, y1, b[1].sc, y2);
    ld_launch<16, 32, TH, TW, 0, false>(st, n, H, W, y2, P, b[2].c1, nullptr, b[2].sc, t);
    ld_launch<32, 32, TH, TW, 16, true>(st, n, H, W, t, P, b[2].c2, y2, b[2].sc, part);
}

#define LD_TILES_IMG (((LD_ROWS + LD_TH - 1) / LD_TH) * ((LD_COLS + LD_TW - 1) / LD_TW))
#define LD_TILES_KMER ((LD_KMER + LD_KT - 1) / LD_KT)

// model == NULL: the features alone (img, kmer); else logits and, when given, pooled
static int ld_run(hite_ctx *ctx, const LdModel *model, int64_t n, const uint8_t *rows, const int64_t *row_off, float *logits, float *pooled,
                  uint8_t *img, int32_t *kmer, int8_t *status) {
    if (!ctx || n < 0) return HITE_EINVAL;
    if (n == 0) return HITE_OK;
    if (!row_off || !status || !csr_ok(row_off, n)) return HITE_EINVAL;
    if (model ? !logits : (!img || !kmer)) return HITE_EINVAL;
    if (row_off[n] > row_off[0] && !rows) return HITE_EINVAL;
    if (model && model->device != ctx->device) return HITE_EINVAL;
    try {
        std::vector<int64_t> scored;
        for (int64_t c = 0; c < n; c++) {
            const int64_t nr = row_off[c + 1] - row_off[c];
            const bool ok = nr >= LD_MIN_ROWS && nr <= LD_ROWS;
            status[c] = ok ? 0 : 1;
            if (ok) { scored.push_back(c); continue; }
            if (model) {
                logits[2 * c] = logits[2 * c + 1] = 0.f;
                if (pooled) memset(pooled + 64 * c, 0, 64 * sizeof(float));
            } else {
                memset(img + (size_t)c * 3 * LD_PIX, 0, 3 * LD_PIX);
                memset(kmer + (size_t)c * 2 * LD_KMER, 0, 2 * LD_KMER * sizeof(int32_t));
            }
        }
        if (scored.empty()) return HITE_OK;
        const size_t B = (size_t)std::min<int64_t>(ctx->ltrdeep_batch > 0 ? ctx->ltrdeep_batch : HITE_LTRDEEP_BATCH_DEFAULT, (int64_t)scored.size());
        const size_t Bm = model ? B : 0;          // the planes exist only with a model
        // 0 rows, 1 row offsets, 2 support table, 3 img, 4 kmer, 5 / 6 normalised, 7 - 9 img planes t, y1, y2, 10 - 12 kmer planes,
        // 13 / 14 tile sums, 15 pooled, 16 logits
        const ScratchPlan lay({{1, B * LD_PIX, 16}, {8, B + 1, 0}, {1, 101 * 101, 0}, {1, B * 3 * LD_PIX, 0}, {4, B * 2 * LD_KMER, 0},
                               {4, Bm * 3 * LD_PIX, 0}, {4, Bm * 2 * LD_KMER, 0},
                               {4, Bm * 32 * LD_PIX, 0}, {4, Bm * 8 * LD_PIX, 0}, {4, Bm * 16 * LD_PIX, 0},
                               {4, Bm * 32 * LD_KMER, 0}, {4, Bm * 8 * LD_KMER, 0}, {4, Bm * 16 * LD_KMER, 0},
                               {4, Bm * LD_TILES_IMG * LD_PLANES, 0}, {4, Bm * LD_TILES_KMER * LD_PLANES, 0}, {4, Bm * 64, 0}, {4, Bm * 2, 0}});
        HITE_CHECK(ctx, hipSetDevice(ctx->device));
        void *scr = nullptr;
        const int rc = hite_scratch_reserve(ctx, lay.total + 256, &scr);
        if (rc) return rc;
        uint8_t *d_rows = lay.at<uint8_t>(scr, 0);
        int64_t *d_off = lay.at<int64_t>(scr, 1);
        uint8_t *d_sup = lay.at<uint8_t>(scr, 2), *d_img = lay.at<uint8_t>(scr, 3);
        int32_t *d_kmer = lay.at<int32_t>(scr, 4);
        float *d_ximg = lay.at<float>(scr, 5), *d_xk = lay.at<float>(scr, 6);
        float *d_ti = lay.at<float>(scr, 7), *d_y1i = lay.at<float>(scr, 8), *d_y2i = lay.at<float>(scr, 9);
        float *d_tk = lay.at<float>(scr, 10), *d_y1k = lay.at<float>(scr, 11), *d_y2k = lay.at<float>(scr, 12);
        float *d_pi = lay.at<float>(scr, 13), *d_pk = lay.at<float>(scr, 14), *d_pool = lay.at<float>(scr, 15), *d_log = lay.at<float>(scr, 16);
        hipStream_t st = nullptr;
        // support[count][total] = int((count / total) * 100) in binary64, as the reference's Python evaluates it
        std::vector<uint8_t> sup(101 * 101, 0);
        for (int c = 0; c <= 100; c++)
            for (int t = std::max(c, 1); t <= 100; t++) sup[c * 101 + t] = (uint8_t)(int)(((double)c / (double)t) * 100.0);
        HITE_CHECK(ctx, hipMemcpyAsync(d_sup, sup.data(), sup.size(), hipMemcpyHostToDevice, st));
        std::vector<uint8_t> stage;
        std::vector<int64_t> off;
        std::vector<float> h_log, h_pool;
        for (size_t at = 0; at < scored.size(); at += B) {
            const size_t nb = std::min(B, scored.size() - at);
            off.assign(nb + 1, 0);
            for (size_t k = 0; k < nb; k++) off[k + 1] = off[k] + (row_off[scored[at + k] + 1] - row_off[scored[at + k]]);
            stage.resize((size_t)off[nb] * LD_COLS);
            for (size_t k = 0; k < nb; k++)
                memcpy(stage.data() + (size_t)off[k] * LD_COLS, rows + (size_t)row_off[scored[at + k]] * LD_COLS, (size_t)(off[k + 1] - off[k]) * LD_COLS);
            HITE_CHECK(ctx, hipMemcpyAsync(d_rows, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
            HITE_CHECK(ctx, hipMemcpyAsync(d_off, off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
            int tk = hite_prof_begin(ctx, "ltrdeep_features", st);
            hipLaunchKernelGGL(ld_feature_kernel, dim3((unsigned)nb), dim3(256), 0, st, d_rows, d_off, d_sup, d_img, d_kmer);
            if (model)
                hipLaunchKernelGGL(ld_normalise_kernel, dim3((unsigned)std::min<size_t>(nb * 94, 2048)), dim3(256), 0, st, (int)nb, d_img, d_kmer,
                                   d_ximg, d_xk);
            hite_prof_end(ctx, tk, st);
            HITE_CHECK(ctx, hipGetLastError());
            if (!model) {
                for (size_t k = 0; k < nb; k++) {           // (the scored candidates of a batch need not be neighbours in the call)
                    HITE_CHECK(ctx, hipMemcpyAsync(img + (size_t)scored[at + k] * 3 * LD_PIX, d_img + k * 3 * LD_PIX, 3 * LD_PIX, hipMemcpyDeviceToHost, st));
                    HITE_CHECK(ctx, hipMemcpyAsync(kmer + (size_t)scored[at + k] * 2 * LD_KMER, d_kmer + k * 2 * LD_KMER, 2 * LD_KMER * 4,
                                                   hipMemcpyDeviceToHost, st));
                }
                HITE_CHECK(ctx, hipStreamSynchronize(st));
                continue;
            }
            tk = hite_prof_begin(ctx, "ltrdeep_conv", st);
            ld_branch<3, LD_TH, LD_TW>(st, (int)nb, LD_ROWS, LD_COLS, d_ximg, d_ti, d_y1i, d_y2i, d_pi, model->d, model->blk[0]);
            ld_branch<2, 1, LD_KT>(st, (int)nb, 1, LD_KMER, d_xk, d_tk, d_y1k, d_y2k, d_pk, model->d, model->blk[1]);
            hite_prof_end(ctx, tk, st);
            HITE_CHECK(ctx, hipGetLastError());
            tk = hite_prof_begin(ctx, "ltrdeep_head", st);
            hipLaunchKernelGGL(ld_head_kernel, dim3((unsigned)nb), dim3(64), 0, st, d_pi, LD_TILES_IMG, d_pk, LD_TILES_KMER, model->d + model->fc,
                               d_pool, d_log);
            hite_prof_end(ctx, tk, st);
            HITE_CHECK(ctx, hipGetLastError());
            h_log.resize(nb * 2);
            h_pool.resize(nb * 64);
            HITE_CHECK(ctx, hipMemcpyAsync(h_log.data(), d_log, nb * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
            if (pooled) HITE_CHECK(ctx, hipMemcpyAsync(h_pool.data(), d_pool, nb * 64 * sizeof(float), hipMemcpyDeviceToHost, st));
            HITE_CHECK(ctx, hipStreamSynchronize(st));          // the next batch overwrites the scratch
            for (size_t k = 0; k < nb; k++) {
                const int64_t c = scored[at + k];
                logits[2 * c] = h_log[2 * k];
                logits[2 * c + 1] = h_log[2 * k + 1];
                if (pooled) memcpy(pooled + 64 * c, h_pool.data() + 64 * k, 64 * sizeof(float));
            }
        }
        hite_prof_resolve(ctx);
        return HITE_OK;
    } catch (const std::bad_alloc &) {
        return HITE_ENOMEM;
    }
}

extern "C" int hite_ltr_deep(hite_ctx *ctx, void *model, int64_t n, const uint8_t *rows, const int64_t *row_off, float *logits, float *pooled,
                             int8_t *status) {
    if (!model) return HITE_EINVAL;
    return ld_run(ctx, (const LdModel *)model, n, rows, row_off, logits, pooled, nullptr, nullptr, status);
}

extern "C" int hite_ltr_deep_features(hite_ctx *ctx, int64_t n, const uint8_t *rows, const int64_t *row_off, uint8_t *img, int32_t *kmer,
                                      int8_t *status) {
    return ld_run(ctx, nullptr, n, rows, row_off, nullptr, nullptr, img, kmer, status);
}

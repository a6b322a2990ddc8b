// mask_kernels.h — per-pixel multi-style blending (rrv_transfer_image_mask_device, rrv_transfer_mask_batch).
//
// The reference's multi-style interpolation replaces every saved quantity q of the decoder by sum_s w_s q_s, one weight vector
// per frame ("Multi-style Interpolation/style_network.py":35-53 mean / rstd / min / max, :135-139 filters, :348-360 style
// moments).  Here the weights vary per pixel: a mask M[S][H][W] at the frame's resolution, averaged down to the resolution of
// each decoder level, and q(p) = sum_s m_s(p) q_s at tensor pixel p.  Three kernels:
//   mask_pyramid_k   the four level masks (stride 1, 2, 4, 8 of the network's input frame) in one pass over the planar mask,
//                    through the edge-inclusive reflect pad of the pad/crop geometry;
//   mask_norm_k      InstanceNorm.forward with saved statistics blended per pixel (+ the upsampled shortcut, + the AdaIN affine);
//   mask_filter_k    KernelFilter's two dynamic 32 x 32 filters blended per pixel, around the LeakyReLU, on the raw output of
//                    the unfolded down_sample convolution (and the sum of its split-K partial sums).
// The states of the S styles are only read.
#pragma once
#include <hip/hip_runtime.h>
#include "conv_thin.h"   // f32x4, reflect_sym

constexpr int MASK_MAX_STYLES = 8;      // = RRV_MAX_STYLES
struct MaskStates { const float* blob[MASK_MAX_STYLES]; };      // the computed state blobs of styles 0..S-1 (RRV_STATE_FLOATS each)

// One level mask as its consumers read it: the weights of pixel (y, x) of image b are the S floats at
// p + b * bstride + y * pitch + x * S (S innermost: one pixel's weights are contiguous, a row's pixels follow each other).
// bstride == 0: one mask for every image.  The floats live in the interior pixels of a ring-layout tensor of MASK_MAX_STYLES
// channels (a row of w pixels holds w * S <= w * 8 floats from its first interior pixel on), so ring and slack stay zero.
struct LevelMask { const float* p; long bstride; int pitch; int S; };

// ---- the four level masks --------------------------------------------------------------------------------------------
// src: planar [Bm][S][SH][SW].  pad: the network's frame is the reflect-padded source (pixel (Y, X) reads source pixel
// (reflect(Y - top), reflect(X - left)), edge-inclusive, as conv_first_k reads the frame); else pixel (Y, X) reads source
// pixel (Y, X) and rows / columns beyond 8 * (SH / 8), 8 * (SW / 8) are never read.  Level l + 1 is the mean of the 2 x 2
// block of level l, ((a + b) + (c + d)) * 0.25 with a, b the upper row: a fixed order, the same for every batch.
struct MaskPyrP {
    const float* src; int SH, SW, pad, top, left;
    int h8, w8;                     // the 1/8 level: every thread makes one of its pixels, and the 8 x 8, 4 x 4, 2 x 2 blocks above it
    float* lv[4]; long bstride[4]; int pitch[4];      // LevelMask geometry of level 0 (full resolution) .. 3 (1/8), writable
};
template <int S>
__global__ __launch_bounds__(256) void mask_pyramid_k(const MaskPyrP p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.h8 * p.w8) return;
    const int y8 = i / p.w8, x8 = i - y8 * p.w8, b = blockIdx.y;
    const float* src = p.src + (size_t)b * S * p.SH * p.SW;
    int sx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) sx[c] = p.pad ? reflect_sym(x8 * 8 + c - p.left, p.SW) : x8 * 8 + c;
    float* const o0 = p.lv[0] + b * p.bstride[0] + (size_t)x8 * 8 * S;
    float* const o1 = p.lv[1] + b * p.bstride[1] + (size_t)x8 * 4 * S;
    float* const o2 = p.lv[2] + b * p.bstride[2] + (size_t)x8 * 2 * S;
    float* const o3 = p.lv[3] + b * p.bstride[3] + (size_t)x8 * S;
    float half[S][4], l1[2][S][4], l2[2][S][2];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int Y = y8 * 8 + r;
        const int sy = p.pad ? reflect_sym(Y - p.top, p.SH) : Y;
        float row[8 * S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float* line = src + ((size_t)s * p.SH + sy) * p.SW;
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) { v[c] = line[sx[c]]; row[c * S + s] = v[c]; }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float hs = v[2 * c] + v[2 * c + 1];
                if (r & 1) l1[(r >> 1) & 1][s][c] = (half[s][c] + hs) * 0.25f;
                else half[s][c] = hs;
            }
        }
        {   // level 0: 8 pixels x S floats, contiguous and 16-byte aligned
            f32x4* d = (f32x4*)(o0 + (size_t)Y * p.pitch[0]);
#pragma unroll
            for (int k = 0; k < 2 * S; ++k) d[k] = f32x4{row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]};
        }
        if (r & 1) {   // level 1: 4 pixels x S floats
            const int a = (r >> 1) & 1;
            float o[4 * S];
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c * S + s] = l1[a][s][c];
            f32x4* d = (f32x4*)(o1 + (size_t)(Y >> 1) * p.pitch[1]);
#pragma unroll
            for (int k = 0; k < S; ++k) d[k] = f32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
        }
        if ((r & 3) == 3) {   // level 2: 2 pixels x S floats
            const int a = (r >> 2) & 1;
            float* d = o2 + (size_t)(Y >> 2) * p.pitch[2];
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    l2[a][s][c] = ((l1[0][s][2 * c] + l1[0][s][2 * c + 1]) + (l1[1][s][2 * c] + l1[1][s][2 * c + 1])) * 0.25f;
                    d[c * S + s] = l2[a][s][c];
                }
        }
    }
    float* d = o3 + (size_t)y8 * p.pitch[3];
#pragma unroll
    for (int s = 0; s < S; ++s) d[s] = ((l2[0][s][0] + l2[0][s][1]) + (l2[1][s][0] + l2[1][s][1])) * 0.25f;
}

// ---- masked normalisation / AdaIN ------------------------------------------------------------------------------------
// y = clamp((x - mean(p)) * rstd(p), lo(p), hi(p)) [+ res, upsampled 2x] [* std(p) + mean_style(p)], every parameter row
// blended per pixel: q(p)[c] = sum_s m_s(p) q_s[c] (s ascending).  The steps and their order are pointwise_k's (res_mode 2).
// Ring layout in and out, valid pixels only; y may alias x.
// A block owns one image row segment and one group of 64 channels: the 4 (6 with AdaIN) parameter rows of the S states for
// that group are loaded into LDS once per block; a thread keeps one channel quad and walks the pixels 16 apart.
struct MaskNormP {
    const float* x; float* y;
    int B, H, W, C;
    MaskStates st; int S;
    int n_off;                       // the normalisation entry in a blob: mean, rstd, lo, hi, C floats each
    int sty_off;                     // the style (mean, std) entry, or -1
    const float* res; int Hr, Wr;    // half-resolution shortcut [B][Hr+2][Wr+2][C], or null
    LevelMask m;
    int segs;                        // blocks per image row and channel group
};
__global__ __launch_bounds__(256) void mask_norm_k(const MaskNormP p) {
    __shared__ __attribute__((aligned(16))) float par[6][MASK_MAX_STYLES][64];
    const int tid = threadIdx.x;
    const int CG = p.C >> 6;
    int bx = blockIdx.x;
    const int cg = bx % CG; bx /= CG;
    const int sg = bx % p.segs;
    const int r = bx / p.segs;
    const int b = r / p.H, y = r - b * p.H;
    const int nrow = p.sty_off >= 0 ? 6 : 4;
    for (int s = 0; s < p.S; ++s) {
        const float* blob = p.st.blob[s];
        for (int i = tid; i < nrow * 64; i += 256) {
            const int k = i >> 6, c = i & 63;
            par[k][s][c] = k < 4 ? blob[p.n_off + k * p.C + cg * 64 + c] : blob[p.sty_off + (k - 4) * p.C + cg * 64 + c];
        }
    }
    __syncthreads();
    const int q4 = (tid & 15) * 4, c4 = cg * 64 + q4;
    const long row = (((long)b * (p.H + 2) + y + 1) * (p.W + 2) + 1) * (long)p.C + c4;
    const long rrow = p.res ? (((long)b * (p.Hr + 2) + (y >> 1) + 1) * (p.Wr + 2) + 1) * (long)p.C + c4 : 0;
    const float* mrow = p.m.p + b * p.m.bstride + (long)y * p.m.pitch;
    const int S = p.S;
    for (int x = sg * 16 + (tid >> 4); x < p.W; x += p.segs * 16) {
        const long idx = row + (long)x * p.C;
        f32x4 v = *(const f32x4*)(p.x + idx);
        f32x4 rv = {0.f, 0.f, 0.f, 0.f};
        if (p.res) rv = *(const f32x4*)(p.res + rrow + (long)(x >> 1) * p.C);
        const float* mk = mrow + (long)x * S;
        f32x4 q[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) q[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < S; ++s) {
            const float w = mk[s];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] += w * *(const f32x4*)&par[k][s][q4];
            if (nrow == 6) {
                q[4] += w * *(const f32x4*)&par[4][s][q4];
                q[5] += w * *(const f32x4*)&par[5][s][q4];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float tv = (v[e] - q[0][e]) * q[1][e];
            tv = fminf(q[3][e], fmaxf(q[2][e], tv));
            if (p.res) tv += rv[e];
            if (nrow == 6) tv = tv * q[5][e] + q[4][e];
            v[e] = tv;
        }
        *(f32x4*)(p.y + idx) = v;
    }
}

// ---- masked KernelFilter ---------------------------------------------------------------------------------------------
// KernelFilter.forward between its two convolutions (test/style_network_global.py:210-217 with apply_filter :194-208):
//   d(p) = down_sample(x)(p)                  the raw convolution output: `split` partial sums per pixel + the bias
//   e(p) = LeakyReLU(F1(p) d(p))              F(p)[i][j] = sum_s m_s(p) F_s[i][j], out[i] = sum_j F[i][j] in[j]
//   out(p) = F2(p) e(p)                       what the 3 x 3 upsample convolution then reads
// A block handles 64 pixels, 8 at a time (a thread = one pixel and one of the 32 channels): the S filters F1_s are staged in
// LDS transposed (consecutive channels i in consecutive banks), applied to all 64 pixels, then F2_s take their place.  The filters
// take S x 32 x 33 floats of DYNAMIC LDS (mask_filter_smem(S): 8.3 KB at S = 2 next to 18 KB static, several workgroups per CU).
// `out` may be `part` itself (split == 1: the raw convolution output is filtered in place): a block reads all of its 64 pixels into
// LDS, passes a __syncthreads, and only then writes those same pixels; no block touches another block's pixels.
struct MaskFilterP {
    const float* part; int split;   // [B][h+2][w+2][32 * split] ring layout
    float* out;                     // [B][h+2][w+2][32] ring layout, interior pixels only
    const float* bias;              // down_sample's bias [32]
    MaskStates st; int S; int f1_off, f2_off;      // the two filters' offsets in a blob ([32][32] each)
    LevelMask m;                    // the 1/8 level mask
    int B, h, w;
};
inline size_t mask_filter_smem(int S) { return (size_t)S * 32 * 33 * sizeof(float); }
__global__ __launch_bounds__(256) void mask_filter_k(const MaskFilterP p) {
    extern __shared__ __attribute__((aligned(16))) float mask_filter_lds[];
    float (*Ft)[32][33] = (float (*)[32][33])mask_filter_lds;      // [s][j][i], rows padded: the transposing stores hit 32 banks too
    __shared__ float xs[64][32], e1[64][32], mk[64][MASK_MAX_STYLES];
    const int tid = threadIdx.x, i = tid & 31, pl = tid >> 5, S = p.S;
    const long npix = (long)p.B * p.h * p.w;
    const long pix0 = (long)blockIdx.x * 64;
    auto ring_px = [&](long pid, int& b, int& y, int& x) {
        b = (int)(pid / ((long)p.h * p.w));
        const int rem = (int)(pid - (long)b * p.h * p.w);
        y = rem / p.w; x = rem - y * p.w;
        return ((long)b * (p.h + 2) + y + 1) * (p.w + 2) + x + 1;
    };
    auto stage = [&](int off) {
        for (int s = 0; s < S; ++s) {
            const float* F = p.st.blob[s] + off;
            for (int k = tid; k < 1024; k += 256) Ft[s][k & 31][k >> 5] = F[k];      // F[i][j] -> Ft[j][i]
        }
    };
    stage(p.f1_off);
    for (int g = 0; g < 8; ++g) {
        const long pid = pix0 + g * 8 + pl;
        float v = 0.f;
        if (pid < npix) {
            int b, y, x;
            const long px = ring_px(pid, b, y, x);
            const float* src = p.part + px * 32 * p.split + i;
            v = src[0];
            for (int k = 1; k < p.split; ++k) v += src[32 * k];
            v += p.bias[i];
            if (i < S) mk[g * 8 + pl][i] = p.m.p[b * p.m.bstride + (long)y * p.m.pitch + (long)x * S + i];
        }
        xs[g * 8 + pl][i] = v;
    }
    __syncthreads();
    for (int g = 0; g < 8; ++g) {
        const int q = g * 8 + pl;
        float acc = 0.f;
        if (pix0 + q < npix) {
            for (int j = 0; j < 32; ++j) {
                float f = 0.f;
                for (int s = 0; s < S; ++s) f += mk[q][s] * Ft[s][j][i];
                acc += f * xs[q][j];
            }
        }
        e1[q][i] = acc >= 0.f ? acc : acc * 0.2f;
    }
    __syncthreads();
    stage(p.f2_off);
    __syncthreads();
    for (int g = 0; g < 8; ++g) {
        const int q = g * 8 + pl;
        const long pid = pix0 + q;
        if (pid >= npix) continue;
        float acc = 0.f;
        for (int j = 0; j < 32; ++j) {
            float f = 0.f;
            for (int s = 0; s < S; ++s) f += mk[q][s] * Ft[s][j][i];
            acc += f * e1[q][j];
        }
        int b, y, x;
        p.out[ring_px(pid, b, y, x) * 32 + i] = acc;
    }
}

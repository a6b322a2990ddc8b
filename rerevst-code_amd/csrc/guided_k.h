// guided_k.h — the guided delivery stage (include/rerevst_hip.h "Guided delivery"), gfx950; part of stages.hip (librerevst_stages.so).
//
// Joint upsampling with the fast guided filter (He & Sun 2015): the source's luma g guides the stylized working frame P to the delivered size.
// Both kernels are bound by HBM traffic; all their scratch is dynamic LDS in planar form ([plane][row][column], 4-byte accesses at stride one:
// consecutive lanes on consecutive banks), and every global access has consecutive lanes on consecutive pixels of a row.
//
// gf_coeff_k: one workgroup of 256 threads owns GF_CT_H x GF_CT_W working pixels of one frame.
//   1  stage, global memory -> LDS: g and the three channels of P over the tile and a halo of r pixels, each minus the tile's anchor (the value
//      at the tile's centre pixel), and 0 outside the frame.  Covariance and variance do not change under a shift, and the moments of the
//      shifted values are small where the picture is smooth, which is where M(g P) - M(g) M(P) cancels worst in float32.
//   2  row sums, LDS -> LDS: for every staged row and tile column the sums over [x - r, x + r] of the eight moments g, g^2, P_c, g P_c.
//   3  column sums of those, the division by the number of pixels of the window inside the frame, a_c and b_c (the anchors added back),
//      stored as six planes [6][H][W] per frame.
// gf_apply_k: one workgroup of 256 threads owns GF_AT_H x p.tw delivered pixels of one frame.
//   1  stage the six planes over the working rows and columns the tile's taps span, plus r on every side (0 outside the frame)
//   2  row sums, 3 column sums and the division: the means A_c, B_c of the spanned working pixels, in LDS
//   4  per delivered pixel: the six planes resampled from LDS (within each working row first, taps ascending, then across rows, fmaf from -0 as
//      deliver_k does), g_hi from the pixel of X_hi, Q_c = fmaf(up(A_c), g_hi, up(B_c)), stored as 12 contiguous bytes per lane.
// Every window sum adds its terms in ascending order in float32.  Reads are bounded by the frame tests of the stages and by the tap tables
// (first + count <= S, built by the host); a tap beyond what the LDS holds (p.sy, p.sx: sized by the host to the largest span) is left out.
#include "guided.h"

__device__ __forceinline__ float gf_luma(float b, float g, float r) {
#pragma clang fp contract(off)
    return (0.114f * b + 0.587f * g) + 0.299f * r;
}
// i / n and i % n for 0 <= i < 2^22 and a divisor known only at run time (inv = 1.0f / n): a multiplication and one correction step either
// way, in place of the forty-odd instructions of an integer division per staged element
__device__ __forceinline__ int gf_div(int i, int n, float inv, int* rem) {
    int q = (int)((float)i * inv);
    int r = i - q * n;
    if (r >= n) { ++q; r -= n; }
    if (r < 0) { --q; r += n; }
    *rem = r;
    return q;
}
__device__ __forceinline__ int gf_count(int v, int r, int n) { return min(v + r, n - 1) - max(v - r, 0) + 1; }      // samples of [v - r, v + r] inside 0..n-1

__global__ __launch_bounds__(256) void gf_coeff_k(const GuidedP p) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int r = p.r, RR = GF_CT_H + 2 * r, CC = GF_CT_W + 2 * r, win = 2 * r + 1;
    float* const s_in = s_dyn;                            // [4][RR][CC]: g, P_B, P_G, P_R, anchored
    float* const s_row = s_dyn + (size_t)4 * RR * CC;     // [8][RR][GF_CT_W]: row sums of g, g^2, P_c, g P_c
    const int tid = threadIdx.x;
    const int tiles_x = (p.W + GF_CT_W - 1) / GF_CT_W, tiles_y = (p.H + GF_CT_H - 1) / GF_CT_H;
    int bx = blockIdx.x;
    const int tx = bx % tiles_x;
    bx /= tiles_x;
    const int ty = bx % tiles_y;
    const int b = bx / tiles_y;
    const int y0 = ty * GF_CT_H, x0 = tx * GF_CT_W;
    const size_t frame = (size_t)b * (size_t)p.H * (size_t)p.W;
    const float* const P = p.P + frame * 3;
    const float* const X = p.xlo + frame * 3;

    float anc[4];      // the anchors: g and P_c at the tile's centre pixel (inside the frame)
    {
        const size_t at = ((size_t)min(y0 + GF_CT_H / 2, p.H - 1) * (size_t)p.W + (size_t)min(x0 + GF_CT_W / 2, p.W - 1)) * 3;
        anc[0] = gf_luma(X[at], X[at + 1], X[at + 2]);
        anc[1] = P[at]; anc[2] = P[at + 1]; anc[3] = P[at + 2];
    }
    const float inv_cc = 1.0f / (float)CC;
    for (int i = tid; i < RR * CC; i += 256) {
        int cc;
        const int rr = gf_div(i, CC, inv_cc, &cc);
        const int y = y0 - r + rr, x = x0 - r + cc;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
            const size_t at = ((size_t)y * (size_t)p.W + (size_t)x) * 3;
            v[0] = gf_luma(X[at], X[at + 1], X[at + 2]) - anc[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[1 + k] = P[at + k] - anc[1 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_in[(size_t)k * RR * CC + i] = v[k];
    }
    __syncthreads();
    for (int i = tid; i < RR * GF_CT_W; i += 256) {
        const int rr = i / GF_CT_W, c = i - rr * GF_CT_W;
        const float* const s = s_in + rr * CC + c;
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < win; ++d) {
            const float g = s[d];
            m[0] += g;
            m[1] = fmaf(g, g, m[1]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v = s[(size_t)(1 + k) * RR * CC + d];
                m[2 + k] += v;
                m[5 + k] = fmaf(g, v, m[5 + k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s_row[(size_t)k * RR * GF_CT_W + i] = m[k];
    }
    __syncthreads();
    float* const ab = p.ab + frame * 6;
    const size_t plane = (size_t)p.H * (size_t)p.W;
    for (int i = tid; i < GF_CT_H * GF_CT_W; i += 256) {
        const int rl = i / GF_CT_W, c = i - rl * GF_CT_W;
        const int y = y0 + rl, x = x0 + c;
        if (y >= p.H || x >= p.W) continue;
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < win; ++d) {
#pragma unroll
            for (int k = 0; k < 8; ++k) m[k] += s_row[((size_t)k * RR + rl + d) * GF_CT_W + c];
        }
        const float n = (float)(gf_count(y, r, p.H) * gf_count(x, r, p.W));
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] /= n;
        const float var = fmaxf(m[1] - m[0] * m[0], 0.f);
        const size_t at = (size_t)y * (size_t)p.W + (size_t)x;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = (m[5 + k] - m[0] * m[2 + k]) / (var + p.e);
            ab[(size_t)k * plane + at] = a;
            ab[(size_t)(3 + k) * plane + at] = (m[2 + k] + anc[1 + k]) - a * (m[0] + anc[0]);
        }
    }
}

__global__ __launch_bounds__(256) void gf_apply_k(const GuidedP p) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int r = p.r, RR = p.sy + 2 * r, CC = p.sx + 2 * r, win = 2 * r + 1;
    float* const s_in = s_dyn;                            // [6][RR][CC] the staged planes; from the column sums on [6][p.sy][p.sx], their means
    float* const s_row = s_dyn + (size_t)6 * RR * CC;     // [6][RR][p.sx] row sums
    const int tid = threadIdx.x;
    const int tiles_x = (p.DW + p.tw - 1) / p.tw, tiles_y = (p.DH + GF_AT_H - 1) / GF_AT_H;
    int bx = blockIdx.x;
    const int tx = bx % tiles_x;
    bx /= tiles_x;
    const int ty = bx % tiles_y;
    const int b = bx / tiles_y;
    const int ox0 = tx * p.tw, oy0 = ty * GF_AT_H;
    const int ncol = min(p.tw, p.DW - ox0), nrow = min(GF_AT_H, p.DH - oy0);
    // the working rows and columns the tile's taps span (first is non-decreasing), never more than the LDS holds
    const int r0y = p.ay.first[oy0], r0x = p.ax.first[ox0];
    const int ny = min(p.ay.first[oy0 + nrow - 1] + p.ay.count[oy0 + nrow - 1] - r0y, p.sy);
    const int nx = min(p.ax.first[ox0 + ncol - 1] + p.ax.count[ox0 + ncol - 1] - r0x, p.sx);
    const int sr = ny + 2 * r, sc = nx + 2 * r;      // staged rows and columns
    const size_t plane = (size_t)p.H * (size_t)p.W;
    const float* const ab = p.ab + (size_t)b * 6 * plane;

    const float inv_sc = 1.0f / (float)sc, inv_nx = 1.0f / (float)nx, inv_sr = 1.0f / (float)sr, inv_ny = 1.0f / (float)ny;
    for (int i = tid; i < 6 * sr * sc; i += 256) {      // row = (plane, staged row)
        int cc;
        const int row = gf_div(i, sc, inv_sc, &cc);
        int rr;
        const int k = gf_div(row, sr, inv_sr, &rr);
        const int y = r0y - r + rr, x = r0x - r + cc;
        float v = 0.f;
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) v = ab[(size_t)k * plane + (size_t)y * (size_t)p.W + (size_t)x];
        s_in[((size_t)k * RR + rr) * CC + cc] = v;
    }
    __syncthreads();
    for (int i = tid; i < 6 * sr * nx; i += 256) {
        int c;
        const int row = gf_div(i, nx, inv_nx, &c);
        int rr;
        const int k = gf_div(row, sr, inv_sr, &rr);
        const float* const s = s_in + ((size_t)k * RR + rr) * CC + c;
        float m = 0.f;
        for (int d = 0; d < win; ++d) m += s[d];
        s_row[((size_t)k * RR + rr) * p.sx + c] = m;
    }
    __syncthreads();
    float* const s_mean = s_in;      // (the staged planes have been read)
    for (int i = tid; i < 6 * ny * nx; i += 256) {
        int c;
        const int row = gf_div(i, nx, inv_nx, &c);
        int yy;
        const int k = gf_div(row, ny, inv_ny, &yy);
        float m = 0.f;
        for (int d = 0; d < win; ++d) m += s_row[((size_t)k * RR + yy + d) * p.sx + c];
        s_mean[((size_t)k * p.sy + yy) * p.sx + c] = m / (float)(gf_count(r0y + yy, r, p.H) * gf_count(r0x + c, r, p.W));
    }
    __syncthreads();
    const size_t dframe = (size_t)b * (size_t)p.DH * (size_t)p.DW * 3;
    const int tw_shift = 31 - __builtin_clz(p.tw);      // (p.tw is a power of two)
    for (int i = tid; i < (nrow << tw_shift); i += 256) {
        const int rl = i >> tw_shift, c = i & (p.tw - 1);
        if (c >= ncol) continue;
        const int oy = oy0 + rl, ox = ox0 + c;
        // An upscale has one or two taps per sample and axis.  Both are taken, a missing second one (or one beyond what the LDS holds) with
        // weight 0 at the first one's place: adding 0 x a finite value changes no sum.
        const int fy = min(p.ay.first[oy] - r0y, ny - 1), fx = min(p.ax.first[ox] - r0x, nx - 1);      // (the min: never beyond the means, whatever the tables hold)
        const bool y2 = p.ay.count[oy] > 1 && fy + 1 < ny, x2 = p.ax.count[ox] > 1 && fx + 1 < nx;
        const float wy0 = p.ay.w[(size_t)oy * RS_TAPS], wy1 = y2 ? p.ay.w[(size_t)oy * RS_TAPS + 1] : 0.f;
        const float wx0 = p.ax.w[(size_t)ox * RS_TAPS], wx1 = x2 ? p.ax.w[(size_t)ox * RS_TAPS + 1] : 0.f;
        const int at0 = fy * p.sx + fx, dy = y2 ? p.sx : 0, dx = x2 ? 1 : 0;
        float up[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float* const s = s_mean + (size_t)k * p.sy * p.sx + at0;
            const float h0 = fmaf(wx1, s[dx], fmaf(wx0, s[0], -0.f));      // -0 + x == x for every x, -0 included
            const float h1 = fmaf(wx1, s[dy + dx], fmaf(wx0, s[dy], -0.f));
            up[k] = fmaf(wy1, h1, fmaf(wy0, h0, -0.f));
        }
        const size_t at = dframe + ((size_t)oy * (size_t)p.DW + (size_t)ox) * 3;
        const float g = gf_luma(p.xhi[at], p.xhi[at + 1], p.xhi[at + 2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) p.q[at + k] = fmaf(up[k], g, up[3 + k]);
    }
}

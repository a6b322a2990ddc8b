// compose_k.h — the compositing stage (include/rerevst_hip.h "Compositing"), gfx950; part of compose.hip (librerevst_compose.so).
//
// composite_k<MATTE>: pointwise and bandwidth bound (24 B read and 12 B written per pixel, plus 0, 4 or 1 B of matte).  The B frames are one
// flat run of n_px = B * frame_px pixels, cut into groups of 4 consecutive pixels (48 bytes of each frame buffer); a thread takes group
// blockIdx.x * 256 + threadIdx.x and then every (gridDim.x * 256)-th one after it.  A full group of 16-byte aligned buffers (p.vec) moves as
// three 16-byte loads from each of P and S and three 16-byte stores; the last group of the run when n_px is not a multiple of 4, and every
// group of buffers that are only element aligned, moves element by element.  Both ways feed the same arithmetic, so the bits are the same.
//   The frame and the in-frame index of a group's first pixel are kept incrementally: one 32-bit division in front of the loop (a thread's
// first pixel lies below 2^23), then a step of p.step_q frames and p.step_r pixels.  When frame_px is not a multiple of 4 a group straddles
// frames (when frame_px < 4, several), so the strength and the matte index are per PIXEL of the group.  A group's four matte values are
// one load (p.mvec) when they are consecutive and aligned: a matte per frame is indexed by the flat pixel, a shared one by the in-frame
// index, which is then a multiple of 4 only if frame_px is.
//   out may be P: a thread reads all of a group before it writes any of it, and no other thread touches that group.  Every offset is a
// size_t (64 frames of 2160p are 6.4e9 bytes per buffer).  Every operation is rounded to float32, none contracted.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "compose.h"

template <int MATTE>
__global__ __launch_bounds__(256) void composite_k(const ComposeP p) {
#pragma clang fp contract(off)
    const size_t fp = p.frame_px, n = p.n_px;
    const size_t groups = (n + 3) / 4, gstep = (size_t)gridDim.x * 256;
    size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    // group g's first pixel: frame `frame`, pixel `rem` of it
    size_t rem = 4 * g;
    unsigned frame = 0;
    if (rem >= fp) {      // (then fp <= rem < 2^23)
        frame = (unsigned)rem / (unsigned)fp;
        rem -= (size_t)frame * fp;
    }
    const bool shared = p.matte_frames == 1;
    for (; g < groups; g += gstep) {
        const size_t pix = 4 * g;
        const int cnt = n - pix < 4 ? (int)(n - pix) : 4;
        const bool full = cnt == 4;

        // ---- alpha of the group's pixels
        float alpha[4];
        size_t mi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            alpha[j] = 0.f; mi[j] = 0;
            if (j < cnt) {
                size_t r = rem + j;
                unsigned f = frame;
                while (r >= fp) { r -= fp; ++f; }
                alpha[j] = p.strength[f];      // (f < p.B: the pixel exists)
                mi[j] = shared ? r : pix + j;
            }
        }
        if constexpr (MATTE == CM_F32) {
            const float* const m = (const float*)p.matte;
            float mv[4] = {0.f, 0.f, 0.f, 0.f};
            if (full && p.mvec) {
                const float4 v = *reinterpret_cast<const float4*>(m + mi[0]);
                mv[0] = v.x; mv[1] = v.y; mv[2] = v.z; mv[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < cnt) mv[j] = m[mi[j]];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) alpha[j] = alpha[j] * mv[j];
        } else if constexpr (MATTE == CM_U8) {
            const uint8_t* const m = (const uint8_t*)p.matte;
            unsigned mv[4] = {0u, 0u, 0u, 0u};
            if (full && p.mvec) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(m + mi[0]);
                mv[0] = v & 255u; mv[1] = (v >> 8) & 255u; mv[2] = (v >> 16) & 255u; mv[3] = v >> 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < cnt) mv[j] = m[mi[j]];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) alpha[j] = alpha[j] * ((float)mv[j] / 255.0f);
        }

        // ---- the group's 12 values of P and S
        const float* const pp = p.P + pix * 3;
        const float* const ps = p.S + pix * 3;
        float* const po = p.out + pix * 3;
        float vp[12], vs[12], vo[12];
        const bool vec = full && p.vec;
        if (vec) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 a = reinterpret_cast<const float4*>(pp)[k], b = reinterpret_cast<const float4*>(ps)[k];
                vp[4 * k] = a.x; vp[4 * k + 1] = a.y; vp[4 * k + 2] = a.z; vp[4 * k + 3] = a.w;
                vs[4 * k] = b.x; vs[4 * k + 1] = b.y; vs[4 * k + 2] = b.z; vs[4 * k + 3] = b.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                vp[e] = 0.f; vs[e] = 0.f;
                if (e < 3 * cnt) { vp[e] = pp[e]; vs[e] = ps[e]; }
            }
        }

        // ---- the arithmetic, pixel by pixel (B, G, R)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* const P = vp + 3 * j;
            const float* const S = vs + 3 * j;
            float C[3] = {P[0], P[1], P[2]};
            if (p.keep != CK_NONE) {
                const float gp = (0.114f * P[0] + 0.587f * P[1]) + 0.299f * P[2];
                const float gs = (0.114f * S[0] + 0.587f * S[1]) + 0.299f * S[2];
                if (p.keep == CK_COLOUR) {
                    const float d = gp - gs;
#pragma unroll
                    for (int c = 0; c < 3; ++c) C[c] = S[c] + d;
                } else {
                    const float d = gs - gp;
#pragma unroll
                    for (int c = 0; c < 3; ++c) C[c] = P[c] + d;
                }
            }
            const float a = alpha[j], na = 1.0f - a;
#pragma unroll
            for (int c = 0; c < 3; ++c) vo[3 * j + c] = na * S[c] + a * C[c];
        }

        if (vec) {
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<float4*>(po)[k] = make_float4(vo[4 * k], vo[4 * k + 1], vo[4 * k + 2], vo[4 * k + 3]);
        } else {
#pragma unroll
            for (int e = 0; e < 12; ++e) if (e < 3 * cnt) po[e] = vo[e];
        }

        rem += p.step_r; frame += (unsigned)p.step_q;
        if (rem >= fp) { rem -= fp; ++frame; }
    }
}

// guided.h — parameters and the launch entry of the guided delivery stage (include/rerevst_hip.h "Guided delivery"; librerevst_stages.so).
//
// Two kernels (guided_k.h) turn B stylized working frames P [H][W][3] and the source at both sizes, X_lo [H][W][3] and X_hi [DH][DW][3] (all
// contiguous float32 BGR PIXEL), into the frames Q [DH][DW][3] of the same form:
//   gf_coeff_k   the local linear model stylized = a * luma + b of every working pixel: ab [B][6][H][W], planes a_B a_G a_R b_B b_G b_R
//   gf_apply_k   box mean of the six planes, resampled H x W -> DH x DW with the delivery stage's tap tables, applied to the luma of X_hi
// This header is all the main library sees of them.
#pragma once
#include "resample.h"   // RsAxis, RS_TAPS

constexpr int GF_R_MAX = 16;              // the largest radius, in working pixels
constexpr int GF_CT_H = 16, GF_CT_W = 32; // gf_coeff_k: working pixels per tile
constexpr int GF_AT_H = 16;               // gf_apply_k: delivered rows per tile; its columns per tile are GuidedP::tw (64, 32, 16 or 8)
constexpr size_t GF_LDS_MAX = 152 * 1024; // dynamic LDS a launch may ask for (160 KB per CU)

struct GuidedP {
    const float* P;       // [B][H][W][3] the stylized working frames
    const float* xlo;     // [B][H][W][3] the source at the working size
    const float* xhi;     // [B][DH][DW][3] the source at the delivered size
    float* ab;            // [B][6][H][W] workspace: the coefficient planes
    float* q;             // [B][DH][DW][3] the result
    int H, W, B;          // working frame
    int DH, DW;           // delivered frame (DH >= H, DW >= W: at most two taps per sample and axis)
    int r;                // box radius in working pixels, 1..GF_R_MAX
    float e;              // eps * 65025
    RsAxis ay, ax;        // vertical (H -> DH) and horizontal (W -> DW) tables
    int tw;               // gf_apply_k: delivered columns per tile
    int sy, sx;           // gf_apply_k: working rows / columns the LDS holds for a tile's taps (the kernel stages no more)
};

// working samples that T consecutive delivered samples' taps span at most, S -> D with D >= S: first(i) = max(floor(s (i + 0.5) - 0.5), 0),
// one or two taps each, so last(i0 + T - 1) - first(i0) + 1 <= floor(s (T - 1)) + 3
inline int guided_span(int S, int D, int T) {
    const long long v = (long long)(T - 1) * S / D + 3;
    return (int)(v < S ? v : S);
}
// the dynamic LDS of the two kernels
inline size_t guided_coeff_lds_bytes(int r) {      // staged g, P_c: [4][TH + 2r][TW + 2r]; row sums of the eight moments: [8][TH + 2r][TW]
    return ((size_t)4 * (GF_CT_H + 2 * r) * (GF_CT_W + 2 * r) + (size_t)8 * (GF_CT_H + 2 * r) * GF_CT_W) * sizeof(float);
}
inline size_t guided_apply_lds_bytes(int r, int sy, int sx) {      // staged a, b: [6][sy + 2r][sx + 2r] (then their means [6][sy][sx]); row sums: [6][sy + 2r][sx]
    return ((size_t)6 * (sy + 2 * r) * (sx + 2 * r) + (size_t)6 * (sy + 2 * r) * sx) * sizeof(float);
}
// Fills tw, sy, sx of `p` from its sizes and radius: the widest tile whose LDS fits.  False: none does (cannot happen for r <= GF_R_MAX).
// Within r <= GF_R_MAX only 64 and 32 are ever chosen (sy <= 18 and sx <= 34 at tw = 32: 120,000 bytes at r = 16); the 16 and 8 of the loop
// are never reached and stay as the margin of a larger radius (tests/test_guided_host.py sweeps the rule through rrv_guided_tile).
inline bool guided_tile(GuidedP* p) {
    p->sy = guided_span(p->H, p->DH, GF_AT_H);
    for (int tw = 64; tw >= 8; tw >>= 1) {
        p->tw = tw;
        p->sx = guided_span(p->W, p->DW, tw);
        if (guided_apply_lds_bytes(p->r, p->sy, p->sx) <= GF_LDS_MAX) return true;
    }
    return false;
}

// Queues gf_coeff_k (grid tiles of GF_CT_H x GF_CT_W working pixels x B) and gf_apply_k (grid tiles of GF_AT_H x tw delivered pixels x B) on
// `stream`, 256 threads each.  Returns the hipError_t of the launches as an int (0 = queued).
extern "C" int rrv_guided_launch(const GuidedP* p, void* stream);

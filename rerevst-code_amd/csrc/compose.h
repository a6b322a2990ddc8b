// compose.h — parameters and the launch entry of the compositing stage behind the delivery stage (librerevst_compose.so).
//
// composite_k<MATTE> (compose_k.h) mixes B contiguous float32 [DH][DW][3] BGR PIXEL frames P (the stylized frame at the delivered size) with
// the source S of the same form and size: include/rerevst_hip.h "Compositing".  This header is all the main library sees of the kernels.
#pragma once
#include <cstddef>

// the matte kinds, one composite_k instantiation each
enum : int { CM_NONE = 0, CM_F32 = 1, CM_U8 = 2, CM_FORMS = 3 };
enum : int { CK_NONE = 0, CK_COLOUR = 1, CK_LUMA = 2 };      // RRV_KEEP_*
constexpr int CM_B_MAX = 64;                // frames per launch (the strengths travel by value)
constexpr unsigned CM_GRID_MAX = 2048;      // workgroups of 256 threads, 4 pixels per thread and step; the rest is grid-strided

struct ComposeP {
    const float* P;            // [B][DH][DW][3] stylized
    const float* S;            // [B][DH][DW][3] source
    const void* matte;         // CM_F32: float32, CM_U8: uint8; [matte_frames][DH][DW], contiguous
    float* out;                // [B][DH][DW][3]; may be P
    size_t frame_px;           // DH * DW
    int B;
    int matte_frames;          // 1 (one matte for every frame) or B
    int keep;                  // CK_*
    float strength[CM_B_MAX];  // per frame
    // filled by rrv_compose_launch
    size_t n_px;               // B * frame_px
    size_t step_q, step_r;     // a grid step of grid * 1024 pixels, in whole frames and the pixels beyond them
    int vec;                   // P, S and out are 16-byte aligned: 16-byte loads and stores
    int mvec;                  // a group's four matte values are one aligned load
};

// The launch rule: one thread per group of 4 pixels of the flat run of n_px pixels, 256 threads per workgroup, at most CM_GRID_MAX workgroups.
inline unsigned compose_grid(size_t n_px) {
    const size_t blocks = (n_px + 1023) / 1024;
    return blocks < 1 ? 1u : blocks > CM_GRID_MAX ? CM_GRID_MAX : (unsigned)blocks;
}

// Queues composite_k<form> on `stream`: grid compose_grid(B * frame_px), 256 threads.  Returns the hipError_t of the launch as an int (0 = queued).
extern "C" int rrv_compose_launch(const ComposeP* p, int form, void* stream);

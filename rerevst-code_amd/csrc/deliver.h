// deliver.h — parameters and the launch entry of the output-side resampler behind the last kernel (librerevst_stages.so).
//
// deliver_k<OUT> (deliver_k.h) reads B contiguous float32 [H][W][3] BGR PIXEL frames (what conv_last_k<false> stores, crop applied),
// resamples them to DH x DW with the input resampler's arithmetic and tap tables (rrv_resample_taps, (H -> DH) and (W -> DW)), and
// writes the result through an ImgView in one of conv_last_k's output forms.  This header is all the main library sees of the kernels.
#pragma once
#include "resample.h"   // RS_* tile and tap constants, RsAxis; conv_thin.h: SP_* spaces, ImgView

// the output forms, one deliver_k instantiation each
enum : int { DL_F32_HWC = 0, DL_F32_CHW = 1, DL_U8_HWC = 2, DL_U8_CHW = 3, DL_YUV8 = 4, DL_YUV16 = 5, DL_FORMS = 6 };

struct DeliverP {
    const float* in;      // [B][H][W][3] float32 BGR PIXEL, contiguous: the working frames
    int H, W, B;          // working frame
    int DH, DW;           // delivered frame
    void* out;            // frame b's planes through `v`, as LastP::out_img
    ImgView v;            // where the DELIVERED frame's rows are, in elements of its type
    RsAxis ay, ax;        // vertical (H -> DH) and horizontal (W -> DW) tables
    int tiles_x, tiles_y; // tiles of RS_TH x RS_TW delivered pixels per frame
    int rows;             // working rows the LDS holds: the largest span of a tile's vertical taps (<= RS_ROWS_MAX)
    int space;            // DL_F32_*: value space of the output (SP_*)
    int nv12;             // DL_YUV*: semi-planar (interleaved CbCr rows) rather than planar
    int csx, csy;         // DL_YUV*: the chroma shifts
    float yuv_hi;         // DL_YUV16: the largest code (LastP::yuv_hi)
    int yuv_shift;        // DL_YUV16: LastP::yuv_shift
    float yuv_m[12];      // DL_YUV*: LastP::yuv_m, by value
};

// the dynamic LDS: the staged working rows [rows][RS_TW][3] and the tile of resampled values [RS_TH][RS_TW][3]
inline size_t deliver_lds_bytes(int rows) { return (size_t)(rows + RS_TH) * RS_TW * 3 * sizeof(float); }

// Queues deliver_k<form> on `stream`: grid tiles_x * tiles_y * B, 256 threads.  Returns the hipError_t of the launch as an int (0 = queued).
extern "C" int rrv_deliver_launch(const DeliverP* p, int form, void* stream);

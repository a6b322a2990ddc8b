// resample.h — parameters and the launch entry of the antialiased resampler in front of the first kernel (librerevst_stages.so).
//
// resample_k<IN> (resample_k.h) reads B source frames of SH x SW pixels in any of conv_first_k's eight input forms, through the same ImgView,
// and writes contiguous [B][H][W][3] float32 BGR PIXEL frames: a separable triangle filter whose per-axis tap tables the host builds
// (rrv_resample_taps: first source sample, tap count and normalised float32 weights per output sample, at most RS_TAPS taps).
// This header is all the main library sees of the kernels.
#pragma once
#include "conv_thin.h"   // IN_* forms, SP_* spaces, ImgView

constexpr int RS_TAPS = 16;       // taps per output sample and axis: ratios up to 8 give 2 x 8
constexpr int RS_TW = 64;         // output columns per tile
constexpr int RS_TH = 16;         // output rows per tile
constexpr int RS_ROWS_MAX = 8 * (RS_TH - 1) + 2 * 8;      // source rows a tile's vertical taps span at ratio 8: 136

// The tap tables of one axis in HBM: first[D], count[D], w[D][RS_TAPS] (weights beyond count are 0).
struct RsAxis { const int* first; const int* count; const float* w; };

struct ResampleP {
    const void* img;      // frame b's planes through `v`, as FirstP::img
    ImgView v;            // where the SOURCE frame's rows are, in elements of its type
    int SH, SW;           // source frame
    int H, W, B;          // output frames
    float* out;           // [B][H][W][3] float32 BGR PIXEL, contiguous
    RsAxis ay, ax;        // vertical (SH -> H) and horizontal (SW -> W) tables
    int tiles_x, tiles_y; // tiles of RS_TH x RS_TW output pixels per frame
    int rows;             // source rows the LDS holds: the largest span of a tile's vertical taps (<= RS_ROWS_MAX)
    int space;            // value space of a float32 input (SP_*)
    float yuv_n[12];      // IN_YUV_*: FirstP::yuv_n
    int yuv_shift;        // IN_YUV_*: FirstP::yuv_shift
    int csx, csy;         // IN_YUV_*: the chroma shifts
};

inline size_t resample_lds_bytes(int rows) { return (size_t)rows * RS_TW * 3 * sizeof(float); }      // the dynamic part: [rows][RS_TW][3]

// Queues resample_k<form> on `stream`: grid tiles_x * tiles_y * B, 256 threads.  Returns the hipError_t of the launch as an int (0 = queued).
extern "C" int rrv_scale_launch(const ResampleP* p, int form, void* stream);

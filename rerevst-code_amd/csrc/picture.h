// picture.h — parameters and the launch entry of the line profile (librerevst_picture.so; include/rerevst_hip.h "Picture area").
//
// picture_lines_k / picture_cols_k (picture_k.h) read B contiguous float32 [H][W][3] BGR PIXEL frames (what the input resampler writes) and
// write uint32 prof[B][H + W]: per frame the number of lit pixels of every row, then of every column, in integers from the rounding on.
// This header is all the main library sees of the kernels.
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int PC_B_MAX = 64;          // frames per launch
constexpr int PC_MIN = 8;             // H, W at least
constexpr int PC_STRIP = 32;          // rows of a frame one workgroup of picture_lines_k takes
constexpr int PC_T_MAX = 254;         // the threshold lies in 0..254: at 255 no pixel could be lit

struct PictureP {
    const float* in;      // [B][H][W][3]
    uint32_t* prof;       // [B][H + W]: row_cnt[H], col_cnt[W]; every word is written, none is read
    uint32_t* part;       // [B][strips][W] scratch: every word is written by picture_lines_k before picture_cols_k reads it
    int B, H, W, threshold;
};

inline int pc_strips(int H) { return (H + PC_STRIP - 1) / PC_STRIP; }
// uint32 words of the scratch a launch of B frames of H x W needs
inline size_t pc_part_words(int B, int H, int W) { return (size_t)B * (size_t)pc_strips(H) * (size_t)W; }

// Queues picture_lines_k (grid B * strips, 256 threads) and picture_cols_k (grid B * ceil(W / 256), 256 threads) on `stream`.  The 16-byte
// loads are taken where every row keeps that alignment (W a multiple of 4 and `in` 16-byte aligned), else the dword loads.  Returns the
// hipError_t of the launches as an int (0 = queued); hipErrorInvalidValue for a null buffer, B outside 1..PC_B_MAX, H, W below PC_MIN or a
// threshold outside 0..PC_T_MAX.
extern "C" int rrv_picture_launch(const PictureP* p, void* stream);

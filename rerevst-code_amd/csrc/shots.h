// shots.h — parameters and the launch entry of the shot signature (librerevst_shots.so; include/rerevst_hip.h "Shots").
//
// shot_sig_k (shots_k.h) reads B contiguous float32 [H][W][3] BGR PIXEL frames (what the input resampler writes) and writes
// uint32 sig[B][16][32]: a 32-bin luma histogram for each cell of a 4 x 4 grid, in integers from the first step on.  This header is all the
// main library sees of the kernel.
#pragma once
#include <cstdint>

constexpr int SG_GRID = 4;                        // cells per axis
constexpr int SG_CELLS = SG_GRID * SG_GRID;       // 16 per frame
constexpr int SG_BINS = 32;                       // luma bins per cell: Y >> 3
constexpr int SG_WORDS = SG_CELLS * SG_BINS;      // 512 uint32 per frame
constexpr int SG_B_MAX = 64;                      // frames per launch
constexpr int SG_MIN = 4;                         // H, W at least: every cell holds a pixel

struct ShotsP {
    const float* in;      // [B][H][W][3]
    uint32_t* sig;        // [B][16][32]; every word is written, none is read
    int B, H, W;
};

// Rows (columns) of cell c of an axis of n pixels: [sg_lo(c, n), sg_lo(c + 1, n)), the pixels y with (4 * y) / n == c.
inline __host__ __device__ int sg_lo(int c, int n) { return (int)(((long long)c * n + SG_GRID - 1) / SG_GRID); }

// Queues shot_sig_k on `stream`: grid B * 16 (one workgroup per frame and cell), 256 threads.  Returns the hipError_t of the launch as an int
// (0 = queued); hipErrorInvalidValue for a null buffer, B outside 1..SG_B_MAX or H, W below SG_MIN.
extern "C" int rrv_shots_launch(const ShotsP* p, void* stream);

// rs_tile.h — the tile skeleton resample_k<IN> and deliver_k<OUT> share: one workgroup of 256 threads resamples a tile of RS_TH x RS_TW
// destination pixels of one frame through LDS.
//   rs_tile_open   the tile of this workgroup, its part of both axes' tap tables staged in LDS, and the source rows its vertical taps span
//   rs_tile_rows   horizontal pass, source -> LDS: for each of those rows and each of the tile's columns, sum_j wx[j] * pixel(row, first_x + j)
//                  for the three BGR channels into s_rows [rows][RS_TW][3]; `pixel` is all a kernel says about where its source lies
//   rs_tile_cols   vertical pass, LDS -> sink: consecutive threads take consecutive floats of a tile row and hand each sum to `sink`
// Both passes accumulate in float32 with fmaf from -0, taps in ascending order.  The host's device tables hold no tap of weight 0 (a trailing
// one is dropped from the count), so an identity row is the one tap {1} and returns the source value bit for bit, -0 and non-finite values
// included, whatever the neighbouring sample holds.  Reads are bounded by the tap tables (first + count <= S on both axes, built by the host).
// The caller puts a __syncthreads() between the passes.
#pragma once
#include "resample.h"

struct RsTaps {                        // a tile's tap tables in LDS
    float wx[RS_TAPS * RS_TW];         // [tap][column]: lanes of a wave read consecutive banks
    int fx[RS_TW], nx[RS_TW];
    float wy[RS_TH * RS_TAPS];         // [row][tap]
    int fy[RS_TH], ny[RS_TH];
};
struct RsTile {
    int b;               // the frame
    int ox0, oy0;        // the tile's first destination column and row
    int ncol, nrow;      // its valid columns and rows
    int r0, nsrc;        // the first source row its vertical taps touch, and how many are staged
};

// H x W: the destination frame; rows: the source rows the LDS holds (the host sized it as the largest nsrc of any tile)
__device__ __forceinline__ RsTile rs_tile_open(RsTaps& s, const RsAxis& ay, const RsAxis& ax, int tiles_x, int tiles_y, int H, int W, int rows) {
    const int tid = threadIdx.x;
    RsTile t;
    int bx = blockIdx.x;
    const int tx = bx % tiles_x;
    bx /= tiles_x;
    const int ty = bx % tiles_y;
    t.b = bx / tiles_y;
    t.ox0 = tx * RS_TW; t.oy0 = ty * RS_TH;
    t.ncol = min(RS_TW, W - t.ox0); t.nrow = min(RS_TH, H - t.oy0);
    for (int i = tid; i < RS_TAPS * RS_TW; i += 256) {
        const int j = i / RS_TW, c = i - j * RS_TW;
        s.wx[i] = c < t.ncol ? ax.w[(size_t)(t.ox0 + c) * RS_TAPS + j] : 0.f;
    }
    if (tid < RS_TW) {
        s.fx[tid] = tid < t.ncol ? ax.first[t.ox0 + tid] : 0;
        s.nx[tid] = tid < t.ncol ? ax.count[t.ox0 + tid] : 0;
    }
    {
        const int r = tid / RS_TAPS;      // 256 = RS_TH * RS_TAPS
        s.wy[tid] = r < t.nrow ? ay.w[(size_t)(t.oy0 + r) * RS_TAPS + (tid - r * RS_TAPS)] : 0.f;
    }
    if (tid < RS_TH) {
        s.fy[tid] = tid < t.nrow ? ay.first[t.oy0 + tid] : 0;
        s.ny[tid] = tid < t.nrow ? ay.count[t.oy0 + tid] : 0;
    }
    __syncthreads();
    t.r0 = s.fy[0];                                                       // (first is non-decreasing)
    t.nsrc = min(s.fy[t.nrow - 1] + s.ny[t.nrow - 1] - t.r0, rows);
    return t;
}

// pixel(y, x, o): the source pixel (y, x) of frame t.b as three float32 BGR values.  thread = (column, row mod 4)
template <class Pixel>
__device__ __forceinline__ void rs_tile_rows(const RsTaps& s, const RsTile& t, float* s_rows, Pixel pixel) {
    const int tid = threadIdx.x, col = tid & (RS_TW - 1);
    if (col >= t.ncol) return;
    const int fx = s.fx[col], nx = s.nx[col];
    for (int r = tid / RS_TW; r < t.nsrc; r += 256 / RS_TW) {
        float acc[3] = {-0.f, -0.f, -0.f};      // -0 + x == x for every x, -0 included
        for (int j = 0; j < nx; ++j) {
            const float w = s.wx[j * RS_TW + col];
            float px[3];
            pixel(t.r0 + r, fx + j, px);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = fmaf(w, px[k], acc[k]);
        }
        float* const d = &s_rows[((size_t)r * RS_TW + col) * 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = acc[k];
    }
}

// sink(r, e, v): v is float e (column e / 3, channel e % 3, BGR) of the tile's row r; called for the tile's valid rows and columns only
template <class Sink>
__device__ __forceinline__ void rs_tile_cols(const RsTaps& s, const RsTile& t, const float* s_rows, Sink sink) {
    const int row_floats = t.ncol * 3;
    for (int i = threadIdx.x; i < t.nrow * RS_TW * 3; i += 256) {
        const int r = i / (RS_TW * 3), e = i - r * (RS_TW * 3);
        if (e >= row_floats) continue;
        const int f = s.fy[r] - t.r0, n = s.ny[r];
        float acc = -0.f;
        for (int j = 0; j < n; ++j) {
            const int sr = f + j;
            if (sr < t.nsrc) acc = fmaf(s.wy[r * RS_TAPS + j], s_rows[(size_t)sr * (RS_TW * 3) + e], acc);
        }
        sink(r, e, acc);
    }
}

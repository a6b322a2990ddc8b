// shots_k.h — the shot signature (include/rerevst_hip.h "Shots"), gfx950; part of shots.hip (librerevst_shots.so).
//
// shot_sig_k: one 256-thread workgroup per (frame, cell) of the 4 x 4 grid.  Cell (cy, cx) holds the rows sg_lo(cy, H) .. sg_lo(cy + 1, H) - 1
// and the columns sg_lo(cx, W) .. sg_lo(cx + 1, W) - 1.  Wave w of the four takes the cell's rows w, w + 4, ..; its lanes run along x, 64
// pixels per step, so a step reads 768 consecutive bytes of the row with three dword loads per lane (the frames are thumbnails of about
// 1.5 MB: the kernel is a few microseconds of a detection pass that is bound by getting the frames to the GPU).
//   Per pixel, in integers: c8 = clamp(rint(v), 0, 255) per channel (half to even; NaN and everything not above 0 give 0, +inf gives 255),
// Y = (29 B8 + 150 G8 + 77 R8 + 128) >> 8, bin = Y >> 3.  Each wave counts into a 32-word histogram of its own in LDS with integer atomics
// whose result nobody reads (ds_add_u32; a constant frame sends all 64 lanes to one word, which the LDS serialises); behind a barrier
// threads 0..31 sum the four and store the cell's row.  No global atomic, no zeroing of the output: every output word is written once by one
// thread, so the result is deterministic and depends neither on B nor on what the buffer held.  Integer sums: no order of arrival shows.
//   Bounds: y < sg_lo(cy + 1, H) <= H and x < sg_lo(cx + 1, W) <= W, so the last float read is in[(b H W + (H - 1) W + W - 1) 3 + 2], the
// frame's last; the stores go to sig[(b 16 + cell) 32 + 0..31], cell < 16, b < B.  Offsets are size_t.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "shots.h"

__device__ __forceinline__ int shot_c8(float v) {
    const int r = __float2int_rn(fminf(v, 255.f));      // v > 0: rint half to even of min(v, 255), 1..255 or 0 (+inf: 255)
    return v > 0.f ? r : 0;                             // NaN, -inf, negatives, 0: !(v > 0) gives 0.  No branch: the three loads of a pixel issue together
}

__global__ __launch_bounds__(256) void shot_sig_k(const ShotsP p) {
    __shared__ unsigned hist[4][SG_BINS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x / SG_CELLS, cell = blockIdx.x % SG_CELLS, cy = cell / SG_GRID, cx = cell % SG_GRID;
    if (tid < 4 * SG_BINS) hist[tid >> 5][tid & 31] = 0u;
    __syncthreads();
    const int y0 = sg_lo(cy, p.H), y1 = sg_lo(cy + 1, p.H), x0 = sg_lo(cx, p.W), x1 = sg_lo(cx + 1, p.W);
    const float* const frame = p.in + (size_t)b * p.H * p.W * 3;
    for (int y = y0 + wave; y < y1; y += 4) {
        const float* const row = frame + (size_t)y * p.W * 3;
        for (int x = x0 + lane; x < x1; x += 64) {
            const float* const px = row + (size_t)x * 3;
            const int b8 = shot_c8(px[0]), g8 = shot_c8(px[1]), r8 = shot_c8(px[2]);
            const int Y = (29 * b8 + 150 * g8 + 77 * r8 + 128) >> 8;      // 0..255
            atomicAdd(&hist[wave][Y >> 3], 1u);
        }
    }
    __syncthreads();
    if (tid < SG_BINS)
        p.sig[((size_t)b * SG_CELLS + cell) * SG_BINS + tid] = (hist[0][tid] + hist[1][tid]) + (hist[2][tid] + hist[3][tid]);
}

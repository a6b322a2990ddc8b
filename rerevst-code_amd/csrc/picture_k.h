// picture_k.h — the line profile (include/rerevst_hip.h "Picture area"), gfx950; part of picture.hip (librerevst_picture.so).
//
// picture_lines_k<VEC>: one 256-thread workgroup per (frame, strip of PC_STRIP = 32 rows).  The strip is walked in steps of 64 * PX columns
// (PX = 4 pixels per lane with VEC, else 1); inside a step wave w of the four takes the strip's rows w, w + 4, .. and its lanes run along x.
// With VEC a lane reads its four pixels as three 16-byte loads (48 consecutive bytes per lane, 3 KB of the row per wave), which needs every
// row 16-byte aligned: W a multiple of 4 and an aligned base (rrv_picture_launch chooses).  Otherwise three dword loads per pixel.
//   Per pixel, in integers: c8 = clamp(rint(v), 0, 255) per channel (half to even; NaN and everything not above 0 give 0, +inf gives 255),
// Y = (29 B8 + 150 G8 + 77 R8 + 128) >> 8, lit = Y > threshold.
//   Rows: a wave's lit lanes are counted by ballot and popcount, and lane 0 adds the count to the row's word in LDS; a row belongs to one
// wave, so this is a plain add.  Columns: a lane keeps the counts of its PX columns over the wave's rows in registers; at the end of a step
// the four waves' counts meet in LDS and thread t stores the sum for column x0 + t of the step to the scratch part[b][strip][x].
// picture_cols_k then sums the strips of a column: one thread per (frame, column).
//   No global atomic, no zeroing of the output: every word of prof and of part is written exactly once by one thread, and part is written
// in full (every strip, every x < W) before picture_cols_k, queued behind on the same stream, reads it.  So the result is deterministic and
// depends neither on B nor on what the buffers held.  Integer sums: no order shows.
//   Bounds: rows y < min(y0 + 32, H), columns x < W (a lane beyond W loads nothing and is not lit; with VEC W is a multiple of 4, so a
// lane's four pixels are inside or outside together): the last float read is the frame's last.  Stores: prof[b (H + W) + y], y < H;
// part[(b strips + s) W + x], x < W; prof[b (H + W) + H + x], x < W.  Offsets are size_t.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "picture.h"

__device__ __forceinline__ int pic_c8(float v) {
    const int r = __float2int_rn(fminf(v, 255.f));      // v > 0: rint half to even of min(v, 255), 1..255 or 0 (+inf: 255)
    return v > 0.f ? r : 0;                             // NaN, -inf, negatives, 0: !(v > 0) gives 0
}
__device__ __forceinline__ bool pic_lit(float b, float g, float r, int threshold) {
    return ((29 * pic_c8(b) + 150 * pic_c8(g) + 77 * pic_c8(r) + 128) >> 8) > threshold;
}

template <int VEC>
__global__ __launch_bounds__(256) void picture_lines_k(const PictureP p) {
    constexpr int PX = VEC ? 4 : 1, STEP = 64 * PX;
    __shared__ unsigned colp[4][STEP];
    __shared__ unsigned rowc[PC_STRIP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = p.H, W = p.W, strips = (H + PC_STRIP - 1) / PC_STRIP;
    const int b = blockIdx.x / strips, s = blockIdx.x % strips;
    const int y0 = s * PC_STRIP, y1 = y0 + PC_STRIP < H ? y0 + PC_STRIP : H;
    if (tid < PC_STRIP) rowc[tid] = 0u;
    __syncthreads();
    const float* const frame = p.in + (size_t)b * H * W * 3;
    uint32_t* const part = p.part + ((size_t)b * strips + s) * W;
    for (int x0 = 0; x0 < W; x0 += STEP) {
        const int x = x0 + lane * PX;
        unsigned col[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) col[j] = 0u;
        for (int y = y0 + wave; y < y1; y += 4) {      // (uniform in the wave: the ballots below see all 64 lanes)
            const float* const px = frame + ((size_t)y * W + x) * 3;
            bool lit[PX];
            if constexpr (VEC != 0) {
                float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, v2 = v0;      // (a lane beyond W: zeros, lit at no threshold)
                if (x < W) {
                    const float4* const q = reinterpret_cast<const float4*>(px);
                    v0 = q[0]; v1 = q[1]; v2 = q[2];
                }
                lit[0] = pic_lit(v0.x, v0.y, v0.z, p.threshold);
                lit[1] = pic_lit(v0.w, v1.x, v1.y, p.threshold);
                lit[2] = pic_lit(v1.z, v1.w, v2.x, p.threshold);
                lit[3] = pic_lit(v2.y, v2.z, v2.w, p.threshold);
            } else {
                float vb = 0.f, vg = 0.f, vr = 0.f;
                if (x < W) { vb = px[0]; vg = px[1]; vr = px[2]; }
                lit[0] = x < W && pic_lit(vb, vg, vr, p.threshold);
            }
            unsigned cnt = 0u;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                cnt += (unsigned)__popcll(__ballot(lit[j]));
                col[j] += lit[j] ? 1u : 0u;
            }
            if (lane == 0) rowc[y - y0] += cnt;      // row y belongs to this wave alone
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) colp[wave][lane * PX + j] = col[j];
        __syncthreads();
        if (tid < STEP && x0 + tid < W) part[x0 + tid] = (colp[0][tid] + colp[1][tid]) + (colp[2][tid] + colp[3][tid]);
        __syncthreads();      // colp is free again, and behind the last step every wave's rowc is complete
    }
    if (tid < y1 - y0) p.prof[(size_t)b * ((size_t)H + W) + y0 + tid] = rowc[tid];
}

__global__ __launch_bounds__(256) void picture_cols_k(const PictureP p) {
    const int H = p.H, W = p.W, strips = (H + PC_STRIP - 1) / PC_STRIP, xb = (W + 255) / 256;
    const int b = blockIdx.x / xb, x = (blockIdx.x % xb) * 256 + (int)threadIdx.x;
    if (x >= W) return;
    const uint32_t* q = p.part + (size_t)b * strips * W + x;
    unsigned sum = 0u;
    for (int s = 0; s < strips; ++s, q += W) sum += *q;
    p.prof[(size_t)b * ((size_t)H + W) + H + x] = sum;
}

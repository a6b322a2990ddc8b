// resample_k.h — the antialiased resampler (include/rerevst_hip.h "Scaling"), gfx950; part of stages.hip (librerevst_stages.so).
//
// resample_k<IN>: one workgroup of 256 threads produces a tile of RS_TH x RS_TW output pixels of one frame, in one launch, on the tile
// skeleton of rs_tile.h; what is its own is the `pixel` functor that reads a source sample in the form IN, and the sink of pass 2:
//   1  horizontal pass, global memory -> LDS: for every source row the tile's vertical taps touch (p.rows at most) and each of the tile's
//      64 output columns, sum_j wx[j] * px(row, first_x + j) for the three BGR channels, px the float32 PIXEL value conv_first_k derives
//      from the same sample (uint8 (float)px; float32 PIXEL v, UNIT v * 255, NORM (v * sd + mean) * 255; YUV: the 3 x 4 matrix with every
//      operation rounded and the clamp to 0..255).  LDS holds [rows][64][3] floats: 26 KB at ratio 2, 104 KB at ratio 8 (RS_ROWS_MAX).
//   2  vertical pass, LDS -> global memory: consecutive lanes take consecutive floats of an output row (192 per tile row), so every
//      store instruction of a wave writes 256 contiguous bytes.
// Both passes accumulate in float32 with fmaf from -0, taps in ascending order (rs_tile.h), so an identity row, the one tap {1}, returns
// the source value bit for bit.
// One launch through LDS rather than two through an HBM intermediate: the intermediate of a 4K frame would be 12 bytes per
// half-scaled pixel written and read again, more than the source itself, and the tile's rows fit the 160 KiB of a CU at every allowed ratio.
// Reads are bounded by the tap tables (first + count <= S on both axes, built by the host); a chroma sample is (y >> csy, x >> csx) of a
// pixel inside the frame.  Every address is computed in 64 bits from the view, as conv_first_k does.
#include "rs_tile.h"

template <int IN>
__global__ __launch_bounds__(256) void resample_k(const ResampleP p) {
    constexpr bool YUV = IN >= IN_YUV_I420, Y16 = IN >= IN_YUV_I420_16, NV12 = IN == IN_YUV_NV12 || IN == IN_YUV_P016, CHW = !YUV && (IN & 1) != 0, F32 = !YUV && (IN & 2) != 0;
    typedef typename std::conditional<F32, float, typename std::conditional<Y16, uint16_t, uint8_t>::type>::type T;
    extern __shared__ __attribute__((aligned(16))) float s_rows[];      // [p.rows][RS_TW][3]
    __shared__ RsTaps s_t;
    const RsTile t = rs_tile_open(s_t, p.ay, p.ax, p.tiles_x, p.tiles_y, p.H, p.W, p.rows);

    const T* img = (const T*)p.img + (size_t)t.b * (size_t)p.v.fs;
    auto at = [&](int k, int row, int col) -> const T* {      // element `col` of row `row` of plane k
        return img + ((size_t)p.v.off[k] + (size_t)((uint64_t)(uint32_t)row * p.v.pitch[k]) + (size_t)col);
    };
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    auto pixel = [&](int y, int x, float (&o)[3]) {            // source pixel -> float32 PIXEL value, BGR order
        if constexpr (YUV) {
            const int crow = y >> p.csy, ccol = x >> p.csx;
            const T* const pcb = at(1, crow, ccol * (NV12 ? 2 : 1));
            const T* const pcr = NV12 ? pcb + 1 : at(2, crow, ccol);
            float yy, cb, cr;
            if constexpr (Y16) {
                yy = (float)(*at(0, y, x) >> p.yuv_shift);
                cb = (float)(*pcb >> p.yuv_shift);
                cr = (float)(*pcr >> p.yuv_shift);
            } else {
                yy = (float)*at(0, y, x); cb = (float)*pcb; cr = (float)*pcr;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {      // rows R, G, B of the matrix
                float v;
                {
#pragma clang fp contract(off)
                    const float a = p.yuv_n[4 * c] * yy + p.yuv_n[4 * c + 1] * cb;
                    const float ab = a + p.yuv_n[4 * c + 2] * cr;
                    v = ab + p.yuv_n[4 * c + 3];
                }
                o[2 - c] = fminf(fmaxf(v, 0.f), 255.f);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {      // c: RGB channel; HWC frames are BGR
                float v = CHW ? (float)*at(c, y, x) : (float)*at(0, y, x * 3 + 2 - c);
                if constexpr (F32) {
#pragma clang fp contract(off)
                    if (p.space == SP_UNIT) v = v * 255.0f;
                    else if (p.space == SP_NORM) v = (v * sd[c] + mean[c]) * 255.0f;
                }
                o[2 - c] = v;
            }
        }
    };

    rs_tile_rows(s_t, t, s_rows, pixel);
    __syncthreads();
    float* const out = p.out + ((size_t)t.b * (size_t)p.H + (size_t)t.oy0) * (size_t)p.W * 3 + (size_t)t.ox0 * 3;
    rs_tile_cols(s_t, t, s_rows, [&](int r, int e, float v) { out[(size_t)r * (size_t)p.W * 3 + e] = v; });
}

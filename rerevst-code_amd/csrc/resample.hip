// resample.hip — librerevst_scale.so: the antialiased resampler (include/rerevst_hip.h "Scaling"), gfx950.
//
// resample_k<IN>: one workgroup of 256 threads produces a tile of RS_TH x RS_TW output pixels of one frame, in one launch:
//   1  horizontal pass, global memory -> LDS: for every source row the tile's vertical taps touch (p.rows at most) and each of the tile's
//      64 output columns, sum_j wx[j] * px(row, first_x + j) for the three BGR channels, px the float32 PIXEL value conv_first_k derives
//      from the same sample (uint8 (float)px; float32 PIXEL v, UNIT v * 255, NORM (v * sd + mean) * 255; YUV: the 3 x 4 matrix with every
//      operation rounded and the clamp to 0..255).  LDS holds [rows][64][3] floats: 26 KB at ratio 2, 104 KB at ratio 8 (RS_ROWS_MAX).
//   2  vertical pass, LDS -> global memory: consecutive lanes take consecutive floats of an output row (192 per tile row), so every
//      store instruction of a wave writes 256 contiguous bytes.
// Both passes accumulate in float32 with fmaf from -0, taps in ascending order.  The host's device tables hold no tap of weight 0 (a trailing
// one is dropped from the count), so an identity row is the one tap {1} and returns the source value bit for bit, -0 and non-finite values
// included, whatever the neighbouring sample holds.
// One launch through LDS rather than two through an HBM intermediate: the intermediate of a 4K frame would be 12 bytes per
// half-scaled pixel written and read again, more than the source itself, and the tile's rows fit the 160 KiB of a CU at every allowed ratio.
// Reads are bounded by the tap tables (first + count <= S on both axes, built by the host); a chroma sample is (y >> csy, x >> csx) of a
// pixel inside the frame.  Every address is computed in 64 bits from the view, as conv_first_k does.
#include "resample.h"

template <int IN>
__global__ __launch_bounds__(256) void resample_k(const ResampleP p) {
    constexpr bool YUV = IN >= IN_YUV_I420, Y16 = IN >= IN_YUV_I420_16, NV12 = IN == IN_YUV_NV12 || IN == IN_YUV_P016, CHW = !YUV && (IN & 1) != 0, F32 = !YUV && (IN & 2) != 0;
    typedef typename std::conditional<F32, float, typename std::conditional<Y16, uint16_t, uint8_t>::type>::type T;
    extern __shared__ __attribute__((aligned(16))) float s_rows[];      // [p.rows][RS_TW][3]
    __shared__ float s_wx[RS_TAPS * RS_TW];                             // [tap][column]: lanes of a wave read consecutive banks
    __shared__ int s_fx[RS_TW], s_nx[RS_TW];
    __shared__ float s_wy[RS_TH * RS_TAPS];                             // [row][tap]
    __shared__ int s_fy[RS_TH], s_ny[RS_TH];
    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int tx = bx % p.tiles_x;
    bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    const int b = bx / p.tiles_y;
    const int ox0 = tx * RS_TW, oy0 = ty * RS_TH;
    const int ncol = min(RS_TW, p.W - ox0), nrow = min(RS_TH, p.H - oy0);      // the tile's valid columns and rows

    for (int i = tid; i < RS_TAPS * RS_TW; i += 256) {
        const int j = i / RS_TW, c = i - j * RS_TW;
        s_wx[i] = c < ncol ? p.ax.w[(size_t)(ox0 + c) * RS_TAPS + j] : 0.f;
    }
    if (tid < RS_TW) {
        s_fx[tid] = tid < ncol ? p.ax.first[ox0 + tid] : 0;
        s_nx[tid] = tid < ncol ? p.ax.count[ox0 + tid] : 0;
    }
    {
        const int r = tid / RS_TAPS;      // 256 = RS_TH * RS_TAPS
        s_wy[tid] = r < nrow ? p.ay.w[(size_t)(oy0 + r) * RS_TAPS + (tid - r * RS_TAPS)] : 0.f;
    }
    if (tid < RS_TH) {
        s_fy[tid] = tid < nrow ? p.ay.first[oy0 + tid] : 0;
        s_ny[tid] = tid < nrow ? p.ay.count[oy0 + tid] : 0;
    }
    __syncthreads();
    const int r0 = s_fy[0];                                               // first source row of the tile (first is non-decreasing)
    const int nsrc = min(s_fy[nrow - 1] + s_ny[nrow - 1] - r0, p.rows);   // rows to stage (the host sized p.rows as the largest of these)

    const T* img = (const T*)p.img + (size_t)b * (size_t)p.v.fs;
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

    {   // horizontal pass: thread = (column, row mod 4)
        const int col = tid & (RS_TW - 1);
        if (col < ncol) {
            const int fx = s_fx[col], nx = s_nx[col];
            for (int r = tid / RS_TW; r < nsrc; r += 256 / RS_TW) {
                float acc[3] = {-0.f, -0.f, -0.f};      // -0 + x == x for every x, -0 included
                for (int j = 0; j < nx; ++j) {
                    const float w = s_wx[j * RS_TW + col];
                    float px[3];
                    pixel(r0 + r, fx + j, px);
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[k] = fmaf(w, px[k], acc[k]);
                }
                float* const d = &s_rows[((size_t)r * RS_TW + col) * 3];
#pragma unroll
                for (int k = 0; k < 3; ++k) d[k] = acc[k];
            }
        }
    }
    __syncthreads();
    {   // vertical pass: consecutive threads take consecutive floats of an output row
        const int row_floats = ncol * 3;
        float* const out = p.out + ((size_t)b * (size_t)p.H + (size_t)oy0) * (size_t)p.W * 3 + (size_t)ox0 * 3;
        for (int i = tid; i < nrow * RS_TW * 3; i += 256) {
            const int r = i / (RS_TW * 3), e = i - r * (RS_TW * 3);
            if (e >= row_floats) continue;
            const int f = s_fy[r] - r0, n = s_ny[r];
            float acc = -0.f;
            for (int j = 0; j < n; ++j) {
                const int sr = f + j;
                if (sr < nsrc) acc = fmaf(s_wy[r * RS_TAPS + j], s_rows[(size_t)sr * (RS_TW * 3) + e], acc);
            }
            out[(size_t)r * (size_t)p.W * 3 + e] = acc;
        }
    }
}

template <int IN>
static hipError_t launch_form(const ResampleP& p, hipStream_t stream) {
    const size_t lds = resample_lds_bytes(p.rows);
    // dynamic LDS above 64 KB needs the attribute on the current device; set at every launch (cheap), so no state is shared between devices or threads
    const hipError_t e = hipFuncSetAttribute((const void*)resample_k<IN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)resample_lds_bytes(RS_ROWS_MAX));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(resample_k<IN>, dim3((unsigned)p.tiles_x * p.tiles_y * p.B), dim3(256), lds, stream, p);
    return hipGetLastError();
}

extern "C" int rrv_scale_launch(const ResampleP* p, int form, void* stream) {
    if (!p || form < 0 || form >= IN_FORMS || p->rows < 1 || p->rows > RS_ROWS_MAX || p->B < 1 || p->tiles_x < 1 || p->tiles_y < 1) return (int)hipErrorInvalidValue;
    static hipError_t (*const fn[IN_FORMS])(const ResampleP&, hipStream_t) = {
        launch_form<IN_U8_HWC>, launch_form<IN_U8_CHW>, launch_form<IN_F32_HWC>, launch_form<IN_F32_CHW>,
        launch_form<IN_YUV_I420>, launch_form<IN_YUV_NV12>, launch_form<IN_YUV_I420_16>, launch_form<IN_YUV_P016>};
    return (int)fn[form](*p, (hipStream_t)stream);
}

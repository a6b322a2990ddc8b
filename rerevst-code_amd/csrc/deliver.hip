// deliver.hip — librerevst_deliver.so: the output-side resampler (include/rerevst_hip.h "Scaling", "Output size"), gfx950.
//
// deliver_k<OUT>: one workgroup of 256 threads produces a tile of RS_TH x RS_TW delivered pixels of one frame, in one launch:
//   1  horizontal pass, global memory -> LDS: for every working row the tile's vertical taps touch (p.rows at most; 18 or fewer when upscaling)
//      and each of the tile's 64 delivered columns, sum_j wx[j] * in(row, first_x + j) for the three BGR channels.  LDS [rows][64][3].
//   2  vertical pass, LDS -> LDS: the tile's resampled values v, [16][64][3] floats (12 KB).  Every instantiation runs passes 1 and 2 with
//      the same code, so v is the same bits in all of them, and an identity axis (the one tap {1}) returns the input value.
//   3  store stage, LDS -> global memory through the view, in the form OUT.  Keeping v in LDS frees the lane mapping of the stores from
//      that of the arithmetic: in every form consecutive lanes write consecutive elements of a plane row (float: 256 contiguous bytes per
//      wave and row, uint8: 64), and a chroma sample reads the 1, 2 or 4 pixels of its block out of LDS with no cross-lane traffic.  Frames,
//      planes and rows of a view are only element aligned, so the integer forms leave as 1- or 2-byte stores.
// Both passes accumulate in float32 with fmaf from -0, taps in ascending order, as resample_k does.  The tables rs_build makes do hold taps of weight
// exactly 0, always a row's last (the 0 of an identity row {1, 0}; the third tap of some upscaled samples, e.g. 7 -> 55, sample 27: {4.4e-16, 1, 0}),
// and rrv_resample_taps reports them; the host drops them from the copy it uploads, so the tables the kernels read hold none.
// Reads are bounded by the tap tables (first + count <= S on both axes, built by the host).  Tile origins are even (16 x 64), so a chroma
// block never straddles tiles; a block's pixel outside the frame (odd last row or column) is replaced by its nearest one inside, which
// lies in the same tile.  Every address is computed in 64 bits from the view, as conv_last_k does.
#include "deliver.h"

template <int OUT>
__global__ __launch_bounds__(256) void deliver_k(const DeliverP p) {
    constexpr bool YUV = OUT == DL_YUV8 || OUT == DL_YUV16, Y16 = OUT == DL_YUV16, CHW = OUT == DL_F32_CHW || OUT == DL_U8_CHW;
    constexpr bool F32 = OUT == DL_F32_HWC || OUT == DL_F32_CHW;
    typedef typename std::conditional<F32, float, typename std::conditional<Y16, uint16_t, uint8_t>::type>::type T;
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];       // [p.rows][RS_TW][3] staged rows, then [RS_TH][RS_TW][3] the tile
    __shared__ float s_wx[RS_TAPS * RS_TW];                             // [tap][column]: lanes of a wave read consecutive banks
    __shared__ int s_fx[RS_TW], s_nx[RS_TW];
    __shared__ float s_wy[RS_TH * RS_TAPS];                             // [row][tap]
    __shared__ int s_fy[RS_TH], s_ny[RS_TH];
    float* const s_rows = s_dyn;
    float* const s_v = s_dyn + (size_t)p.rows * (RS_TW * 3);
    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int tx = bx % p.tiles_x;
    bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    const int b = bx / p.tiles_y;
    const int ox0 = tx * RS_TW, oy0 = ty * RS_TH;
    const int ncol = min(RS_TW, p.DW - ox0), nrow = min(RS_TH, p.DH - oy0);      // the tile's valid columns and rows

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
    const int r0 = s_fy[0];                                               // first working row of the tile (first is non-decreasing)
    const int nsrc = min(s_fy[nrow - 1] + s_ny[nrow - 1] - r0, p.rows);   // rows to stage (the host sized p.rows as the largest of these)

    {   // horizontal pass: thread = (column, row mod 4)
        const float* const img = p.in + (size_t)b * (size_t)p.H * (size_t)p.W * 3;
        const int col = tid & (RS_TW - 1);
        if (col < ncol) {
            const int fx = s_fx[col], nx = s_nx[col];
            for (int r = tid / RS_TW; r < nsrc; r += 256 / RS_TW) {
                const float* const src = img + ((size_t)(r0 + r) * (size_t)p.W + (size_t)fx) * 3;
                float acc[3] = {-0.f, -0.f, -0.f};      // -0 + x == x for every x, -0 included
                for (int j = 0; j < nx; ++j) {
                    const float w = s_wx[j * RS_TW + col];
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[k] = fmaf(w, src[j * 3 + k], acc[k]);
                }
                float* const d = &s_rows[((size_t)r * RS_TW + col) * 3];
#pragma unroll
                for (int k = 0; k < 3; ++k) d[k] = acc[k];
            }
        }
    }
    __syncthreads();
    {   // vertical pass: consecutive threads take consecutive floats of a tile row
        const int row_floats = ncol * 3;
        for (int i = tid; i < nrow * RS_TW * 3; i += 256) {
            const int r = i / (RS_TW * 3), e = i - r * (RS_TW * 3);
            if (e >= row_floats) continue;
            const int f = s_fy[r] - r0, n = s_ny[r];
            float acc = -0.f;
            for (int j = 0; j < n; ++j) {
                const int sr = f + j;
                if (sr < nsrc) acc = fmaf(s_wy[r * RS_TAPS + j], s_rows[(size_t)sr * (RS_TW * 3) + e], acc);
            }
            s_v[i] = acc;
        }
    }
    __syncthreads();

    // ---- store stage.  s_v[(r * RS_TW + c) * 3 + k]: channel k (B, G, R) of the tile's pixel (r, c), valid for r < nrow, c < ncol
    T* const fr = (T*)p.out + (size_t)b * (size_t)p.v.fs;
    auto at = [&](int k, int row, int col) -> T* {      // element `col` of row `row` of plane k of the delivered frame
        return fr + ((size_t)p.v.off[k] + (size_t)((uint64_t)(uint32_t)row * p.v.pitch[k]) + (size_t)col);
    };
    if constexpr (!YUV) {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};      // RGB order
        auto value = [&](float v, int c) -> T {      // the stored value of RGB channel c
            if constexpr (F32) {
#pragma clang fp contract(off)
                if (p.space == SP_PIXEL) return v;
                const float u = v / 255.0f;
                if (p.space == SP_UNIT) return u;
                return (u - mean[c]) / sd[c];
            } else {
                return (T)__builtin_rintf(fminf(fmaxf(v, 0.f), 255.f));      // half to even
            }
        };
        if constexpr (CHW) {      // planar RGB: consecutive lanes take consecutive columns of a plane row
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                for (int i = tid; i < nrow * RS_TW; i += 256) {
                    const int r = i / RS_TW, col = i - r * RS_TW;
                    if (col < ncol) *at(c, oy0 + r, ox0 + col) = value(s_v[i * 3 + 2 - c], c);
                }
            }
        } else {                  // HWC BGR: consecutive lanes take consecutive elements of a row
            const int row_elems = ncol * 3;
            for (int i = tid; i < nrow * RS_TW * 3; i += 256) {
                const int r = i / (RS_TW * 3), e = i - r * (RS_TW * 3);
                if (e < row_elems) *at(0, oy0 + r, ox0 * 3 + e) = value(s_v[i], 2 - e % 3);
            }
        }
    } else {
        const float hi = Y16 ? p.yuv_hi : 255.f;
        auto sample = [&](float v) -> T {      // clamp, round half to even, and (uint16 only) move the code to where the layout keeps it
            const float code = __builtin_rintf(fminf(fmaxf(v, 0.f), hi));
            if constexpr (Y16) return (T)((unsigned)code << p.yuv_shift);
            else return (T)code;
        };
        auto comp = [&](int k, int r, int c) -> float {      // c_k of the tile's pixel (r, c): ((m0 R + m1 G) + m2 B) + m3, every operation rounded
#pragma clang fp contract(off)
            const float* const px = &s_v[(r * RS_TW + c) * 3];
            const float rg = p.yuv_m[4 * k] * px[2] + p.yuv_m[4 * k + 1] * px[1];
            const float rgb = rg + p.yuv_m[4 * k + 2] * px[0];
            return rgb + p.yuv_m[4 * k + 3];
        };
        for (int i = tid; i < nrow * RS_TW; i += 256) {      // Y: consecutive lanes, consecutive samples of a row
            const int r = i / RS_TW, col = i - r * RS_TW;
            if (col < ncol) *at(0, oy0 + r, ox0 + col) = sample(comp(0, r, col));
        }
        const int csx = p.csx, csy = p.csy;
        auto chroma = [&](int k, int cr, int cc) -> float {      // the unrounded sample (cr, cc) of the tile's plane k, from the unclamped c_k
#pragma clang fp contract(off)
            const int y = cr << csy, x = cc << csx;
            const int y1 = min(y + 1, nrow - 1), x1 = min(x + 1, ncol - 1);      // outside the frame: the nearest pixel inside
            if (csy) return ((comp(k, y, x) + comp(k, y, x1)) + (comp(k, y1, x) + comp(k, y1, x1))) * 0.25f;      // 4:2:0
            if (csx) return (comp(k, y, x) + comp(k, y, x1)) * 0.5f;                                               // 4:2:2
            return comp(k, y, x);                                                                                  // 4:4:4
        };
        const int tcw = RS_TW >> csx;                                             // chroma columns of a full tile
        const int ncc = (ncol + csx) >> csx, ncr = (nrow + csy) >> csy;           // the tile's valid chroma columns and rows
        const int cy0 = oy0 >> csy, cx0 = ox0 >> csx;                             // the tile's chroma origin
        if (p.nv12) {      // interleaved CbCr rows: consecutive lanes take consecutive elements, Cb and Cr in turn
            for (int i = tid; i < ncr * 2 * tcw; i += 256) {
                const int cr = i / (2 * tcw), e = i - cr * (2 * tcw);
                if ((e >> 1) < ncc) *at(1, cy0 + cr, 2 * cx0 + e) = sample(chroma(1 + (e & 1), cr, e >> 1));
            }
        } else {
#pragma unroll
            for (int k = 1; k < 3; ++k) {
                for (int i = tid; i < ncr * tcw; i += 256) {
                    const int cr = i / tcw, cc = i - cr * tcw;
                    if (cc < ncc) *at(k, cy0 + cr, cx0 + cc) = sample(chroma(k, cr, cc));
                }
            }
        }
    }
}

template <int OUT>
static hipError_t launch_form(const DeliverP& p, hipStream_t stream) {
    const size_t lds = deliver_lds_bytes(p.rows);
    // dynamic LDS above 64 KB needs the attribute on the current device; set at every launch (cheap), so no state is shared between devices or threads
    const hipError_t e = hipFuncSetAttribute((const void*)deliver_k<OUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)deliver_lds_bytes(RS_ROWS_MAX));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(deliver_k<OUT>, dim3((unsigned)p.tiles_x * p.tiles_y * p.B), dim3(256), lds, stream, p);
    return hipGetLastError();
}

extern "C" int rrv_deliver_launch(const DeliverP* p, int form, void* stream) {
    if (!p || form < 0 || form >= DL_FORMS || p->rows < 1 || p->rows > RS_ROWS_MAX || p->B < 1 || p->tiles_x < 1 || p->tiles_y < 1) return (int)hipErrorInvalidValue;
    if (p->tiles_x != (p->DW + RS_TW - 1) / RS_TW || p->tiles_y != (p->DH + RS_TH - 1) / RS_TH) return (int)hipErrorInvalidValue;      // (the kernel trusts them)
    static hipError_t (*const fn[DL_FORMS])(const DeliverP&, hipStream_t) = {
        launch_form<DL_F32_HWC>, launch_form<DL_F32_CHW>, launch_form<DL_U8_HWC>, launch_form<DL_U8_CHW>, launch_form<DL_YUV8>, launch_form<DL_YUV16>};
    return (int)fn[form](*p, (hipStream_t)stream);
}

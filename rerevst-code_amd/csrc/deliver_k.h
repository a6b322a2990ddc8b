// deliver_k.h — the output-side resampler (include/rerevst_hip.h "Scaling", "Output size"), gfx950; part of stages.hip (librerevst_stages.so).
//
// deliver_k<OUT>: one workgroup of 256 threads produces a tile of RS_TH x RS_TW delivered pixels of one frame, in one launch.  Passes 1 and 2
// are resample_k's, the tile skeleton of rs_tile.h over a three-load `pixel` functor and a sink into LDS; the store stage is its own:
//   1  horizontal pass, global memory -> LDS: for every working row the tile's vertical taps touch (p.rows at most; 18 or fewer when upscaling)
//      and each of the tile's 64 delivered columns, sum_j wx[j] * in(row, first_x + j) for the three BGR channels.  LDS [rows][64][3].
//   2  vertical pass, LDS -> LDS: the tile's resampled values v, [16][64][3] floats (12 KB).  Every instantiation runs passes 1 and 2 with
//      the same code, so v is the same bits in all of them, and an identity axis (the one tap {1}) returns the input value.
//   3  store stage, LDS -> global memory through the view, in the form OUT.  Keeping v in LDS frees the lane mapping of the stores from
//      that of the arithmetic: in every form consecutive lanes write consecutive elements of a plane row (float: 256 contiguous bytes per
//      wave and row, uint8: 64), and a chroma sample reads the 1, 2 or 4 pixels of its block out of LDS with no cross-lane traffic.  Frames,
//      planes and rows of a view are only element aligned, so the integer forms leave as 1- or 2-byte stores.
// Both passes accumulate in float32 with fmaf from -0, taps in ascending order (rs_tile.h).  The tables rs_build makes do hold taps of weight
// exactly 0, always a row's last (the 0 of an identity row {1, 0}; the third tap of some upscaled samples, e.g. 7 -> 55, sample 27: {4.4e-16, 1, 0}),
// and rrv_resample_taps reports them; the host drops them from the copy it uploads, so the tables the kernels read hold none.
// Reads are bounded by the tap tables (first + count <= S on both axes, built by the host).  Tile origins are even (16 x 64), so a chroma
// block never straddles tiles; a block's pixel outside the frame (odd last row or column) is replaced by its nearest one inside, which
// lies in the same tile.  Every address is computed in 64 bits from the view, as conv_last_k does.
#include "deliver.h"
#include "rs_tile.h"

template <int OUT>
__global__ __launch_bounds__(256) void deliver_k(const DeliverP p) {
    constexpr bool YUV = OUT == DL_YUV8 || OUT == DL_YUV16, Y16 = OUT == DL_YUV16, CHW = OUT == DL_F32_CHW || OUT == DL_U8_CHW;
    constexpr bool F32 = OUT == DL_F32_HWC || OUT == DL_F32_CHW;
    typedef typename std::conditional<F32, float, typename std::conditional<Y16, uint16_t, uint8_t>::type>::type T;
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];       // [p.rows][RS_TW][3] staged rows, then [RS_TH][RS_TW][3] the tile
    __shared__ RsTaps s_t;
    float* const s_rows = s_dyn;
    float* const s_v = s_dyn + (size_t)p.rows * (RS_TW * 3);
    const RsTile t = rs_tile_open(s_t, p.ay, p.ax, p.tiles_x, p.tiles_y, p.DH, p.DW, p.rows);
    const int tid = threadIdx.x, b = t.b, ox0 = t.ox0, oy0 = t.oy0, ncol = t.ncol, nrow = t.nrow;

    const float* const img = p.in + (size_t)b * (size_t)p.H * (size_t)p.W * 3;
    rs_tile_rows(s_t, t, s_rows, [&](int y, int x, float (&o)[3]) {
        const float* const px = img + ((size_t)y * (size_t)p.W + (size_t)x) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = px[k];
    });
    __syncthreads();
    rs_tile_cols(s_t, t, s_rows, [&](int r, int e, float v) { s_v[r * (RS_TW * 3) + e] = v; });
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

// conv_thin.h — the two HBM-bound ends of the per-frame path, on the vector ALUs.
//
// conv_first_k: uint8 BGR HWC frame -> [greyscale] -> ImageNet normalise -> conv3x3 3->64
//   + bias + ReLU.  Fuses numpy2tensor/transform_image (test/framework.py:26-35),
//   TransformerNet.RGB2Gray (test/style_network_global.py:487-497, quirk Q5) and
//   vgg19.features[0:2].  Reads 3 B/pixel, writes 256 B/pixel.
// conv_last_k: conv3x3 64->3 + bias (Decoder.slice1, :341,450) fused with
//   transform_back_image/tensor2numpy (test/framework.py:39-49): *std+mean, clamp(0,1),
//   *255, RGB->BGR, HWC float32.  Reads 256 B/pixel, writes 12 (+12) B/pixel.
//   conv_last_k<true>: the same, then rint (v_rndne_f32: round half to even, as np.rint) and one byte per channel: HWC
//   uint8, the float form's values quantised on the GPU (cv2.imwrite's conversion).  Writes 3 (+12) B/pixel.
// Torch forms (rrv_transfer_image_device): conv_first_k<IN> also reads planar [B][3][H][W] RGB (torch's NCHW) and float32
//   frames in one of three value spaces; conv_last_k<U8, CHW, SPACE> also writes planar RGB and the UNIT / NORM spaces.  The
//   default instantiations are the uint8 BGR HWC forms above, unchanged.
// YUV form (the rrv_*_yuv entries, out.layout = RRV_LAY_I420 / RRV_LAY_NV12): conv_last_k<true, false, SP_PIXEL, true> converts the
//   float form's values with a 3 x 4 matrix and stores 8-bit 4:2:0, a Y byte per pixel and a Cb, Cr pair per 2 x 2 block.  Writes
//   1.5 (+12) B/pixel.
// YUV input (the rrv_*_from_yuv entries): conv_first_k<IN_YUV_I420 / IN_YUV_NV12> reads a Y byte per pixel and the Cb, Cr bytes of its
//   2 x 2 block, converts them with a 3 x 4 matrix to the float32 PIXEL value and goes on as the float32 form does.  Reads 1.5 B/pixel.
// 10 / 12 / 16-bit YUV (RRV_LAY_I420_16 / RRV_LAY_P016, uint16 samples): conv_first_k<IN_YUV_I420_16 / IN_YUV_P016> loads a uint16 per sample
//   and shifts it right by FirstP::yuv_shift (0 for the planar form, whose code sits in the low bits; 16 - d for P016, whose code sits in the
//   high bits); conv_last_k<true, false, SP_PIXEL, true, true> clamps to LastP::yuv_hi = 2^d - 1, shifts the code left by LastP::yuv_shift
//   and stores a uint16.  3 B/pixel each way.  The 8-bit instantiations are the code they were: the depth is a template argument.
// 4:2:2 / 4:4:4 (RRV_LAY_422 / RRV_LAY_444 on a YUV layout): no instantiation of their own — FirstP::csx / csy and LastP::csx / csy are the chroma
//   shifts of the launch, (1, 1) 4:2:0, (1, 0) 4:2:2, (0, 0) 4:4:4: a pixel reads chroma sample (y >> csy, x >> csx); the last kernel keeps the lane ^ 1
//   step of its mean only where csx is set and the lane ^ 16 step only where csy is, and stores a chroma sample per 2^csy x 2^csx block.  2 / 3 samples
//   per pixel each way.  The shifts are kernel arguments, uniform over the launch.
// Image views (rrv_image_view, the rrv_*_view_device entries): both kernels find a frame's rows through FirstP::v / LastP::v — frame stride, plane
//   offsets and pitches in elements — so pitched surfaces, crops and canvas windows are read and written in place.  Packed frames are the view
//   contiguous_view() builds; the values and their order are those of the packed code, only the addresses differ.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "conv_mfma.h"   // bufld16

// Value spaces of a frame (include/rerevst_hip.h RRV_SP_*): PIXEL 0..255, UNIT 0..1, NORM transform_image's (x/255 - mean)/std
enum : int { SP_PIXEL = 0, SP_UNIT = 1, SP_NORM = 2 };
// conv_first_k's input forms (the template argument): bit 0 planar CHW RGB (else HWC BGR), bit 1 float32 (else uint8)
// 4, 5: 8-bit YUV 4:2:0 frames, [Y: H*W][Cb: CH*CW][Cr: CH*CW] (I420) or [Y: H*W][CbCr interleaved: CH*CW*2] (NV12), CH = (H+1)/2, CW = (W+1)/2
// 6, 7: the same two layouts in uint16 samples (10 / 12 / 16-bit codes: planar with the code in the low bits, semi-planar P010 / P012 / P016 with it in the high bits)
enum : int { IN_U8_HWC = 0, IN_U8_CHW = 1, IN_F32_HWC = 2, IN_F32_CHW = 3, IN_YUV_I420 = 4, IN_YUV_NV12 = 5, IN_YUV_I420_16 = 6, IN_YUV_P016 = 7, IN_FORMS = 8 };
inline bool in_yuv(int form) { return form >= IN_YUV_I420; }
inline bool in_yuv16(int form) { return form >= IN_YUV_I420_16; }
inline size_t in_elem(int form) { return in_yuv16(form) ? sizeof(uint16_t) : !in_yuv(form) && (form & 2) ? sizeof(float) : 1; }     // bytes per input value
// Chroma format of a YUV frame (include/rerevst_hip.h RRV_LAY_422 / RRV_LAY_444 on a YUV layout): pixel (y, x) belongs to chroma sample
// (y >> sy, x >> sx), the planes are CH = ceil(H / 2^sy) rows of CW = ceil(W / 2^sx) samples.  The plane ORDER stays the layout's.
enum : int { CS_420 = 0, CS_422 = 1, CS_444 = 2 };
inline int chroma_sx(int cs) { return cs == CS_444 ? 0 : 1; }
inline int chroma_sy(int cs) { return cs == CS_420 ? 1 : 0; }
inline double yuv_samples_per_pixel(int cs) { return 1.0 + 2.0 / (double)(1 << (chroma_sx(cs) + chroma_sy(cs))); }      // 1.5, 2, 3
inline size_t yuv_frame_samples(size_t H, size_t W, int cs = CS_420) {     // Y, Cb, Cr samples of one frame
    return H * W + 2 * ((H + chroma_sy(cs)) >> chroma_sy(cs)) * ((W + chroma_sx(cs)) >> chroma_sx(cs));
}
inline size_t in_frame_bytes(int form, size_t H, size_t W, int cs = CS_420) {                     // bytes of one H x W input frame
    return (in_yuv(form) ? yuv_frame_samples(H, W, cs) : H * W * 3) * in_elem(form);
}

// Where the rows of a frame's planes lie (include/rerevst_hip.h rrv_image_view), in ELEMENTS of the frame's type: frame b starts fs * b elements
// after the base pointer, row r of plane k at off[k] + r * pitch[k] from there.  Planes: HWC one (a row is 3 W elements); CHW R, G, B; I420 Y, Cb,
// Cr; NV12 / P016 Y and the interleaved CbCr rows (2 CW elements).  Both kernels address every frame through one of these, the contiguous
// frames of the plain entries included (contiguous_view): there is no second addressing path.
// A pitch is below 2^31 elements (rrv_image_view_check refuses more), so row x pitch is one 32 x 32 -> 64-bit multiply, what row x W was.
struct ImgView { int64_t fs, off[3]; uint32_t pitch[3]; };
enum : int { VL_HWC = 0, VL_CHW = 1, VL_I420 = 2, VL_NV12 = 3 };      // plane structure of a layout (the 16-bit YUV layouts share the 8-bit ones')
inline ImgView contiguous_view(int vl, int64_t H, int64_t W, int cs = CS_420) {
    const int64_t CH = (H + chroma_sy(cs)) >> chroma_sy(cs), CW = (W + chroma_sx(cs)) >> chroma_sx(cs);
    switch (vl) {
    case VL_HWC:  return ImgView{3 * H * W, {0, 0, 0}, {(uint32_t)(3 * W), 0, 0}};
    case VL_CHW:  return ImgView{3 * H * W, {0, H * W, 2 * H * W}, {(uint32_t)W, (uint32_t)W, (uint32_t)W}};
    case VL_I420: return ImgView{H * W + 2 * CH * CW, {0, H * W, H * W + CH * CW}, {(uint32_t)W, (uint32_t)CW, (uint32_t)CW}};
    default:      return ImgView{H * W + 2 * CH * CW, {0, H * W, 0}, {(uint32_t)W, (uint32_t)(2 * CW), 0}};
    }
}

struct FirstP {
    const void* img;      // frame b's planes through `v`; IN_*_HWC BGR, IN_*_CHW RGB planes, uint8 or float32; IN_YUV_*: Y and chroma planes, uint8 (uint16 for the two 16-bit forms)
    int H, W, B;
    float* out;           // [B,H,W,64] ring layout
    const float* w;       // [27][64]: row (ky*3+kx)*3 + c_rgb
    const float* bias;    // [64]
    int grey;             // 1: content frame (greyscaled), 0: style image (colour)
    int tiles_x, tiles_y;
    const float* wg;      // grey fold (pack_first_grey_k): W1 [9][64] | W0 [9][64] | bias + sum W0 [64]; null: never fold
    // optional on-device ReshapeTool.process (test/generate_real_video.py:61-83): img is the UNPADDED [B][src_H][src_W][3]
    // frame and padded pixel (y, x) reads source pixel (reflect(y - pad_top), reflect(x - pad_left)), edge-inclusive
    // (cv2.BORDER_REFLECT = numpy 'symmetric').  src_H == 0: img already has the padded geometry.
    int src_H, src_W, pad_top, pad_left;
    int p8;               // 1: `out` is channel-chunk-major [B][8 chunks][H+2][W+8][8], pixel x at column x + 4 (conv_f43.h LAY: what conv1_2 on conv_f43_k reads 12-19 % faster); same values
    int space;            // value space of a float32 input (SP_*); a uint8 input is PIXEL
    float yuv_n[12];      // IN_YUV_*: rows R, G, B; columns the coefficients of Y, Cb, Cr and an offset (rrv_set_yuv_input_matrix; the 16-bit forms: rrv_set_yuv16_input_matrix), by value
    int yuv_shift;        // IN_YUV_I420_16: 0; IN_YUV_P016: 16 - d, the code is sample >> yuv_shift (the low bits are ignored)
    int csx, csy;         // IN_YUV_*: the chroma shifts, (1, 1) 4:2:0, (1, 0) 4:2:2, (0, 0) 4:4:4: pixel (y, x) reads chroma sample (y >> csy, x >> csx)
    ImgView v;            // where the source frame's rows are, in elements of its type (the SOURCE frame: src_H x src_W in the pad geometry)
};
inline int in_view_layout(int form) { return form == IN_YUV_I420 || form == IN_YUV_I420_16 ? VL_I420 : in_yuv(form) ? VL_NV12 : (form & 1) ? VL_CHW : VL_HWC; }

// symmetric (edge-inclusive) reflection of t into [0, n), any distance
__device__ __forceinline__ int reflect_sym(int t, int n) {
    const int period = 2 * n;
    t %= period;
    if (t < 0) t += period;
    return t < n ? t : period - 1 - t;
}

// IN: input form (IN_*).  Every form turns a source pixel into the normalised value n the uint8 form computes,
// ((float)px / 255 - mean) / std: a float PIXEL value v as v / 255 (bit-identical for integral v), a UNIT value x in place of
// px / 255 (the same float where x is the correctly rounded px / 255), a NORM value n as it is.  Everything after that (grey
// fold, border path, P8 stores, reflect-pad addressing) is shared.
// IN_YUV_*: source pixel (y, x) takes Y[y][x] and the chroma sample (y >> csy, x >> csx) (4:2:0: (y >> 1, x >> 1)) — after the reflection of the pad geometry, which
// therefore equals reflect-padding the converted frame, also for odd H / W — and v_k = ((n[k][0] Y + n[k][1] Cb) + n[k][2] Cr) + n[k][3],
// every product and sum rounded to float32 (no contraction), px_k = min(max(v_k, 0), 255), not rounded to an integer: the float PIXEL
// value.  Frame starts and chroma planes are in general not dword aligned: byte loads (the uint16 forms: 2-byte loads; a frame is an odd
// number of samples where H*W is odd).  The uint16 forms use code = sample >> yuv_shift in place of the byte.
template <int IN = IN_U8_HWC>
__global__ __launch_bounds__(256) void conv_first_k(const FirstP p) {
    constexpr bool YUV = IN >= IN_YUV_I420, Y16 = IN >= IN_YUV_I420_16, NV12 = IN == IN_YUV_NV12 || IN == IN_YUV_P016, CHW = !YUV && (IN & 1) != 0, F32 = !YUV && (IN & 2) != 0;
    typedef typename std::conditional<F32, float, typename std::conditional<Y16, uint16_t, uint8_t>::type>::type T;
    __shared__ __attribute__((aligned(16))) float s_in[18 * 18 * 4];
    __shared__ __attribute__((aligned(16))) float s_w[27 * 64];
    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int tx = bx % p.tiles_x;
    bx /= p.tiles_x;
    const int ty = bx % p.tiles_y;
    const int b = bx / p.tiles_y;
    const int y0 = ty * 16, x0 = tx * 16;
    const int SH = p.src_H ? p.src_H : p.H, SW = p.src_H ? p.src_W : p.W;
    const T* img = (const T*)p.img + (size_t)b * (size_t)p.v.fs;
    struct SrcPx { int y, x; };             // row and column of a pixel in the source frame
    auto src_px = [&](int y, int x) {       // padded-frame pixel -> the source pixel it reads
        if (p.src_H) { y = reflect_sym(y - p.pad_top, SH); x = reflect_sym(x - p.pad_left, SW); }
        return SrcPx{y, x};
    };
    auto at = [&](int k, int row, int col) -> const T* {      // element `col` of row `row` of plane k
        return img + ((size_t)p.v.off[k] + (size_t)((uint64_t)(uint32_t)row * p.v.pitch[k]) + (size_t)col);
    };

    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    auto norm_of = [&](const SrcPx& s, int c) -> float {      // source pixel -> normalised value of channel c, RGB order (framework.py:27,33-34)
        if constexpr (YUV) {
            const int crow = s.y >> p.csy, ccol = s.x >> p.csx;      // (wave-uniform shifts: the chroma format is a launch parameter)
            const T* const pcb = at(1, crow, ccol * (NV12 ? 2 : 1));
            const T* const pcr = NV12 ? pcb + 1 : at(2, crow, ccol);
            float yy, cb, cr;
            if constexpr (Y16) {
                yy = (float)(*at(0, s.y, s.x) >> p.yuv_shift);
                cb = (float)(*pcb >> p.yuv_shift);
                cr = (float)(*pcr >> p.yuv_shift);
            } else {
                yy = (float)*at(0, s.y, s.x); cb = (float)*pcb; cr = (float)*pcr;
            }
            float v;
            {
#pragma clang fp contract(off)
                const float a = p.yuv_n[4 * c] * yy + p.yuv_n[4 * c + 1] * cb;
                const float ab = a + p.yuv_n[4 * c + 2] * cr;
                v = ab + p.yuv_n[4 * c + 3];
            }
            return (fminf(fmaxf(v, 0.f), 255.f) / 255.0f - mean[c]) / sd[c];      // as a float32 PIXEL value from here on
        }
        const float v = CHW ? (float)*at(c, s.y, s.x) : (float)*at(0, s.y, s.x * 3 + 2 - c);
        if constexpr (F32) {
            if (p.space == SP_NORM) return v;
            return ((p.space == SP_UNIT ? v : v / 255.0f) - mean[c]) / sd[c];
        }
        return (v / 255.0f - mean[c]) / sd[c];
    };
    // A greyscaled frame feeds the three input channels with affine functions of one value g (RGB2Gray + the
    // re-normalisation, test/style_network_global.py:487-497): 9 multiplies per output instead of 27.  The fold
    // assumes all nine taps inside the image, so tiles that touch the image border take the general path below.
    if (p.grey && p.wg && y0 > 0 && x0 > 0 && y0 + 16 < p.H && x0 + 16 < p.W) {
        float* s_g = s_in;      // [18][18] grey values
        for (int i = tid; i < 18 * 18; i += 256) {
            const int hy = i / 18, hx = i - hy * 18;
            const SrcPx px = src_px(y0 + hy - 1, x0 + hx - 1);
            float d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = norm_of(px, c) * sd[c] + mean[c];   // as the reference rounds it
            s_g[i] = d[2] * 0.299f + d[1] * 0.587f + d[0] * 0.114f;   // :493 (sic)
        }
        __syncthreads();
        if (p.p8) {      // the same arithmetic under another thread mapping: thread = (half of a chunk: 4 channels, pixel column, chunk), a loop over the 16 rows —
                         // consecutive lanes store consecutive 16-byte pieces: 32 lanes = 16 pixels x 32 bytes = 512 contiguous bytes of one chunk plane
            const int half = tid & 1, pc = (tid >> 1) & 15, k8 = tid >> 5, q4 = (k8 * 2 + half) * 4;
            f32x4 w1[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) w1[k] = *(const f32x4*)&p.wg[k * 64 + q4];
            const f32x4 bias = *(const f32x4*)&p.wg[1152 + q4];
            float* const plane = p.out + ((size_t)b * 8 + k8) * (size_t)(p.H + 2) * (p.W + 8) * 8 + ((size_t)(y0 + 1) * (p.W + 8) + x0 + pc + 4) * 8 + half * 4;      // rows pitched W + 8, pixel x at column x + 4: every 512-byte run starts on a line (conv_f43.h P8_PAD / P8_COL0)
            float g[3][3];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) g[r + 1][c] = s_g[r * 18 + pc + c];
#pragma unroll
            for (int prow = 0; prow < 16; ++prow) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { g[0][c] = g[1][c]; g[1][c] = g[2][c]; g[2][c] = s_g[(prow + 2) * 18 + pc + c]; }
                f32x4 acc = bias;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) acc += w1[ky * 3 + kx] * g[ky][kx];
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = fmaxf(acc[e], 0.f);
                __builtin_nontemporal_store(r, (f32x4*)&plane[(size_t)prow * (p.W + 8) * 8]);
            }
            return;
        }
        const int q = tid & 15, prow = tid >> 4;
        f32x4 w1[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w1[k] = *(const f32x4*)&p.wg[k * 64 + q * 4];
        const f32x4 bias = *(const f32x4*)&p.wg[1152 + q * 4];
        float g[3][18];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 18; ++c) g[r][c] = s_g[(prow + r) * 18 + c];
        float* orow = p.out + (size_t)b * (size_t)(p.H + 2) * (p.W + 2) * 64 + ((size_t)(y0 + prow + 1) * (p.W + 2) + x0 + 1) * 64 + q * 4;
#pragma unroll
        for (int pc = 0; pc < 16; ++pc) {
            f32x4 acc = bias;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc += w1[ky * 3 + kx] * g[ky][pc + kx];
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fmaxf(acc[e], 0.f);
            __builtin_nontemporal_store(r, (f32x4*)&orow[pc * 64]);
        }
        return;
    }
    for (int i = tid; i < 27 * 64; i += 256) s_w[i] = p.w[i];
    for (int i = tid; i < 18 * 18; i += 256) {
        const int hy = i / 18, hx = i - hy * 18;
        const int y = y0 + hy - 1, x = x0 + hx - 1;
        float o[3] = {0.f, 0.f, 0.f};
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
            const SrcPx px = src_px(y, x);
            float n[3];   // normalised, RGB order (framework.py:27,33-34)
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = norm_of(px, c);
            if (p.grey) {
                float d[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = n[c] * sd[c] + mean[c];
                const float g = d[2] * 0.299f + d[1] * 0.587f + d[0] * 0.114f;   // :493 (sic)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = (g - mean[c]) / sd[c];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = n[c];
            }
        }
        *(f32x4*)&s_in[i * 4] = f32x4{o[0], o[1], o[2], 0.f};
    }
    __syncthreads();

    if (p.p8) {      // border tiles of a channel-chunk-major output: the general arithmetic below under the thread mapping of the fast path above
        const int half = tid & 1, pc = (tid >> 1) & 15, k8 = tid >> 5, q4 = (k8 * 2 + half) * 4;
        f32x4 w[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) w[k] = *(const f32x4*)&s_w[k * 64 + q4];
        const f32x4 bias = *(const f32x4*)&p.bias[q4];
        float* const plane = p.out + ((size_t)b * 8 + k8) * (size_t)(p.H + 2) * (p.W + 8) * 8 + half * 4;
        const int x = x0 + pc;
        for (int prow = 0; prow < 16; ++prow) {
            f32x4 acc = bias;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const f32x4 v = *(const f32x4*)&s_in[((prow + ky) * 18 + pc + kx) * 4];
                    const int k = (ky * 3 + kx) * 3;
                    acc += w[k] * v[0];
                    acc += w[k + 1] * v[1];
                    acc += w[k + 2] * v[2];
                }
            const int y = y0 + prow;
            if (y < p.H && x < p.W) {
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = fmaxf(acc[e], 0.f);
                *(f32x4*)&plane[((size_t)(y + 1) * (p.W + 8) + x + 4) * 8] = r;
            }
        }
        return;
    }
    const int q = tid & 15;      // output channels 4q..4q+3
    const int prow = tid >> 4;   // pixel row inside the tile
    f32x4 w[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = *(const f32x4*)&s_w[k * 64 + q * 4];
    const f32x4 bias = *(const f32x4*)&p.bias[q * 4];
    float* out_b = p.out + (size_t)b * (size_t)(p.H + 2) * (p.W + 2) * 64;
    const int y = y0 + prow;
    for (int pc = 0; pc < 16; ++pc) {
        f32x4 acc = bias;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 v = *(const f32x4*)&s_in[((prow + ky) * 18 + pc + kx) * 4];
                const int k = (ky * 3 + kx) * 3;
                acc += w[k] * v[0];
                acc += w[k + 1] * v[1];
                acc += w[k + 2] * v[2];
            }
        const int x = x0 + pc;
        if (y < p.H && x < p.W) {
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fmaxf(acc[e], 0.f);
            *(f32x4*)&out_b[((size_t)(y + 1) * (p.W + 2) + x + 1) * 64 + q * 4] = r;
        }
    }
}

struct LastP {
    const float* in;      // [B,H,W,64] ring layout
    int H, W, B;
    const float* w;       // pack_last_k: [blk 2][c 4][lane 64][s 4] MFMA A operands of the 27 x 64 tap-rgb matrix
    const float* bias;    // [4]
    void* out_img;        // [B][H][W][3] BGR: float32 0..255 (conv_last_k<false>) or its rint as uint8 (conv_last_k<true>); CHW: [B][3][H][W] RGB
    float* out_pre;       // optional [B][H][W][3] RGB pre-clamp (normalised units), may be null
    int tiles_x, tiles_y;
    // optional on-device crop (generate_real_video.py:167): out_img is [B][out_H][out_W][3] and receives the window
    // that starts at (crop_top, crop_left) of the padded frame.  out_H == 0: the whole padded frame.
    int out_H, out_W, crop_top, crop_left;
    int ty0, tx0;         // first tile row / column of the computed window (tiles_x, tiles_y count its tiles)
    // the YUV 4:2:0 store form (conv_last_k<true, false, SP_PIXEL, true>): out_img is [B][OH*OW Y][chroma] uint8, frame b at b * (OH*OW + 2*CH*CW)
    float yuv_m[12];      // rows Y, Cb, Cr; columns the coefficients of R, G, B and an offset (rrv_set_yuv_matrix), by value
    int yuv_nv12;         // 0: I420, planes [Cb: CH*CW][Cr: CH*CW]; 1: NV12, one plane of CH*CW (Cb, Cr) pairs
    // the uint16 instantiation (conv_last_k<true, false, SP_PIXEL, true, true>): samples in place of bytes, yuv_m the 16-bit matrix
    float yuv_hi;         // 2^d - 1, the upper clamp bound of a d-bit code
    int yuv_shift;        // stored sample = code << yuv_shift: 0 planar (code in the low bits), 16 - d for P016 (code in the high bits)
    int csx, csy;         // the chroma shifts of the YUV forms: (1, 1) 4:2:0, (1, 0) 4:2:2, (0, 0) 4:4:4; a chroma sample per 2^csy x 2^csx block
    ImgView v;            // where out_img's rows are, in elements of its type (the frame as delivered: OH x OW); out_pre stays contiguous
};

// GEMM first, taps second.  out[y][x][rgb] = sum_tap sum_c w[tap][c][rgb] in[y+ky][x+kx][c] is evaluated as
//   G[p][tap*3+rgb] = sum_c W[tap*3+rgb][c] in[p][c]     for the 18 x 18 halo pixels p of a 16 x 16 tile — one
//                     [27 -> 32] x [64] x [324] GEMM on v_mfma_f32_16x16x4_f32, the input straight from global memory
//                     into the B operand (each value is read ONCE), the weights resident in 32 registers per lane,
//   out[y][x][rgb] = bias + sum_tap G[(y+ky, x+kx)][tap*3+rgb]      27 shifted LDS reads per output value (planes of
//                     324 floats: consecutive lanes = consecutive pixels, conflict-free).
// Round 2's direct form re-read every input value from LDS for each of its nine taps (288 ds_read_b128 per wave and
// tile, LDS-bound at 0.38 of the HBM peak); here LDS carries 27 floats per halo pixel once in and once out.
// Workgroups are persistent (the weight registers are loaded once) and walk the tiles of the window.
#define LAST_GP 330       /* floats per G plane (324 used); 4 planes = 8 banks on: the four row groups of a wave write disjoint banks */
// U8: the uint8 store form; everything before the store is the same code in both instantiations (a template kernel, not an
// inlined body: the float instantiation compiles to the instructions of the non-template kernel it replaced)
// CHW: planar [B][3][OH][OW] RGB (torch's NCHW) instead of HWC BGR.  SPACE: SP_PIXEL (0..255, the forms above), SP_UNIT (the
// clamped 0..1 value the PIXEL form multiplies by 255, so UNIT * 255.0f == PIXEL bit for bit) or SP_NORM (the pre-clamp network
// output, the out_pre value); UNIT and NORM are float32 only.
// YUV: 8-bit YUV 4:2:0 from the float32 PIXEL values (with U8, HWC, SP_PIXEL): c_k = ((m[k][0] R + m[k][1] G) + m[k][2] B) + m[k][3], every
// product and sum rounded to float32 (no contraction); a Y byte per pixel, rint(clamp(c_0, 0, 255)); a Cb and a Cr byte per 2 x 2 block
// of the OUTPUT frame, rint(clamp(((tl + tr) + (bl + br)) * 0.25f, 0, 255)) of the unclamped c_1 / c_2, a pixel of the block outside
// the frame (odd OH / OW, last row / column) replaced by its nearest one inside.  The crop origin and the tile origins are even, so
// a block's four pixels are lanes l, l^1, l^16, l^17 of one wave.
// Chroma format (p.csx, p.csy; wave-uniform): 4:2:2 keeps the lane ^ 1 step only, (l + r) * 0.5f per pixel pair of a row, a last odd column
// paired with itself; 4:4:4 keeps neither, every pixel stores its own c_1, c_2.  Both shuffles are issued in every format (all 64 lanes
// active, before the bounds branch); a format only chooses which sums enter the value, so 4:2:0 evaluates the expression above unchanged.
// Y16 (with YUV): d-bit codes in uint16 samples, 10 / 12 / 16 bits: the clamp's upper bound is p.yuv_hi = 2^d - 1 and the stored sample is
// code << p.yuv_shift.  The 16 lanes of a tile row write 32 contiguous bytes of Y.  Frames, the chroma planes (OH*OW samples in) and rows are
// in general only 2-byte aligned, so Cb and Cr leave as two 2-byte stores in both layouts.
template <bool U8, bool CHW = false, int SPACE = SP_PIXEL, bool YUV = false, bool Y16 = false>
__global__ __launch_bounds__(256) void conv_last_k(const LastP p) {
    __shared__ __attribute__((aligned(16))) float s_g[27 * LAST_GP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int t = lane & 15, kq = lane >> 4;
    f32x4 wreg[2][4];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int c = 0; c < 4; ++c) wreg[blk][c] = *(const f32x4*)(p.w + ((blk * 4 + c) * 64 + lane) * 4);
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const float bias[3] = {p.bias[0], p.bias[1], p.bias[2]};
    const int ntiles = p.tiles_x * p.tiles_y * p.B;
    const int OH = p.out_H ? p.out_H : p.H, OW = p.out_H ? p.out_W : p.W;
    // Store addresses through the view, split as the loads are: a lane's pixel is (lrow, lcol) of EVERY tile, so its offset inside a tile's
    // rows of each plane is computed once, here; a tile adds its own origin in those planes (tile_org below: uniform, scalar arithmetic).
    // Planes: HWC one (3 elements per pixel); CHW R, G, B; YUV Y, then Cb | CbCr, then Cr — a chroma sample per 2^csy x 2^csx block.
    const int lrow = 4 * wave + (lane >> 4), lcol = lane & 15;
    constexpr int NPL = (YUV || CHW) ? 3 : 1;
    int64_t lane_off[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const bool chroma = YUV && k > 0;
        const int r = chroma ? lrow >> p.csy : lrow, c = chroma ? (lcol >> p.csx) * (k == 1 && p.yuv_nv12 ? 2 : 1) : (YUV || CHW) ? lcol : lcol * 3;
        lane_off[k] = (int64_t)((uint64_t)(uint32_t)r * p.v.pitch[k]) + c;
    }
    // element index in out_img of (lrow, lcol) = (0, 0) of the tile at frame b, delivered-frame pixel (cy0, cx0) (both even; negative left
    // and above the crop window, where no lane stores)
    auto tile_org = [&](int k, int b, int cy0, int cx0) -> int64_t {
        const bool chroma = YUV && k > 0;
        const int r = chroma ? cy0 >> p.csy : cy0, c = chroma ? (cx0 >> p.csx) * (k == 1 && p.yuv_nv12 ? 2 : 1) : (YUV || CHW) ? cx0 : cx0 * 3;
        return (int64_t)b * p.v.fs + p.v.off[k] + (int64_t)r * (int64_t)p.v.pitch[k] + c;
    };
    // Tile walk.  Workgroup w runs on XCD w % 8 (observed dispatch order; locality only): each XCD gets ONE contiguous band of
    // the tile list, and the workgroups of an XCD take consecutive tiles of it — horizontally adjacent tiles run on the same
    // XCD at the same time and the rows above / below a round or two apart, so the 18 x 18 halos (1.27x the tensor) are
    // fetched from HBM once and hit that XCD's L2 afterwards (round 3's round-robin over the XCDs measured 1.22x).
    int tile, tile_end, tile_step;
    if ((gridDim.x & 7) == 0) {
        const int band = (ntiles + 7) >> 3, xcd = blockIdx.x & 7;
        tile = xcd * band + (blockIdx.x >> 3); tile_step = gridDim.x >> 3;
        tile_end = (xcd + 1) * band < ntiles ? (xcd + 1) * band : ntiles;
    } else { tile = blockIdx.x; tile_step = gridDim.x; tile_end = ntiles; }
    auto origin_of = [&](int tl) {      // 64-bit tile origin (halo pixel (0,0) = ring pixel (y0, x0)); lane offsets are tile-relative and 32-bit
        const int tx = tl % p.tiles_x, ty = (tl / p.tiles_x) % p.tiles_y, b = tl / (p.tiles_x * p.tiles_y);
        return p.in + ((size_t)b * (size_t)(p.H + 2) + (ty + p.ty0) * 16) * (size_t)(p.W + 2) * 64 + (size_t)((tx + p.tx0) * 16) * 64 + 4 * kq;
    };
    auto halo_off = [&](int g) {
        int P = 16 * g + t;
        P = P < 324 ? P : 323;
        const int hy = P / 18, hx = P - 18 * hy;
        return (hy * (p.W + 2) + hx) * 64;
    };
    f32x4 x[4], xn[4];
    if (tile < tile_end) {               // the first tile's first group; every later tile's is requested under the previous tile's taps
        const float* src = origin_of(tile) + halo_off(wave);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = *(const f32x4*)(src + 16 * c);
    }
    for (; tile < tile_end; tile += tile_step) {
        const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, b = tile / (p.tiles_x * p.tiles_y);
        const int y0 = (ty + p.ty0) * 16, x0 = (tx + p.tx0) * 16;
        const float* in_t = origin_of(tile);
        const bool more = tile + tile_step < tile_end;
        const float* in_n = more ? origin_of(tile + tile_step) : in_t;
        // ---- G = W . in over the halo: 21 groups of 16 pixels, round-robin over the waves
        for (int g = wave; g < 21; g += 4) {
            if (g + 4 < 21) {                 // next group's pixels while this one is multiplied
                const float* src = in_t + halo_off(g + 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) xn[c] = *(const f32x4*)(src + 16 * c);
            } else if (more) {                // the NEXT tile's first group: its latency lies under this tile's taps and stores
                const float* src = in_n + halo_off(wave);
#pragma unroll
                for (int c = 0; c < 4; ++c) xn[c] = *(const f32x4*)(src + 16 * c);
            }
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int blk = 0; blk < 2; ++blk) acc[blk] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[blk][c][s], x[c][s], acc[blk], 0, 0, 0);
            // D: register i of lane (pixel t, row group kq) = row n = 16 blk + 4 kq + i of that pixel
            const int P = 16 * g + t;
            if (P < 324) {
#pragma unroll
                for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int n = 16 * blk + 4 * kq + i;
                        if (n < 27) s_g[n * LAST_GP + P] = acc[blk][i];
                    }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = xn[c];
        }
        __syncthreads();
        // ---- taps: one output pixel per lane (wave w = tile rows 4w .. 4w+3)
        const int row = 4 * wave + (lane >> 4), col = lane & 15;
        float o[3] = {bias[0], bias[1], bias[2]};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const float* gp = &s_g[(tap * 3) * LAST_GP + (row + ky) * 18 + col + kx];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] += gp[c * LAST_GP];
        }
        __syncthreads();                      // G is free for the next tile
        const int y = y0 + row, xx = x0 + col;
        if constexpr (YUV) {
            static_assert(U8 && !CHW && SPACE == SP_PIXEL, "the YUV form stores integer codes of the PIXEL values");
            typedef typename std::conditional<Y16, uint16_t, uint8_t>::type S;      // a stored sample
            const float hi = Y16 ? p.yuv_hi : 255.f;
            auto sample = [&](float v) -> S {      // clamp, round half to even, and (uint16 only) move the code to where the layout keeps it
                const float code = __builtin_rintf(fminf(fmaxf(v, 0.f), hi));
                if constexpr (Y16) return (S)((unsigned)code << p.yuv_shift);
                else return (S)code;
            };
            // every lane computes its pixel's three components: the chroma sums cross lanes, so they run before the bounds branch,
            // with all 64 lanes active (a lane outside the frame holds a value nobody uses)
            float im[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) im[c] = fminf(fmaxf(o[c] * sd[c] + mean[c], 0.f), 1.f) * 255.f;      // the float form's value
            const int cy = p.out_H ? y - p.crop_top : y, cx = p.out_H ? xx - p.crop_left : xx;
            float yuv[3];
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float rg = p.yuv_m[4 * k] * im[0] + p.yuv_m[4 * k + 1] * im[1];
                    const float rgb = rg + p.yuv_m[4 * k + 2] * im[2];
                    yuv[k] = rgb + p.yuv_m[4 * k + 3];
                }
            }
            // row sums first (lane ^ 1), then the two rows (lane ^ 16): ((tl + tr) + (bl + br)); a partner outside the frame is
            // replaced by this lane's own value, a row outside by this row's sum (the same bits as replicating both pixels)
            const bool right_in = cx + 1 < OW, below_in = cy + 1 < OH;
            float blk[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float c = yuv[k + 1];
                const float side = __shfl_xor(c, 1);
                float rs = c;
                if (p.csx) {
#pragma clang fp contract(off)
                    rs = c + (right_in ? side : c);
                }
                const float other = __shfl_xor(rs, 16);
                if (p.csy) {             // 4:2:0 (csy implies csx)
#pragma clang fp contract(off)
                    blk[k] = (rs + (below_in ? other : rs)) * 0.25f;
                } else if (p.csx) {      // 4:2:2: the pair mean (l + r) * 0.5f
#pragma clang fp contract(off)
                    blk[k] = rs * 0.5f;
                } else blk[k] = rs;      // 4:4:4: the pixel's own component
            }
            if (y < p.H && xx < p.W) {
                typedef float f32x3 __attribute__((ext_vector_type(3)));
                if (p.out_pre) *(f32x3*)(p.out_pre + (((size_t)b * p.H + y) * p.W + xx) * 3) = f32x3{o[0], o[1], o[2]};
                if (cy >= 0 && cy < OH && cx >= 0 && cx < OW) {
                    // sample stores: the 16 lanes of a tile row write 16 contiguous Y samples, its 8 even lanes 8 (I420) or 16 (NV12)
                    // chroma samples (4:4:4: all 16 lanes, 16 or 32); rows are OW samples and frames OH*OW + 2*CH*CW, in general not dword
                    // aligned, so a semi-planar Cb, Cr pair leaves as two sample stores in every chroma format
                    S* const fr = (S*)p.out_img;
                    const int cy0 = p.out_H ? y0 - p.crop_top : y0, cx0 = p.out_H ? x0 - p.crop_left : x0;      // the tile's origin in the delivered frame
                    fr[tile_org(0, b, cy0, cx0) + lane_off[0]] = sample(yuv[0]);
                    if (!((row & p.csy) | (col & p.csx))) {       // the block's top left pixel (cy, cx even: crop and tile origins are even)
                        const S cb = sample(blk[0]);
                        const S cr = sample(blk[1]);
                        const int64_t a1 = tile_org(1, b, cy0, cx0) + lane_off[1];
                        if (p.yuv_nv12) { fr[a1] = cb; fr[a1 + 1] = cr; }
                        else { fr[a1] = cb; fr[tile_org(2, b, cy0, cx0) + lane_off[2]] = cr; }
                    }
                }
            }
        } else if (y < p.H && xx < p.W) {
            typedef float f32x3 __attribute__((ext_vector_type(3)));
            if (p.out_pre) *(f32x3*)(p.out_pre + (((size_t)b * p.H + y) * p.W + xx) * 3) = f32x3{o[0], o[1], o[2]};
            float im[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (SPACE == SP_NORM) im[c] = o[c];
                else if constexpr (SPACE == SP_UNIT) im[c] = fminf(fmaxf(o[c] * sd[c] + mean[c], 0.f), 1.f);
                else im[c] = fminf(fmaxf(o[c] * sd[c] + mean[c], 0.f), 1.f) * 255.f;
            }
            const int cy = p.out_H ? y - p.crop_top : y, cx = p.out_H ? xx - p.crop_left : xx;
            const int cy0 = p.out_H ? y0 - p.crop_top : y0, cx0 = p.out_H ? x0 - p.crop_left : x0;      // the tile's origin in the delivered frame
            // RGB -> BGR; a lane stores its pixel's 12 bytes, a row of the tile leaves as one 192-byte burst (uint8: 3 bytes as one
            // short + one byte store, a 48-byte row; rows are OW * 3 bytes and in general not dword aligned — measured no slower
            // than the float form, into HBM and into page-locked host memory: profiles/u8_output_rate.json)
            // Planar: one store per plane; the 16 lanes of a tile row write 64 contiguous bytes of each plane (uint8: 16), three
            // streams instead of one 192-byte burst, and a plane row starts on a 64-byte line only where OW * 4 (uint8: OW) is a
            // multiple of 64 — DESIGN §4's misaligned line starts, up to half the write bandwidth of this 12 (3) B/pixel store.
            if constexpr (CHW) {
                if (cy >= 0 && cy < OH && cx >= 0 && cx < OW) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int64_t at = tile_org(c, b, cy0, cx0) + lane_off[c];
                        if constexpr (U8) ((uint8_t*)p.out_img)[at] = (uint8_t)__builtin_rintf(im[c]);
                        else ((float*)p.out_img)[at] = im[c];
                    }
                }
            } else if constexpr (U8) {
                if (cy >= 0 && cy < OH && cx >= 0 && cx < OW) {
                    uint8_t* q = (uint8_t*)p.out_img + (tile_org(0, b, cy0, cx0) + lane_off[0]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c] = (uint8_t)__builtin_rintf(im[2 - c]);      // im is in [0, 255] and never NaN
                }
            } else {
                if (cy >= 0 && cy < OH && cx >= 0 && cx < OW)
                    *(f32x3*)((float*)p.out_img + (tile_org(0, b, cy0, cx0) + lane_off[0])) = f32x3{im[2], im[1], im[0]};
            }
        }
    }
}

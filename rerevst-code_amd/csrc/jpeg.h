// jpeg.h — the plan, the tables, the header and the launch entries of the JPEG output stage (librerevst_jpeg.so; include/rerevst_hip.h
// "JPEG output").  This header is all the main library sees of the kernels (jpeg_k.h).  Everything here but the two launch entries is host
// arithmetic on a handful of integers: the same inline functions answer rrv_jpeg_tables / _bound / _plan and fill the kernels' parameters.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

constexpr int JP_B_MAX = 64;              // frames per launch (blockIdx.y)
constexpr int JP_HEADER_MAX = 640;        // room for the 629 header bytes in the kernel parameters
constexpr int JP_BLOCK_BITS = 1658;       // most bits a block can code to: 9 + 11 for the DC difference, 63 x (16 + 10) for the ACs
constexpr int JP_BLOCK_BYTES = 208;       // ... in whole bytes

// Annex K.1, natural order
constexpr uint8_t JP_Q_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                   14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t JP_Q_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// zigzag position -> natural index
constexpr uint8_t JP_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3: code counts per length 1..16, then the symbols in code order
constexpr uint8_t JP_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t JP_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t JP_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t JP_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// The coder's tables: entry = code | length << 16, indexed by the symbol; [0] luma, [1] chroma.  Built once on the host (jpeg_huff) and carried
// to the kernels in their parameters.
struct JpegHuff {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};
inline void jpeg_huff_one(const uint8_t* bits, const uint8_t* vals, uint32_t* tab) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) tab[vals[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
}
inline void jpeg_huff(JpegHuff* t) {
    memset(t, 0, sizeof *t);
    for (int c = 0; c < 2; ++c) {
        jpeg_huff_one(JP_DC_BITS[c], JP_DC_VALS, t->dc[c]);
        jpeg_huff_one(JP_AC_BITS[c], JP_AC_VALS[c], t->ac[c]);
    }
}

// What both halves are launched with.  The caller sets the pointers, B, cap and the three parameters; jpeg_fill works out the rest.
struct JpegP {
    const float* in;           // blocks: [B][H][W][3] float32 BGR PIXEL, contiguous
    int16_t* coef;             // [B][blocks][64], zigzag order, blocks in scan order: written by the first half, read by the second
    uint8_t* out;              // entropy: frame b's stream at out + b * cap
    int* sizes;                // [B]
    uint32_t* lens;            // [B][n_int] scratch: the stuffed bytes of every interval ...
    uint32_t* offs;            // [B][n_int] ... and where it starts in its frame's slot
    size_t cap;
    int B, H, W;
    int hs, vs;                // Y's sampling factors: 2 x 2, 2 x 1 or 1 x 1
    int mcu_cols, mcu_rows, mcus;
    int bpm;                   // blocks per MCU: hs * vs + 2
    int interval;              // MCUs per restart interval actually used
    int n_int;                 // intervals per frame
    int blocks;                // per frame
    int header_len;
    uint16_t q[2][64];         // the quantisers, natural order
    uint8_t zz_pos[64];        // natural index -> zigzag position
    float yuv_m[12];           // BT.601 full range, rrv_yuv_matrix's values
    uint8_t header[JP_HEADER_MAX];
    JpegHuff huff;
};

inline bool jpeg_chroma_ok(int chroma) { return chroma == 420 || chroma == 422 || chroma == 444; }
// IJG scaling of the Annex K tables
inline void jpeg_tables(int quality, uint16_t* luma, uint16_t* chroma) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (JP_Q_LUMA[i] * s + 50) / 100, c = (JP_Q_CHROMA[i] * s + 50) / 100;
        luma[i] = (uint16_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma[i] = (uint16_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
}
// the geometry of an H x W frame: false outside the ranges (H, W 1..65535; chroma; restart 0..65535, 0 = one MCU row per interval)
inline bool jpeg_plan(int H, int W, int chroma, int restart, JpegP* p) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || !jpeg_chroma_ok(chroma) || restart < 0 || restart > 65535) return false;
    p->H = H; p->W = W;
    p->hs = chroma == 444 ? 1 : 2; p->vs = chroma == 420 ? 2 : 1;
    p->mcu_cols = (W + 8 * p->hs - 1) / (8 * p->hs);
    p->mcu_rows = (H + 8 * p->vs - 1) / (8 * p->vs);
    p->mcus = p->mcu_cols * p->mcu_rows;
    p->bpm = p->hs * p->vs + 2;
    p->interval = restart ? restart : p->mcu_cols;
    p->n_int = (p->mcus + p->interval - 1) / p->interval;
    p->blocks = p->mcus * p->bpm;
    p->header_len = 629;
    return true;
}
// no stream of the plan's frame is longer: every block at its most bits with every byte stuffed, every interval's padding byte stuffed too
inline size_t jpeg_bound(const JpegP& p) {
    return (size_t)p.header_len + (size_t)p.blocks * (2 * JP_BLOCK_BYTES) + (size_t)p.n_int * 4 + 2;
}
// SOI .. SOS of the plan's frame at `quality`; returns the byte count (p->header_len)
inline int jpeg_header(JpegP* p) {
    uint8_t* h = p->header;
    int n = 0;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) h[n++] = (uint8_t)b; };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xDB, 0, 67, t});
        for (int i = 0; i < 64; ++i) h[n++] = (uint8_t)p->q[t][JP_ZIGZAG[i]];
    }
    put({0xFF, 0xC0, 0, 17, 8, p->H >> 8, p->H & 255, p->W >> 8, p->W & 255, 3, 1, p->hs << 4 | p->vs, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 12, c});
        for (int i = 0; i < 16; ++i) h[n++] = JP_DC_BITS[c][i];
        for (int i = 0; i < 12; ++i) h[n++] = JP_DC_VALS[i];
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 162, 0x10 | c});
        for (int i = 0; i < 16; ++i) h[n++] = JP_AC_BITS[c][i];
        for (int i = 0; i < 162; ++i) h[n++] = JP_AC_VALS[c][i];
    }
    put({0xFF, 0xDD, 0, 4, p->interval >> 8, p->interval & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return n;
}
// plan, quantisers, header and coder tables; false outside the ranges (quality 1..100 and jpeg_plan's)
inline bool jpeg_fill(JpegP* p, int H, int W, int chroma, int quality, int restart) {
    if (quality < 1 || quality > 100 || !jpeg_plan(H, W, chroma, restart, p)) return false;
    jpeg_tables(quality, p->q[0], p->q[1]);
    p->header_len = jpeg_header(p);
    jpeg_huff(&p->huff);
    for (int i = 0; i < 64; ++i) p->zz_pos[JP_ZIGZAG[i]] = (uint8_t)i;
    // rrv_yuv_matrix(RRV_YUV_BT601, full range): each coefficient evaluated in double and rounded once
    const double kr = 0.299, kb = 0.114, kg = 1.0 - kr - kb, y[3] = {kr, kg, kb};
    for (int c = 0; c < 3; ++c) {
        p->yuv_m[c] = (float)y[c];
        p->yuv_m[4 + c] = (float)(((c == 2 ? 1.0 : 0.0) - y[c]) / (2.0 * (1.0 - kb)));
        p->yuv_m[8 + c] = (float)(((c == 0 ? 1.0 : 0.0) - y[c]) / (2.0 * (1.0 - kr)));
    }
    p->yuv_m[3] = 0.f;
    p->yuv_m[7] = p->yuv_m[11] = 128.f;
    return true;
}

// First half: queues jpeg_blocks_k<hs, vs> on `stream` (p->in -> p->coef).  Second half: queues jpeg_entropy_k<0> (interval lengths), jpeg_place_k
// (offsets, sizes, header and EOI) and jpeg_entropy_k<1> (the intervals and their RST markers) (p->coef -> p->out, p->sizes, through p->lens and
// p->offs).  Both return the hipError_t of the launches as an int (0 = queued).
extern "C" int rrv_jpeg_blocks_launch(const JpegP* p, void* stream);
extern "C" int rrv_jpeg_entropy_launch(const JpegP* p, void* stream);

// jpeg_dec_k.h — the kernels of the JPEG input stage (include/rerevst_hip.h "JPEG input"), gfx950; part of jpeg_in.hip (librerevst_jpeg_in.so).
//
// jpeg_marks_k            one workgroup of 256 threads per frame.  A frame with restart intervals: the scan's bytes 256 at a time, a thread per
//     byte; a marker is FF followed by a byte that is neither 00 nor FF.  Wave ballots and a scan over the four waves' counts number the markers
//     in stream order.  Marker k < n_int - 1 must be RST(k & 7) and gives interval k + 1 its start; marker n_int - 1 (EOI, as a rule) ends the
//     scan and must not be a restart marker; what follows it is not looked at.  A frame without DRI has one interval and is not searched.
//     Writes status[b]: 0 or the marker code.
// jpeg_huff_k             one lane per (frame, restart interval), a wave of 64 intervals per workgroup, the frame's four decode tables in LDS.
//     A lane owns a bit reader over its interval's bytes (stuffed zeros skipped; FF followed by anything else ends the data) and decodes the
//     interval's MCUs: DC prediction from 0, run/size symbols, ZRL, EOB.  Only non-zero coefficients are stored (the launch entry cleared the
//     buffer).  Bounds: every symbol takes at least one bit, every loop runs over the interval's blocks and a block's 64 coefficients, never over
//     the data; beyond its bytes the reader hands out zeros and the block that used them ends the interval with JD_DATA.  A store's block index
//     is below the frame's blocks and its coefficient index below 64 by construction, whatever the bytes say.  A frame whose status
//     jpeg_marks_k set is skipped (its interval starts are not all written).
// jpeg_planes_k<HS, VS>   coefficient blocks -> the 8-bit planes.  256 threads take G = 32 / (blocks per MCU) consecutive MCUs, eight lanes per
//     block: a lane loads 16 bytes (eight zigzag coefficients), dequantises and scatters them into the block's natural 8 x 8 in LDS (blocks 72
//     floats apart: the eight blocks of a wave start in different banks); then owns a column (vertical pass), then a row (horizontal pass, two
//     16-byte LDS reads), adds 128, clamps, rounds half to even and stores the row's eight bytes as one 8-byte word where the address allows,
//     byte by byte at a ragged edge.  Rows and columns of the MCU padding are dropped.
// Every address is a size_t.  What the frame descriptors say is clamped against the call's own geometry before it addresses anything.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "jpeg_dec.h"

__constant__ const uint8_t jd_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the scan of frame b inside its slot: offset and length clamped to the slot
__device__ inline const uint8_t* jd_scan(const JpegDecP& p, const JpegDecFrame& f, int b, uint32_t* len) {
    const size_t off = f.scan_off < p.cap ? (size_t)f.scan_off : p.cap;
    const size_t n = (size_t)f.scan_len < p.cap - off ? (size_t)f.scan_len : p.cap - off;
    *len = (uint32_t)(n < 0xfffffff0u ? n : 0xfffffff0u);
    return p.streams + (size_t)b * p.cap + off;
}
__device__ inline int jd_intervals(const JpegDecP& p, const JpegDecFrame& f) { return f.n_int < 1 ? 1 : f.n_int > p.n_int_max ? p.n_int_max : f.n_int; }

__global__ __launch_bounds__(256) void jpeg_marks_k(const JpegDecP p) {
    __shared__ uint32_t s_cnt[2][4];
    __shared__ int s_err;
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const JpegDecFrame& f = p.frames[b];
    uint32_t len;
    const uint8_t* const s = jd_scan(p, f, b, &len);
    const int n_int = jd_intervals(p, f);
    uint32_t* const ivl = p.ivl + (size_t)b * (p.n_int_max + 1);
    if (n_int == 1) {
        if (tid == 0) { ivl[0] = 0; ivl[1] = len + 2; p.status[b] = JD_OK; }
        return;
    }
    if (tid == 0) { s_err = JD_OK; ivl[0] = 0; }
    __syncthreads();
    uint32_t total = 0;      // markers in front of this round's bytes: the same in every thread
    int round = 0;
    for (uint32_t base = 0; base < len && total < (uint32_t)n_int; base += 256, round ^= 1) {
        const uint32_t i = base + tid;
        uint32_t code = 0;
        bool mark = false;
        if (i + 1 < len && s[i] == 0xFF) {
            code = s[i + 1];
            mark = code != 0x00 && code != 0xFF;
        }
        const uint64_t m = __ballot(mark);
        if (lane == 0) s_cnt[round][wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = total;
        for (int w = 0; w < 4; ++w) {
            const uint32_t c = s_cnt[round][w];
            if (w < wave) before += c;
            total += c;
        }
        if (mark) {
            const uint32_t k = before + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            const bool rst = code >= 0xD0 && code <= 0xD7;
            if (k < (uint32_t)n_int - 1) {
                ivl[k + 1] = i + 2;
                if (code != 0xD0 + (k & 7)) atomicMax(&s_err, (int)JD_MARKER_WRONG);
            } else if (k == (uint32_t)n_int - 1) {
                ivl[n_int] = i + 2;
                if (rst) atomicMax(&s_err, (int)JD_MARKER_SURPLUS);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        int e = s_err;
        if (total < (uint32_t)n_int - 1 && e == JD_OK) e = JD_MARKER_MISSING;
        if (total < (uint32_t)n_int) ivl[n_int] = len + 2;
        p.status[b] = e;
    }
}

// A lane's bit reader.  acc holds n unread bits, the oldest on top; `real` counts those of them that came from the stream (the reader hands
// out zero bytes beyond the data, and a decoder that consumed one of those sees real < 0).
struct JdBits {
    const uint8_t* s;
    uint32_t pos, end;
    uint64_t acc;
    int n, real;
};
__device__ inline void jd_refill(JdBits& r) {      // n >= 57 afterwards; at most eight bytes
    while (r.n <= 56) {
        uint32_t byte = 0;
        if (r.pos < r.end) {
            byte = r.s[r.pos++];
            bool data = true;
            if (byte == 0xFF) {
                if (r.pos < r.end && r.s[r.pos] == 0x00) ++r.pos;    // a stuffed zero: FF is data
                else { r.pos = r.end; byte = 0; data = false; }      // a marker, fill bytes, or an FF that ends the interval (a fill byte in
            }                                                        // front of its marker: a data FF has its 00 inside the interval): the data ends here
            if (data) r.real += 8;
        }
        r.acc = (r.acc << 8) | byte;
        r.n += 8;
    }
}
__device__ inline uint32_t jd_take(JdBits& r, int k) {      // k in 0..16 of the n >= k unread bits
    r.n -= k; r.real -= k;
    return (uint32_t)(r.acc >> r.n) & ((1u << k) - 1);
}
// one symbol of table t (LDS), -1: no code of up to 16 bits matches
__device__ inline int jd_symbol(JdBits& r, const JpegDecTab& t) {
    const uint32_t v = (uint32_t)(r.acc >> (r.n - 16)) & 0xFFFFu;
    const uint32_t e = t.look[v >> 8];
    if (e) { r.n -= (int)(e >> 8); r.real -= (int)(e >> 8); return (int)(e & 255u); }
#pragma unroll 1
    for (int len = 9; len <= 16; ++len) {
        const int code = (int)(v >> (16 - len));
        if (code <= t.maxcode[len]) {
            r.n -= len; r.real -= len;
            return t.vals[(code + t.delta[len]) & 255];
        }
    }
    return -1;
}
__device__ inline int jd_extend(uint32_t bits, int size) { return size && bits < (1u << (size - 1)) ? (int)bits - (1 << size) + 1 : (int)bits; }

__global__ __launch_bounds__(64) void jpeg_huff_k(const JpegDecP p) {
    __shared__ JpegDecTab s_tab[4];
    const int lane = threadIdx.x, b = blockIdx.y;
    if (p.status[b] != JD_OK) return;      // (uniform: jpeg_marks_k refused the frame's markers)
    const JpegDecFrame& f = p.frames[b];
    {
        const uint32_t* const src = reinterpret_cast<const uint32_t*>(f.tab);
        uint32_t* const dst = reinterpret_cast<uint32_t*>(s_tab);
        for (int i = lane; i < (int)(sizeof(s_tab) / 4); i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const int n_int = jd_intervals(p, f);
    const int it = blockIdx.x * 64 + lane;
    if (it >= n_int) return;
    const int interval = f.interval < 1 ? 1 : f.interval;
    const long m0 = (long)it * interval;
    if (m0 >= p.mcus) return;
    const int nm = (int)(p.mcus - m0 < interval ? p.mcus - m0 : interval);
    uint32_t len;
    const uint8_t* const s = jd_scan(p, f, b, &len);
    const uint32_t* const ivl = p.ivl + (size_t)b * (p.n_int_max + 1);
    const uint32_t a = ivl[it] < len ? ivl[it] : len;
    uint32_t e = ivl[it + 1] >= 2 ? ivl[it + 1] - 2 : 0;
    e = e < a ? a : e > len ? len : e;
    JdBits r{s, a, e, 0, 0, 0};
    const int ny = p.bpm - 2;      // (grey: bpm = 1, every block is component 0)
    int16_t* const coef = p.coef + ((size_t)b * p.blocks + (size_t)m0 * p.bpm) * 64;
    int pred[3] = {0, 0, 0};
    int err = JD_OK;
#pragma unroll 1
    for (int k = 0; k < nm * p.bpm && err == JD_OK; ++k) {      // (m0 * bpm + k < blocks: m0 + nm <= mcus)
        const int j = k % p.bpm;
        const int c = p.ncomp == 1 || j < ny ? 0 : j - ny + 1;
        int16_t* const blk = coef + (size_t)k * 64;
        const JpegDecTab& dc = s_tab[f.tdc[c] & 1];
        const JpegDecTab& ac = s_tab[2 + (f.tac[c] & 1)];
        jd_refill(r);
        const int sz = jd_symbol(r, dc);
        if (sz < 0) { err = JD_CODE; break; }
        if (sz > 11) { err = JD_CATEGORY; break; }
        pred[c] += jd_extend(jd_take(r, sz), sz);
        if (pred[c]) blk[0] = (int16_t)pred[c];
        int z = 1;
#pragma unroll 1
        while (z < 64) {
            jd_refill(r);
            const int rs = jd_symbol(r, ac);
            if (rs < 0) { err = JD_CODE; break; }
            const int run = rs >> 4, size = rs & 15;
            if (size == 0) {
                if (run != 15) break;      // EOB
                z += 16;                   // ZRL
                continue;
            }
            if (size > 10) { err = JD_CATEGORY; break; }
            z += run;
            if (z > 63) { err = JD_RUN; break; }
            blk[z++] = (int16_t)jd_extend(jd_take(r, size), size);      // (never 0: a category's values exclude it)
        }
        if (err == JD_OK && r.real < 0) err = JD_DATA;
    }
    if (err != JD_OK) atomicCAS(&p.status[b], (int)JD_OK, err);
}

// 8-point inverse DCT with JPEG's normalisation: s[x] = sum_u C(u)/2 F[u] cos((2x+1) u pi / 16), in place
__device__ inline void jd_idct8(float* s) {
    constexpr float c1 = 0.49039264020161522f, c2 = 0.46193976625564337f, c3 = 0.41573480615127262f, c4 = 0.35355339059327376f,
                    c5 = 0.27778511650980111f, c6 = 0.19134171618254489f, c7 = 0.09754516100806413f;
    const float t0 = c4 * (s[0] + s[4]), t1 = c4 * (s[0] - s[4]);
    const float t2 = c2 * s[2] + c6 * s[6], t3 = c6 * s[2] - c2 * s[6];
    const float e0 = t0 + t2, e3 = t0 - t2, e1 = t1 + t3, e2 = t1 - t3;
    const float o0 = c1 * s[1] + c3 * s[3] + c5 * s[5] + c7 * s[7];
    const float o1 = c3 * s[1] - c7 * s[3] - c1 * s[5] - c5 * s[7];
    const float o2 = c5 * s[1] - c1 * s[3] + c7 * s[5] + c3 * s[7];
    const float o3 = c7 * s[1] - c5 * s[3] + c3 * s[5] - c1 * s[7];
    s[0] = e0 + o0; s[7] = e0 - o0;
    s[1] = e1 + o1; s[6] = e1 - o1;
    s[2] = e2 + o2; s[5] = e2 - o2;
    s[3] = e3 + o3; s[4] = e3 - o3;
}

// eight bytes of a plane row: one 8-byte store when all eight are inside the row and the address allows it
__device__ inline void jd_store_row(uint8_t* row, int x0, int PW, uint32_t lo, uint32_t hi) {
    const int n = PW - x0 < 8 ? PW - x0 : 8;
    uint8_t* const d = row + x0;
    if (n == 8 && ((uintptr_t)d & 7) == 0) {
        *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
    } else {
        for (int i = 0; i < n; ++i) d[i] = (uint8_t)((i < 4 ? lo >> (8 * i) : hi >> (8 * (i - 4))) & 255u);
    }
}

constexpr int JD_BLK_STRIDE = 72;      // floats between the blocks in LDS

template <int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_planes_k(const JpegDecP p) {
    __shared__ __attribute__((aligned(16))) float s_t[32 * JD_BLK_STRIDE];
    __shared__ float s_q[3][64];      // zigzag order
    __shared__ uint8_t s_zz[64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int bpm = p.ncomp == 1 ? 1 : HS * VS + 2, ny = bpm - 2;
    const int G = 32 / bpm;
    const int m0 = blockIdx.x * G;
    const int ng = min(G, p.mcus - m0);      // (>= 1: the grid is ceil(mcus / G))
    const JpegDecFrame& f = p.frames[b];
    if (tid < 192) s_q[tid >> 6][tid & 63] = (float)f.q[tid >> 6][tid & 63];
    if (tid < 64) s_zz[tid] = jd_zigzag[tid];
    __syncthreads();
    const int blk = tid >> 3, r = tid & 7;
    const int g = blk / bpm, j = blk - g * bpm;
    const bool live = g < ng;
    const int c = p.ncomp == 1 || j < ny ? 0 : j - ny + 1;
    float* const t = s_t + blk * JD_BLK_STRIDE;
    if (live) {
        const uint4 v = *reinterpret_cast<const uint4*>(p.coef + ((size_t)b * p.blocks + (size_t)m0 * bpm + blk) * 64 + r * 8);
        const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int z = r * 8 + i;
            t[s_zz[z]] = (float)(int)(int16_t)(ws[i >> 1] >> (16 * (i & 1))) * s_q[c][z];
        }
    }
    __syncthreads();
    float s[8];
    if (live) {      // column r: the vertical pass
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = t[i * 8 + r];
        jd_idct8(s);
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i * 8 + r] = s[i];
    }
    __syncthreads();
    if (!live) return;
    {      // row r: the horizontal pass
        const float4 a = *reinterpret_cast<const float4*>(t + r * 8), d = *reinterpret_cast<const float4*>(t + r * 8 + 4);
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = d.x; s[5] = d.y; s[6] = d.z; s[7] = d.w;
    }
    jd_idct8(s);
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i >> 2] |= (uint32_t)__builtin_rintf(fminf(fmaxf(s[i] + 128.f, 0.f), 255.f)) << (8 * (i & 3));
    const int m = m0 + g, my = m / p.mcu_cols, mx = m - my * p.mcu_cols;
    uint8_t* const frame = p.planes + (size_t)b * p.frame_bytes;
    const size_t ysz = (size_t)p.H * p.W, csz = (size_t)p.CH * p.CW;
    if (p.ncomp == 1) {      // grey: an I444 frame, the chroma planes hold 128
        const int y = my * 8 + r, x0 = mx * 8;
        if (y < p.H && x0 < p.W) {
            jd_store_row(frame + (size_t)y * p.W, x0, p.W, w[0], w[1]);
            jd_store_row(frame + ysz + (size_t)y * p.W, x0, p.W, 0x80808080u, 0x80808080u);
            jd_store_row(frame + 2 * ysz + (size_t)y * p.W, x0, p.W, 0x80808080u, 0x80808080u);
        }
    } else if (c == 0) {
        const int y = (my * VS + j / HS) * 8 + r, x0 = (mx * HS + j % HS) * 8;
        if (y < p.H && x0 < p.W) jd_store_row(frame + (size_t)y * p.W, x0, p.W, w[0], w[1]);
    } else {
        const int y = my * 8 + r, x0 = mx * 8;
        if (y < p.CH && x0 < p.CW) jd_store_row(frame + ysz + (size_t)(c - 1) * csz + (size_t)y * p.CW, x0, p.CW, w[0], w[1]);
    }
}

// jpeg_k.h — the kernels of the JPEG output stage (include/rerevst_hip.h "JPEG output"), gfx950; part of jpeg.hip (librerevst_jpeg.so).
//
// jpeg_blocks_k<HS, VS>   float32 BGR PIXEL frames -> quantised coefficient blocks, int16, zigzag order, blocks in scan order.  A workgroup of
//     256 threads takes G = 32 / (HS VS + 2) consecutive MCUs of one frame (5, 8 or 10: at most 32 blocks).  Their pixels are read once into
//     LDS, rows and columns beyond the frame taking the last row / column.  Then eight lanes own a block, one row each: the row's eight
//     samples (Y: the clamped, rounded c_0; chroma: the clamped, rounded box mean of the unrounded c_k, a sample beyond the chroma plane
//     repeating the plane's last) minus 128, the row transform in registers, a transpose through LDS, the column transform, the division by
//     the quantiser, rint.  The G MCUs' blocks are contiguous in the output and leave LDS as one run of 32-bit words.
// jpeg_entropy_k<WRITE>   one wave per restart interval.  64 blocks at a time: every lane measures its block's code (DC difference against the
//     previous block of its component inside the interval, read from the coefficient array; run/size symbols, ZRL, EOB), a wave prefix sum
//     places the blocks, LDS words are cleared and every lane ORs its bits in.  Then a byte pass over the chunk's whole bytes counts the 0xFF
//     bytes in front of every lane (ballot) and, with WRITE, stores the bytes and their 0x00 stuffing; up to seven bits carry over to the
//     next chunk, the last one is padded with 1-bits.  WRITE = 0 only counts: lens[b][i] = the interval's stuffed bytes.  WRITE = 1 stores
//     at the offset jpeg_place_k gave the interval and appends RSTn; a frame that did not fit (sizes[b] < 0) is skipped.
// jpeg_place_k            one workgroup per frame: exclusive scan of the interval lengths (plus two bytes of RST marker behind all but the
//     last), the frame's size against cap, the header and EOI.
// Every address is a size_t.  Nothing here depends on what lens, offs or LDS held before: each word read was written by the same call.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "jpeg.h"

// c_k of a BGR pixel: ((m0 R + m1 G) + m2 B) + m3, every operation rounded ("Output size")
__device__ inline float jp_comp(const float* m, int k, const float* px) {
#pragma clang fp contract(off)
    const float rg = m[4 * k] * px[2] + m[4 * k + 1] * px[1];
    const float rgb = rg + m[4 * k + 2] * px[0];
    return rgb + m[4 * k + 3];
}
__device__ inline float jp_mean4(float tl, float tr, float bl, float br) {
#pragma clang fp contract(off)
    return ((tl + tr) + (bl + br)) * 0.25f;
}
__device__ inline float jp_mean2(float l, float r) {
#pragma clang fp contract(off)
    return (l + r) * 0.5f;
}
__device__ inline float jp_sample(float v) { return __builtin_rintf(fminf(fmaxf(v, 0.f), 255.f)) - 128.f; }

// 8-point DCT-II with JPEG's normalisation per axis: F[u] = C(u)/2 sum_x s[x] cos((2x+1) u pi / 16), in place
__device__ inline void jp_dct8(float* s) {
    constexpr float c1 = 0.49039264020161522f, c2 = 0.46193976625564337f, c3 = 0.41573480615127262f, c4 = 0.35355339059327376f,
                    c5 = 0.27778511650980111f, c6 = 0.19134171618254489f, c7 = 0.09754516100806413f;
    const float a0 = s[0] + s[7], a1 = s[1] + s[6], a2 = s[2] + s[5], a3 = s[3] + s[4];
    const float b0 = s[0] - s[7], b1 = s[1] - s[6], b2 = s[2] - s[5], b3 = s[3] - s[4];
    const float e0 = a0 + a3, e1 = a1 + a2, d0 = a0 - a3, d1 = a1 - a2;
    s[0] = c4 * (e0 + e1);
    s[4] = c4 * (e0 - e1);
    s[2] = c2 * d0 + c6 * d1;
    s[6] = c6 * d0 - c2 * d1;
    s[1] = c1 * b0 + c3 * b1 + c5 * b2 + c7 * b3;
    s[3] = c3 * b0 - c7 * b1 - c1 * b2 - c5 * b3;
    s[5] = c5 * b0 - c1 * b1 + c7 * b2 + c3 * b3;
    s[7] = c7 * b0 - c5 * b1 + c3 * b2 - c1 * b3;
}

template <int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_blocks_k(const JpegP p) {
    constexpr int MW = 8 * HS, MH = 8 * VS, NY = HS * VS, BPM = NY + 2, G = 32 / BPM, MPX = MW * MH;
    __shared__ float s_px[G * MPX * 3];      // the workgroup's MCUs, BGR as read
    __shared__ float s_t[256 * 9];           // row-transformed blocks: thread t's eight values at 9 t
    __shared__ int16_t s_c[32 * 64];
    __shared__ float s_q[2][64];
    __shared__ float s_m[12];
    __shared__ uint8_t s_zz[64];             // natural index -> zigzag position
    __shared__ int s_my[G], s_mx[G];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int m0 = blockIdx.x * G;
    const int ng = min(G, p.mcus - m0);      // (>= 1: the grid is ceil(mcus / G))
    if (tid < 128) s_q[tid >> 6][tid & 63] = (float)p.q[tid >> 6][tid & 63];
    if (tid < 64) s_zz[tid] = p.zz_pos[tid];
    if (tid < 12) s_m[tid] = p.yuv_m[tid];
    if (tid < ng) {
        const int m = m0 + tid, my = m / p.mcu_cols;
        s_my[tid] = my; s_mx[tid] = m - my * p.mcu_cols;
    }
    __syncthreads();
    const float* const in = p.in + (size_t)b * (size_t)p.H * (size_t)p.W * 3;
    for (int e = tid; e < ng * MPX * 3; e += 256) {
        const int g = e / (MPX * 3), r = e - g * (MPX * 3);
        const int y = r / (MW * 3), xe = r - y * (MW * 3);
        const int x = xe / 3, ch = xe - x * 3;
        const int gy = min(s_my[g] * MH + y, p.H - 1), gx = min(s_mx[g] * MW + x, p.W - 1);
        s_px[e] = in[((size_t)gy * p.W + gx) * 3 + ch];
    }
    __syncthreads();

    const int blk = tid >> 3, r = tid & 7;
    const int g = blk / BPM, j = blk - g * BPM;
    const bool live = blk < ng * BPM;
    float s[8];
    if (live) {
        const float* const px = s_px + g * MPX * 3;
        if (j < NY) {
            const int y = (j / HS) * 8 + r, x0 = (j % HS) * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] = jp_sample(jp_comp(s_m, 0, px + (y * MW + x0 + i) * 3));
        } else {
            const int k = j - NY + 1;
            const int CH = (p.H + VS - 1) / VS, CW = (p.W + HS - 1) / HS;
            const int nr = min(8, CH - s_my[g] * 8), nc = min(8, CW - s_mx[g] * 8);      // the MCU's rows and columns inside the chroma plane (>= 1)
            const int y = min(r, nr - 1) * VS;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int x = min(i, nc - 1) * HS;
                const float* const q = px + (y * MW + x) * 3;      // (the pixel right of / below it is in the MCU, clamped to the frame as read)
                float v;
                if constexpr (HS == 2 && VS == 2) v = jp_mean4(jp_comp(s_m, k, q), jp_comp(s_m, k, q + 3), jp_comp(s_m, k, q + MW * 3), jp_comp(s_m, k, q + MW * 3 + 3));
                else if constexpr (HS == 2) v = jp_mean2(jp_comp(s_m, k, q), jp_comp(s_m, k, q + 3));
                else v = jp_comp(s_m, k, q);
                s[i] = jp_sample(v);
            }
        }
        jp_dct8(s);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_t[tid * 9 + i] = s[i];
    }
    __syncthreads();
    if (live) {      // lane r now owns column r of its block: horizontal frequency r
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = s_t[(blk * 8 + i) * 9 + r];
        jp_dct8(s);
        const float* const q = s_q[j < NY ? 0 : 1];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int n = v * 8 + r;
            const float c = __builtin_rintf(s[v] / q[n]);
            s_c[blk * 64 + s_zz[n]] = (int16_t)fminf(fmaxf(c, n ? -1023.f : -1024.f), 1023.f);
        }
    }
    __syncthreads();
    uint32_t* const dst = reinterpret_cast<uint32_t*>(p.coef + ((size_t)b * p.blocks + (size_t)m0 * BPM) * 64);
    const uint32_t* const src = reinterpret_cast<const uint32_t*>(s_c);
    for (int i = tid; i < ng * BPM * 32; i += 256) dst[i] = src[i];
}

__device__ inline int jp_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// The code of one block (eight 16-byte loads of zigzag int16), DC predicted by `pred`: returns its length in bits and, with EMIT, ORs the bits
// into the cleared big-endian words `lds` from bit `pos` on.  A DC outside -1024..1023 or an AC outside -1023..1023 is coded as the nearest end.
template <bool EMIT>
__device__ inline int jp_code_block(const uint4* blk, int pred, const uint32_t* dc_tab, const uint32_t* ac_tab, uint32_t* lds, int pos) {
    int bits = 0, na = pos & 31;
    uint64_t acc = 0;
    uint32_t* w = lds + (pos >> 5);
    auto emit = [&](uint32_t code, int len) {      // len <= 27
        bits += len;
        if constexpr (EMIT) {
            acc = (acc << len) | code;
            na += len;
            if (na >= 32) {
                atomicOr(w++, (uint32_t)(acc >> (na - 32)));
                na -= 32;
                acc &= (1ull << na) - 1;
            }
        }
    };
    auto symbol = [&](uint32_t t, int v, int sz) {      // a table entry, then the sz low bits of v (v - 1 when negative)
        const uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << sz) - 1);
        emit(((t & 0xFFFFu) << sz) | low, (int)(t >> 16) + sz);
    };
    int run = 0;
#pragma unroll 1
    for (int v4 = 0; v4 < 8; ++v4) {
        const uint4 q = blk[v4];
        const uint32_t ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            int v = (int)(int16_t)(ws[h >> 1] >> (16 * (h & 1)));
            if (v4 == 0 && h == 0) {
                const int d = jp_clamp(v, -1024, 1023) - pred;
                const int sz = d ? 32 - __clz(d < 0 ? -d : d) : 0;
                symbol(dc_tab[sz], d, sz);
                continue;
            }
            v = jp_clamp(v, -1023, 1023);
            if (v == 0) { ++run; continue; }
            while (run >= 16) { const uint32_t t = ac_tab[0xF0]; emit(t & 0xFFFFu, (int)(t >> 16)); run -= 16; }
            const int sz = 32 - __clz(v < 0 ? -v : v);
            symbol(ac_tab[run << 4 | sz], v, sz);
            run = 0;
        }
    }
    if (run) { const uint32_t t = ac_tab[0]; emit(t & 0xFFFFu, (int)(t >> 16)); }
    if constexpr (EMIT) if (na) atomicOr(w, (uint32_t)(acc << (32 - na)));
    return bits;
}

constexpr int JP_CHUNK_WORDS = (64 * JP_BLOCK_BITS + 7 + 7 + 31) / 32 + 1;      // 64 blocks at their most, the carry in front, the padding behind, and one

template <int WRITE>
__global__ __launch_bounds__(64) void jpeg_entropy_k(const JpegP p) {
    __shared__ uint32_t s_bits[JP_CHUNK_WORDS];
    __shared__ uint32_t s_dc[2][12], s_ac[2][256];
    const int lane = threadIdx.x, it = blockIdx.x, b = blockIdx.y;
    if (WRITE && p.sizes[b] < 0) return;      // the frame did not fit: nothing of it is written
    for (int i = lane; i < 24; i += 64) s_dc[i / 12][i % 12] = p.huff.dc[i / 12][i % 12];
    for (int i = lane; i < 512; i += 64) s_ac[i >> 8][i & 255] = p.huff.ac[i >> 8][i & 255];
    const int bpm = p.bpm, ny = bpm - 2;
    const int ma = it * p.interval;
    const int nb = min(p.interval, p.mcus - ma) * bpm;      // blocks of the interval (>= bpm)
    const size_t kb0 = (size_t)b * p.blocks + (size_t)ma * bpm;
    const int16_t* const coef = p.coef + kb0 * 64;
    uint8_t* const dst = WRITE ? p.out + (size_t)b * p.cap + p.offs[(size_t)b * p.n_int + it] : nullptr;
    uint32_t carry_val = 0, out_len = 0;
    int carry_n = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += 64) {
        const int k = c0 + lane;
        const bool live = k < nb;
        int pred = 0, comp = 0, len = 0;
        const uint4* const blk = reinterpret_cast<const uint4*>(coef + (size_t)(live ? k : 0) * 64);      // (a dead lane: block 0, never read)
        if (live) {
            const int m = k / bpm, j = k - m * bpm;
            comp = j < ny ? 0 : 1;
            // the previous block of the component inside the interval: Y's are consecutive in an MCU, then the last Y of the MCU before
            const int kp = j < ny ? (j > 0 ? k - 1 : m > 0 ? k - bpm + ny - 1 : -1) : (m > 0 ? k - bpm : -1);
            if (kp >= 0) pred = jp_clamp(coef[(size_t)kp * 64], -1024, 1023);
            len = jp_code_block<false>(blk, pred, s_dc[comp], s_ac[comp], nullptr, 0);
        }
        int inc = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        int tbits = carry_n + __shfl(inc, 63);
        const bool last = c0 + 64 >= nb;
        const int pad = last ? (8 - (tbits & 7)) & 7 : 0;
        const int nwords = min(((tbits + pad + 31) >> 5) + 1, JP_CHUNK_WORDS);
        for (int i = lane; i < nwords; i += 64) s_bits[i] = 0;
        __syncthreads();
        if (lane == 0 && carry_n) atomicOr(&s_bits[0], carry_val << (32 - carry_n));
        if (live) jp_code_block<true>(blk, pred, s_dc[comp], s_ac[comp], s_bits, carry_n + inc - len);
        if (lane == 0 && pad) atomicOr(&s_bits[tbits >> 5], ((1u << pad) - 1) << (32 - (tbits & 31) - pad));      // (the padding ends its byte, so its word)
        tbits += pad;
        __syncthreads();
        const int nbytes = tbits >> 3;
        carry_n = tbits & 7;
        if (carry_n) carry_val = ((s_bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xFFu) >> (8 - carry_n);
        for (int i0 = 0; i0 < nbytes; i0 += 64) {
            const int i = i0 + lane;
            const bool ok = i < nbytes;
            const uint32_t byte = ok ? (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu : 0u;
            const bool ff = ok && byte == 0xFFu;
            const uint64_t mask = __ballot(ff);
            if (WRITE && ok) {
                uint8_t* const d = dst + out_len + lane + __popcll(mask & ((1ull << lane) - 1));
                d[0] = (uint8_t)byte;
                if (ff) d[1] = 0;
            }
            out_len += (uint32_t)min(64, nbytes - i0) + (uint32_t)__popcll(mask);
        }
        __syncthreads();
    }
    if (WRITE) {
        if (lane == 0 && it < p.n_int - 1) { dst[out_len] = 0xFF; dst[out_len + 1] = (uint8_t)(0xD0 + (it & 7)); }
    } else if (lane == 0) {
        p.lens[(size_t)b * p.n_int + it] = out_len;
    }
}

__global__ __launch_bounds__(256) void jpeg_place_k(const JpegP p) {
    __shared__ uint32_t s_scan[256];
    const int tid = threadIdx.x, b = blockIdx.x, n = p.n_int;
    const uint32_t* const lens = p.lens + (size_t)b * n;
    uint32_t* const offs = p.offs + (size_t)b * n;
    uint64_t base = (uint64_t)p.header_len;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const uint32_t v = i < n ? lens[i] + (i < n - 1 ? 2u : 0u) : 0u;
        s_scan[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t t = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += t;
            __syncthreads();
        }
        if (i < n) offs[i] = (uint32_t)(base + s_scan[tid] - v);
        base += s_scan[255];
        __syncthreads();
    }
    const uint64_t total = base + 2;      // EOI
    const bool fits = total <= (uint64_t)p.cap;
    if (tid == 0) p.sizes[b] = fits ? (int)total : -(int)total;
    if (!fits) return;
    uint8_t* const o = p.out + (size_t)b * p.cap;
    for (int i = tid; i < p.header_len; i += 256) o[i] = p.header[i];
    if (tid == 0) { o[total - 2] = 0xFF; o[total - 1] = 0xD9; }
}

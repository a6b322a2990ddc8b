// conv_ups5.h — ResidualBlock.conv1 behind the nearest-x2 upsample WITH the block's 1x1 shortcut (conv_wino_k<.., UPS = 1,
// SC = 1>): five products per two low-resolution pixels and axis, 25 + 4 GEMM positions per 2x2 low-resolution pixels
// (4x4 outputs) instead of 4 x 10.
//
// Per axis, low-resolution x0..x3 (x1, x2 the tile's pixels) and y0..y3 = the four outputs of "nearest x2, then 3-tap
// conv g": y = A^T [(G g) .* (B^T x)] with
//   G   = [[1,0,0], [.5,.5,.5], [-.5,-.5,.5], [-.5,.5,.5], [0,0,1]]
//   B^T = [[1,0,-1,0], [0,1,1,0], [0,-1,1,0], [0,-1,1,0], [0,-1,0,1]]      (rows 2 and 3 are the same: 4 distinct values)
//   A^T = [[1,1,0,-1,0], [0,1,1,0,0], [0,1,0,1,0], [0,1,-1,0,1]]
// (rank 5 of the 4-DOF sequence (x0,x1,x1,x2,x2,x3) against g; tools/ups5_search.py derives the family and ranks its
// members by an fp32 error study; tests/test_ups5_transform.py checks the table in float64).  Data and output transforms
// are additions only, the weight transform halves (exact).  In 2-D: V = B^T d B has 16 distinct values per tile and
// channel, M[i][j] = U[i][j] V[s(i)][s(j)], s = (0,1,2,2,3).
// The shortcut: x1 = (m - d)/2, x2 = (m + d)/2 with m = x1 + x2, d = x2 - x1 (slots 1 and 2), so the four centre pixels
// are a Hadamard combination of V[m|d][m|d]: four GEMMs with ONE weight block (the shortcut weights / 4), combined in
// the epilogue.  Outputs: the low-resolution shortcut tensor that conv2's epilogue adds (E_RES_UPS).
//
// Mapping: a tile = 2x2 low-resolution pixels (4x4 patch, halo 1) -> 4x4 outputs.  v_mfma_f32_16x16x4_f32 with
// M = 16 couts, N = 16 tiles, K = 4 channels, as in conv_wino.h.  4 waves, each 16 tiles (2 x 8) x 32 couts: a
// workgroup is 16x16 low-resolution pixels (32x32 outputs, 18x18 halo, the LDS image of conv_wino_split_k) x 32 couts.
// Registers: 29 positions x 2 cout blocks x 4 = 232 accumulators, two 64-register V arrays (current chunk, next chunk
// transformed in place), 32 for U fragments in flight: ~420, so one wave per SIMD (MI355X_MICROARCH §Register files:
// 264-512 registers -> 1 wave).  16 couts per wave (116 accumulators) would allow two waves per SIMD only below 256
// registers, which the two V arrays alone make impossible, and would double the transform work per MFMA.
// LDS: U 26 blocks x 2 KB = 52 KB per chunk (positions 25..28 share one block), raw halo 24 KB, both double buffered,
// + 2 KB epilogue parameters = 154 KB: one workgroup per CU.
// Pipeline as conv_wino_k: the transformed input is the MFMA B operand (never stored), LDS-DMA double buffering, the
// next chunk's patch read and transformed under the current chunk's MFMAs with counted waits, persistent XCD-aware
// item walk whose consecutive K loops form one stream.
#pragma once      // included by conv_wino.h after its helpers

// THE coefficient table of the form: the weight pack, the input transform and the output transform below are generated
// from these arrays (tests/test_ups5_transform.py reads the same three arrays).  G2 = 2 G; BT4 = the four distinct rows of
// B^T (data slots a, m, d, e; product row r reads slot DS[r]); AT = A^T.
struct Ups5Tab {
    static constexpr int G2[5][3] = {{2, 0, 0}, {1, 1, 1}, {-1, -1, 1}, {-1, 1, 1}, {0, 0, 2}};
    static constexpr int BT4[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, -1, 0, 1}};
    static constexpr int AT[4][5] = {{1, 1, 0, -1, 0}, {0, 1, 1, 0, 0}, {0, 1, 0, 1, 0}, {0, 1, -1, 0, 1}};
    static constexpr int DS[5] = {0, 1, 2, 2, 3};
};
template <int T, int R>
constexpr int ups5_coef(int k) { return T == 0 ? Ups5Tab::BT4[R][k] : Ups5Tab::AT[R][k]; }
// row R of BT4 (T = 0) or AT (T = 1) applied to x: one addition or subtraction per further non-zero coefficient, starting
// from the first +1 (every row has one)
template <int T, int R, int N>
__device__ __forceinline__ f32x4 ups5_comb(const f32x4 (&x)[N]) {
    constexpr int F = [] { for (int k = 0; k < N; ++k) if (ups5_coef<T, R>(k) == 1) return k; return -1; }();
    static_assert(F >= 0, "every row has a +1 coefficient");
    f32x4 r = x[F];
    static_for([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        constexpr int c = ups5_coef<T, R>(k);
        static_assert(c == 0 || c == 1 || c == -1, "0 / +-1 coefficients");
        if constexpr (k != F && c == 1) r = e4add(r, x[k]);
        else if constexpr (c == -1) r = f4sub(r, x[k]);
    }, std::make_integer_sequence<int, N>{});
    return r;
}

struct Ups5Geo {
    static constexpr int NT = 256, NB = 2;
    static constexpr int NPOS = 29;                          // GEMM positions: 25 upsample-conv + 4 shortcut
    static constexpr int NUB = 26;                           // U blocks per chunk: positions 25..28 share block 25
    static constexpr int NPIECE = 16;                        // 4x4 patch pieces, index dx*4 + dy
    static constexpr int HALO = 18, HALF = 18 * 9;           // halo pixels in even (= odd) columns
    static constexpr int PIECES = HALO * HALO * 4;
    static constexpr int RAW_IT = (PIECES + NT - 1) / NT;    // 6
    static constexpr int RAW_BYTES = RAW_IT * NT * 16;       // 24576 (the disabled tail of the last slot writes zeros)
    static constexpr int U_BYTES = NUB * 32 * 16 * 4;        // 53248
    static constexpr int U_IT = U_BYTES / 16 / NT;           // 13, no partial slot
    static_assert(U_IT * NT * 16 == U_BYTES, "U image is a whole number of LDS-DMA rounds");
    static constexpr int SMEM = 2 * RAW_BYTES + 2 * U_BYTES + WINO_PAR_BYTES;   // 157696
    static_assert(SMEM <= 160 * 1024, "LDS");
    static constexpr int OCC = 1;
    // V index (kx*4 + ry) of GEMM position i
    static constexpr int vidx(int i) { return i < 25 ? Ups5Tab::DS[i % 5] * 4 + Ups5Tab::DS[i / 5] : (i == 25 ? 5 : i == 26 ? 9 : i == 27 ? 6 : 10); }
    // LDS read schedule: iteration i issues U(i+2) (2 reads, i+2 < NUB) and patch piece i (i < 16); LDS returns in order
    static constexpr int issued(int j) { return (j + 2 < NUB ? 2 : 0) + (j < NPIECE ? 1 : 0); }
    static constexpr int younger(int i) {      // reads younger than U(i) when iteration i waits for it
        return i == 0 ? 2 + issued(0) : i == 1 ? issued(0) + issued(1) : (i - 2 < NPIECE ? 1 : 0) + issued(i - 1) + issued(i);
    }
    // piece k is complete once U(k+3) is: column dx (pieces 4dx..4dx+3) in iteration 4dx+6, then the row passes
    static constexpr int col_iter(int dx) { return 4 * dx + 6; }
    static constexpr int row_iter(int r) { return col_iter(3) + 1 + r; }
};
static_assert(Ups5Geo::row_iter(3) < Ups5Geo::NPOS, "next chunk transformed inside the MFMA loop");

// the shortcut-fused body of conv_wino_k<EPI, 0, 4, 1, 1, PERIMG>
template <int EPI, int PERIMG>
__device__ __forceinline__ void conv_ups5_body() {
    static_assert(!(EPI & (E_POOL | E_RES | E_RES_UPS | E_NORM2)), "conv1 epilogues only: bias, activation, saved-stat normalise");
    using G = Ups5Geo;
    constexpr int RAW_BYTES = G::RAW_BYTES, U_BYTES = G::U_BYTES, NT = G::NT, NB = G::NB, NPOS = G::NPOS, NUB = G::NUB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, t = lane & 15, q = lane >> 4;
    const int tr = t >> 3, tc = t & 7;
    const int tg = wave;                                // tile rows 2 tg, 2 tg + 1 of the workgroup's 8x8 tiles
    // ConvP through conv_args() (conv_mfma.h), region by region as in conv_f43_k: no field is held in SGPRs across the K loop
    const ConvPK p0 = conv_args();
    const int nchunks = p0->Cin >> 4;                   // even (Cin >= 64)

    // ---- work items: the walk of conv_wino_k
    struct Item { int tx, ty, b, nt; };
    Item cur, nxt, dlt;
    {
        const ConvPK p = p0;
        const int n_ntiles = p->Cout >> 5;
        const int GD = gridDim.x, w = blockIdx.x;
        int pix, dpix;
        if (p->xcd_slabs) {
            const int PT = (GD >> 3) / n_ntiles;
            pix = (w & 7) * PT + (w >> 3) / n_ntiles; dpix = 8 * PT;
            cur.nt = (w >> 3) % n_ntiles; dlt.nt = 0;
        } else {
            cur.nt = w % n_ntiles; pix = w / n_ntiles;
            dlt.nt = GD % n_ntiles; dpix = GD / n_ntiles;
        }
        cur.tx = pix % p->tiles_x; cur.ty = (pix / p->tiles_x) % p->tiles_y; cur.b = pix / (p->tiles_x * p->tiles_y);
        dlt.tx = dpix % p->tiles_x; dlt.ty = (dpix / p->tiles_x) % p->tiles_y; dlt.b = dpix / (p->tiles_x * p->tiles_y);
    }
    auto advance = [&](const ConvPK p, const Item& a) {
        const int n_ntiles = p->Cout >> 5;
        Item r = a;
        r.nt += dlt.nt;
        int carry = 0;
        if (r.nt >= n_ntiles) { r.nt -= n_ntiles; carry = 1; }
        r.tx += dlt.tx + carry;
        if (r.tx >= p->tiles_x) { r.tx -= p->tiles_x; r.ty += 1; }
        r.ty += dlt.ty;
        if (r.ty >= p->tiles_y) { r.ty -= p->tiles_y; r.b += 1; }
        r.b += dlt.b;
        return r;
    };
    auto in_of = [&](const ConvPK p, const Item& a) {      // 16x16 low-resolution pixels per item
        return p->in + (size_t)a.b * (size_t)(p->Hi + 2) * (p->Wi + 2) * p->Cin + (size_t)(((a.ty + p->ty0) * 16) * (p->Wi + 2) + (a.tx + p->tx0) * 16) * p->Cin;
    };
    auto w_of = [&](const ConvPK p, const Item& a) { return p->wpk + (size_t)a.nt * nchunks * (NUB * 32 * 16); };      // weights shared by the images of a launch
    int asrc[G::RAW_IT];
#pragma unroll
    for (int it = 0; it < G::RAW_IT; ++it) {     // LDS image of the 18x18 halo: even / odd column split (conv_wino_split_k)
        const int e = it * NT + tid;
        int P = e >> 2;
        const int qq = e & 3;
        if (P >= G::HALO * G::HALO) P = 0;
        const int hf = P >= G::HALF, rem = P - hf * G::HALF;
        const int hy = rem / 9, hx = 2 * (rem - hy * 9) + hf;
        asrc[it] = ((hy * (p0->Wi + 2) + hx) * p0->Cin + 4 * (qq ^ ((hx >> 1) & 3))) * 4;
    }
    const int tid16 = tid * 16;      // the U requests' lane offset; the epilogue takes its lane id from it
    const int raw_last_num = ((G::RAW_IT - 1) * NT + wave * 64 < G::PIECES) ? 0x7fffffff : 0;
    bool have = cur.b < p0->B, have_nxt = false;
    const float* in_t = in_of(p0, cur);
    const float* w_t = w_of(p0, cur);
    const float* in_n = in_t;
    const float* w_n = w_t;
    auto stage_u = [&](int chunk) {
        char* udst = smem + 2 * RAW_BYTES + (chunk & 1) * U_BYTES;
#pragma unroll
        for (int it = 0; it < G::U_IT; ++it) bufld16(w_t, udst + (it * NT + wave * 64) * 16, tid * 16, chunk * U_BYTES + it * NT * 16);
    };
    auto stage_raw = [&](int chunk) {
        char* rdst = smem + (chunk & 1) * RAW_BYTES;
#pragma unroll
        for (int it = 0; it < G::RAW_IT; ++it)
            if (it * NT + wave * 64 < G::PIECES) bufld16(in_t, rdst + (it * NT + wave * 64) * 16, asrc[it], chunk * 64);
    };
    // per-channel epilogue parameters: rows of 32 floats, 0 bias | 1-4 n1 (mean, rstd, lo, hi)
    char* const par = smem + 2 * RAW_BYTES + 2 * U_BYTES;
    auto stage_params = [&](int ntile, int img) {
        if (wave < 2) {
            const ConvPK p = conv_args();
            const int e = tid;
            const int row = e >> 3, col = (e & 7) * 4;
            int rrow = tid16;      // the row again, from a value that is live anyway and through an empty asm: (row - 1) is not precomputed and held in a VGPR across the item loop
            asm volatile("" : "+v"(rrow));
            rrow >>= 7;
            const float* src = p->bias;
            const int pb = PERIMG ? img * p->par_bstride : 0;
            int off = ntile * 32 + col;
            if (row >= 1 && row <= 4) { src = (EPI & E_NORM1) ? p->n1 : p->bias; off = (EPI & E_NORM1) ? ntile * 32 + col + pb + (rrow - 1) * p->Cout : off; }
            if (row > 4) { src = p->bias; off = ntile * 32; }
            glds16(src + off, par + wave * 1024);
        }
    };

    // LDS byte addresses: patch piece dx*4 + dy = halo pixel (4 tg + 2 tr + dy, 2 tc + dx), 16-byte piece q; U fragments
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    unsigned offD[4];      // column dx, row 0; row dy is dy * 9 pixels further (an immediate)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
        const int hy = 4 * tg + 2 * tr, hx = 2 * tc + dx;
        const int P = (hx & 1) * G::HALF + hy * 9 + (hx >> 1);
        offD[dx] = lds0 + P * 64 + ((q ^ ((hx >> 1) & 3)) << 4);
    }
    const unsigned offU = lds0 + 2 * RAW_BYTES + t * 64 + ((q ^ ((0 - (t >> 2)) & 3)) << 4);

    f32x4 acc[NPOS][NB];
    f32x4 va[16], vb[16];      // V of the current / next chunk: V[ry][kx] in element kx*4 + ry
    // (x0, x1, x2, x3) -> BT4 x = (x0 - x2, x1 + x2, x2 - x1, x3 - x1), in place
    auto pass = [](f32x4& x0, f32x4& x1, f32x4& x2, f32x4& x3) {
        const f32x4 a[4] = {x0, x1, x2, x3};
        x0 = ups5_comb<0, 0>(a); x1 = ups5_comb<0, 1>(a); x2 = ups5_comb<0, 2>(a); x3 = ups5_comb<0, 3>(a);
    };
    auto col_pass = [&](f32x4 (&d)[16], int dx) { pass(d[dx * 4 + 0], d[dx * 4 + 1], d[dx * 4 + 2], d[dx * 4 + 3]); };
    auto row_pass = [&](f32x4 (&d)[16], int r) { pass(d[0 * 4 + r], d[1 * 4 + r], d[2 * 4 + r], d[3 * 4 + r]); };

    // TAIL (compile time; an item's last two chunks are peeled out of the K loop): 0 a chunk with two more behind it, 1 the second-to-last,
    // 2 the last — whose requests carry the next item's first tiles, so the next item's addresses are live in the peeled pair only
    auto chunk_body = [&](int c, auto par_c, auto first_c, auto tail_c, f32x4 (&vcur)[16], f32x4 (&vnext)[16]) {
        constexpr int PAR = decltype(par_c)::value;
        constexpr bool FIRST = decltype(first_c)::value;
        constexpr int TAIL = decltype(tail_c)::value;
        // U(c+1) -> U buffer (c+1)&1, raw(c+2) -> raw buffer c&1; past the item's end the next item's U(0), raw(0), raw(1)
        constexpr bool own_u = TAIL < 2, own_r = TAIL < 1;
        const rsrc_t rs_u = make_rsrc(own_u ? w_t : w_n);
        const rsrc_t rs_r = make_rsrc(own_r ? in_t : in_n);
        const rsrc_t rs_rl = make_rsrc(own_r ? in_t : in_n, raw_last_num);
        const int usoff = own_u ? (c + 1) * U_BYTES : 0;
        const int rsoff = (own_r ? c + 2 : TAIL - 1) * 64;
        // LDS-DMA destinations = the wave's base + a literal, added where the request is issued; the base passes through an empty asm once
        // per chunk so that the 38 sums of a chunk pair are not hoisted out of the item loop into SGPRs held across it (conv_f43.h)
        int wb = wave * 1024;
        asm volatile("" : "+s"(wb));
        lds_char* const wdst = (lds_char*)smem + wb;
        lds_char* const udst = wdst + 2 * RAW_BYTES + (1 - PAR) * U_BYTES;
        lds_char* const rdst = wdst + PAR * RAW_BYTES;
        unsigned ub = offU;      // the odd chunks' U buffer: one v_add per chunk instead of a second address held in a VGPR across the item loop
        if constexpr (PAR != 0) { asm volatile("" : "+v"(ub)); ub += U_BYTES; }
        constexpr int RB = (1 - PAR) * RAW_BYTES;    // raw buffer (c+1)&1
        f32x4 u[4][NB];      // U fragments in flight, slot = position & 3
        f32x4 (&d)[16] = vnext;
        u[0][0] = lds_rd128<0>(ub);
        u[0][1] = lds_rd128<1024>(ub);
        u[1][0] = lds_rd128<2048>(ub);
        u[1][1] = lds_rd128<2048 + 1024>(ub);
        static_for([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr (i + 2 < NUB) {
                u[(i + 2) & 3][0] = lds_rd128<(i + 2) * 2048>(ub);
                u[(i + 2) & 3][1] = lds_rd128<(i + 2) * 2048 + 1024>(ub);
            }
            if constexpr (i < 16) d[i] = lds_rd128<RB + (i & 3) * 576>(offD[i >> 2]);
            constexpr int US = (i < NUB ? i : NUB - 1) & 3;      // positions 26..28 reuse the shortcut block of 25
            if constexpr (i < NUB) {
                constexpr int cdx = (i - 6) / 4;
                if constexpr (i >= 6 && (i - 6) % 4 == 0 && cdx < 4) {      // U(i) and column cdx of the patch
                    static_assert(G::col_iter(cdx) == i, "column release schedule");
                    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(d[cdx * 4 + 0]), "+v"(d[cdx * 4 + 1]), "+v"(d[cdx * 4 + 2]), "+v"(d[cdx * 4 + 3]),
                                 "+v"(u[US][0]), "+v"(u[US][1]) : "i"(G::younger(i)));
                } else {
                    lds_release2<G::younger(i)>(u[US][0], u[US][1]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i < G::U_IT) bufld16_rs(rs_u, udst + i * NT * 16, tid16, usoff + i * NT * 16);
            if constexpr (i < G::RAW_IT) bufld16_rs(i == G::RAW_IT - 1 ? rs_rl : rs_r, rdst + i * NT * 16, asrc[i], rsoff);
            const f32x4 vv = vcur[G::vidx(i)];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[i][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[US][nb][s], vv[s], (FIRST && s == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[i][nb], 0, 0, 0);
            static_for([&](auto xc) {
                constexpr int k = decltype(xc)::value;
                if constexpr (G::col_iter(k) == i) col_pass(d, k);
                if constexpr (G::row_iter(k) == i) row_pass(d, k);
            }, std::make_integer_sequence<int, 4>{});
        }, std::make_integer_sequence<int, NPOS>{});
    };

    int par_ntile = -1, par_img = -1;
    if (have) {
        stage_raw(0);
        stage_u(0);
        stage_raw(1);
        stage_params(cur.nt, cur.b);
        par_ntile = cur.nt; par_img = cur.b;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) va[k] = *(const f32x4*)(smem + (offD[k >> 2] - lds0) + (k & 3) * 576);
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) col_pass(va, dx);
#pragma unroll
        for (int r = 0; r < 4; ++r) row_pass(va, r);
        __syncthreads();      // raw(0) read by every wave before the first chunk requests raw(2) into its buffer
    }
    while (have) {
        if (par_ntile != cur.nt || (PERIMG && par_img != cur.b)) {
            __syncthreads();
            stage_params(cur.nt, cur.b);
            par_ntile = cur.nt; par_img = cur.b;
        }
        using C0 = std::integral_constant<int, 0>; using C1 = std::integral_constant<int, 1>; using C2 = std::integral_constant<int, 2>;
        chunk_body(0, C0{}, std::true_type{}, C0{}, va, vb);
        __syncthreads();
        chunk_body(1, C1{}, std::false_type{}, C0{}, vb, va);
        __syncthreads();
        for (int c = 2; c + 2 < nchunks; c += 2) {
            chunk_body(c, C0{}, std::false_type{}, C0{}, va, vb);
            __syncthreads();
            chunk_body(c + 1, C1{}, std::false_type{}, C0{}, vb, va);
            __syncthreads();
        }
        // the next item: only the peeled last two chunks (which request its first tiles) and the loop's next turn need it
        const int e_b = cur.b, e_ntile = cur.nt;
        int e_y0, e_x0;
        {
            const ConvPK pn = conv_args();
            e_y0 = (cur.ty + pn->ty0) * 32; e_x0 = (cur.tx + pn->tx0) * 32;
            nxt = advance(pn, cur);
            have_nxt = nxt.b < pn->B;
            in_n = have_nxt ? in_of(pn, nxt) : in_t;
            w_n = have_nxt ? w_of(pn, nxt) : w_t;
        }
        chunk_body(nchunks - 2, C0{}, std::false_type{}, C1{}, va, vb);
        __syncthreads();
        chunk_body(nchunks - 1, C1{}, std::false_type{}, C2{}, vb, va);
        __syncthreads();
        cur = nxt; have = have_nxt; in_t = in_n; w_t = w_n;

        // ---- output transform + epilogue.  The lane's tile: outputs (yb..yb+3, xb..xb+3), low-resolution pixels (ly0.., lx0..)
        const ConvPK p = conv_args();      // the epilogue's fields: loaded here
        // ... and its lane coordinates derived here, from a lane id the compiler cannot trace to the kernel's start: hoisted out of the
        // item loop, the epilogue's per-lane offsets and 64-bit addresses sat in VGPRs across the K loop (parked in AGPRs or scratch)
        int ln = tid16;
        asm volatile("" : "+v"(ln));
        ln = (ln >> 4) & 63;
        const int t = ln & 15, q = ln >> 4, tr = t >> 3, tc = t & 7;
        float* out_b = p->out + (size_t)e_b * (size_t)(p->H + 2) * (p->W + 2 + (p->out_p8 ? 6 : 0)) * p->Cout;
        const int yb = e_y0 + 8 * tg + 4 * tr, xb = e_x0 + 4 * tc;
        // the epilogue starts behind the K loop's last MFMA run: scheduled into it, its first reads met the next item's patch (64 VGPRs, live
        // across the epilogue) at the register limit, and an accumulator quad of the frame-mode instantiation went through scratch
        __builtin_amdgcn_sched_barrier(0);
        {      // shortcut: sc[a][b] = P_mm + sb P_md + sa P_dm + sa sb P_dd, s0 = -1, s1 = +1 (no bias: conv_shortcut has none)
            const int ly0 = yb >> 1, lx0 = xb >> 1;
            float* sc_b = p->sc_out + (size_t)e_b * (size_t)(p->Hi + 2) * (p->Wi + 2) * p->Cout;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const f32x4 s0 = f4sub(acc[25][nb], acc[27][nb]), s1 = e4add(acc[25][nb], acc[27][nb]);      // a = 0 / 1
                const f32x4 t0 = f4sub(acc[26][nb], acc[28][nb]), t1 = e4add(acc[26][nb], acc[28][nb]);
                const f32x4 sc[2][2] = {{f4sub(s0, t0), e4add(s0, t0)}, {f4sub(s1, t1), e4add(s1, t1)}};
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int ly = ly0 + a, lx = lx0 + b;
                        if (ly < p->Hi && lx < p->Wi)
                            *(f32x4*)(sc_b + ((size_t)(ly + 1) * (p->Wi + 2) + lx + 1) * p->Cout + e_ntile * 32 + nb * 16 + 4 * q) = sc[a][b];
                    }
            }
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int co = e_ntile * 32 + nb * 16 + 4 * q;
            // Y = A^T M A: first along x (column index j), then along y
            f32x4 T[5][4];
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const f32x4 m[5] = {acc[r * 5 + 0][nb], acc[r * 5 + 1][nb], acc[r * 5 + 2][nb], acc[r * 5 + 3][nb], acc[r * 5 + 4][nb]};
                T[r][0] = ups5_comb<1, 0>(m); T[r][1] = ups5_comb<1, 1>(m); T[r][2] = ups5_comb<1, 2>(m); T[r][3] = ups5_comb<1, 3>(m);
            }
            f32x4 Y[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 tj[5] = {T[0][j], T[1][j], T[2][j], T[3][j], T[4][j]};
                Y[0][j] = ups5_comb<1, 0>(tj); Y[1][j] = ups5_comb<1, 1>(tj); Y[2][j] = ups5_comb<1, 2>(tj); Y[3][j] = ups5_comb<1, 3>(tj);
            }
            const char* pl = par + (nb * 16 + 4 * q) * 4;
            const f32x4 bias = *(const f32x4*)(pl);
            f32x4 m1, r1, lo1, hi1;
            if (EPI & E_NORM1) {
                m1 = *(const f32x4*)(pl + 128); r1 = *(const f32x4*)(pl + 256);
                lo1 = *(const f32x4*)(pl + 384); hi1 = *(const f32x4*)(pl + 512);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int y = yb + i, x = xb + j;
                    f32x4 o = e4add(Y[i][j], bias);
                    if (EPI & E_RELU) o = f4relu(o);
                    if (EPI & E_LRELU) o = f4lrelu(o);
                    if (EPI & E_NORM1) o = f4norm_clamp(o, m1, r1, lo1, hi1);
                    if (y < p->H && x < p->W) {
                        if (p->out_p8) *(f32x4*)(out_b + (size_t)(co >> 3) * ((size_t)(p->H + 2) * (p->W + 8) * 8) + ((size_t)(y + 1) * (p->W + 8) + x + 4) * 8 + (co & 7)) = o;
                        else *(f32x4*)(out_b + ((size_t)(y + 1) * (p->W + 2) + x + 1) * p->Cout + co) = o;
                    }
                }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the last LDS-DMA transfers land before the workgroup frees its LDS
}

// U = G g G^T of the upsample-fused form above, in double and rounded once, packed as [Cout/32][Cin/16][26 blocks][32 couts]
// [16 floats] with the pieces XOR-swizzled by -(cout>>2)&3 (pack_wino_k's image); block 25 = the 1x1 shortcut / 4.
__global__ void pack_ups5_k(const float* __restrict__ w, const float* __restrict__ wsc, float* __restrict__ dst, int Cout, int Cin) {
    constexpr int CH = 16, NUB = Ups5Geo::NUB;
    const size_t total = (size_t)Cout * Cin * NUB;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t r = i;
        const int cl = (int)(r % CH); r /= CH;
        const int j = r & 31; r >>= 5;
        const int pos = (int)(r % NUB); r /= NUB;
        const int nchunks = Cin / CH;
        const int chunk = r % nchunks; r /= nchunks;
        const int n_tile = (int)r;
        const int e = cl & 3, qs = cl >> 2;
        const int qq = qs ^ ((0 - (j >> 2)) & 3);
        const int co = n_tile * 32 + j, ci = chunk * CH + qq * 4 + e;
        if (pos == 25) { dst[i] = wsc[(size_t)co * Cin + ci] * 0.25f; continue; }
        const float* g = w + ((size_t)co * Cin + ci) * 9;
        auto G5 = [](int row, double g0, double g1, double g2) {      // (G g)[row] = G2[row] . g / 2, exact in double
            return 0.5 * (Ups5Tab::G2[row][0] * g0 + Ups5Tab::G2[row][1] * g1 + Ups5Tab::G2[row][2] * g2);
        };
        const int pr = pos / 5, pc = pos % 5;      // pr acts on ky, pc on kx
        double rowv[3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) rowv[kx] = G5(pr, g[0 * 3 + kx], g[1 * 3 + kx], g[2 * 3 + kx]);
        dst[i] = (float)G5(pc, rowv[0], rowv[1], rowv[2]);
    }
}

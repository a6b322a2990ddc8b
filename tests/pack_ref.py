"""Float64 references for every weight buffer the handle holds (rrv_debug_copy_weights) and the checks that bound each pack / fold
kernel's own rounding.  Plain module (no pytest): imported by tests/test_gpu_packs.py and tests/test_pack_ref.py.

Written from the documented layouts (the comment above each pack kernel), as whole-array reshapes and one gather per
swizzle, not from the kernels' index arithmetic:

  pk          pack_conv_k   [Cout/BN][Cin/16][taps][BN couts][4 pieces][4 floats]      piece q of cout j is stored at q ^ ((j >> 2) & 3)
  pk_wino     pack_wino_k   [Cout/32][Cin/16][16 positions][32 couts][4 pieces][4]     piece q of cout j is stored at q ^ (-(j >> 2) & 3);
  pk_ups      pack_wino_k   [Cout/32][Cin/16][ 9 positions][32 couts][4 pieces][4]     the same image
  pk_ups_sc   pack_ups5_k   [Cout/32][Cin/16][25 positions + the shortcut / 4][32][4][4]   the same image
  pk_f43      pack_f43_k    [Cout/32][Cin/8][36 positions][16 rows][4 slots][2 blocks][2 channels]: cout 2 row + block, channel
                            2 pair + c, pair p of row r stored in slot p ^ (-(r >> 2) & 3)
  first       pack_first_k  [tap][rgb][64]        first_grey  pack_first_grey_k  W1 [9][64] | W0 [9][64] | bias + sum W0 [64]
  last        pack_last_k   [blk 2][chunk 4][lane 64][step 4] = W[n = 16 blk + (lane & 15)][channel 16 chunk + 4 (lane >> 4) + step], n = 3 tap + rgb,
                            rows 27..31 zero
The mask (0, 3, 2, 1)[(j >> 2) & 3] of the transform-domain packs is what the consumers' LDS readers undo (offU in conv_wino.h,
conv_wino_split.h, conv_ups5.h and conv_f43.h: row t reads piece q at q ^ (-(t >> 2) & 3)); the direct-form pack keeps the plain
(j >> 2) & 3 (offB in conv_mfma.h).

A position p = pr * n + pc of a transformed pack holds U[pr][pc] = sum_ky,kx G[pr][ky] g[ky][kx] G[pc][kx]; its magnitude m is the
same sum on absolute values.  The transforms' G:
  F(2x2,3x3)   [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]              nine-product upsample   [[1,1,1],[1,0,0],[0,0,1]]
  five-product [[1,0,0],[.5,.5,.5],[-.5,-.5,.5],[-.5,.5,.5],[0,0,1]]  (conv_ups5.h)
  F(4x4,3x3)   row j = (1, p_j, p_j^2) / prod_{l != j} (p_j - p_l) for the points 0, 3/4, -3/4, 3/2, -3/2, then (0, 0, 1)  (conv_f43.h)

Checks (each returns (passes, worst figure)):
  exact(got, ref)                 bit for bit
  rounded_once(got, u)            |got - u| <= (1/2 + 2^-20) ulp32(u): u evaluated in extended precision, got its one rounding
  within(got, v, m, n)            |got - v| <= n 2^-24 m [+ 2^-24 |v|]: n float32 roundings on an element's path
"""
import numpy as np

U24 = 2.0 ** -24
ONCE = 0.5 + 2.0 ** -20

G23 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
GUPS9 = np.array([[1, 1, 1], [1, 0, 0], [0, 0, 1]], np.float64)
GUPS5 = np.array([[1, 0, 0], [.5, .5, .5], [-.5, -.5, .5], [-.5, .5, .5], [0, 0, 1]], np.float64)
F43_POINTS = (0.0, 0.75, -0.75, 1.5, -1.5)


def g43(dtype=np.longdouble):
    rows = []
    for j, p in enumerate(F43_POINTS):
        n = dtype(1)
        for l, q in enumerate(F43_POINTS):
            if l != j:
                n = n * dtype(p - q)
        rows.append([dtype(1) / n, dtype(p) / n, dtype(p * p) / n])
    rows.append([dtype(0), dtype(0), dtype(1)])
    return np.array(rows, dtype)


# ---- the convolutions of the checkpoint and the buffers each one gets (rrv_finalize_weights) ------------------------------------------------
VGG = ((2, 64, 64), (5, 128, 64), (7, 128, 128), (10, 256, 128), (12, 256, 256), (14, 256, 256), (16, 256, 256), (19, 512, 256))   # (index, cout, cin) of conv1_2 .. conv4_1
STYLE_SLICE = {2: 2, 5: 2, 7: 3, 10: 3, 12: 4, 14: 4, 16: 4, 19: 4}
BLOCKS = (("slice4", 256), ("slice3", 128), ("slice2", 64))
N_SETS = 32


def expected_buffers():
    """[(key, form)] of every buffer rrv_debug_weight_count enumerates, as a set would hold them (the library's order is its own)."""
    out = []

    def conv(key, cout, cin, taps, pk=True, extra=()):
        forms = ["raw", "bias"] + (["pk"] if pk else []) + (["pk_wino"] if pk and taps == 9 and cin >= 64 and cout >= 64 else []) + list(extra)
        out.extend((key, f) for f in forms)

    for idx, cout, cin in VGG:
        conv("Encoder.slice.%d" % idx, cout, cin, 9, extra=("pk_f43",) if idx != 19 else ())
        conv("EncoderStyle.slice%d.%d" % (STYLE_SLICE[idx], idx), cout, cin, 9)
    for blk, cout in BLOCKS:
        conv("Decoder.%s.conv1" % blk, cout, 2 * cout, 9, pk=False, extra=("pk_ups", "pk_ups_sc"))
        conv("Decoder.%s.conv2" % blk, cout, cout, 9, extra=("pk_f43",))
        conv("Decoder.%s.conv_shortcut" % blk, cout, 2 * cout, 1)
    for f in (1, 2, 3):
        conv("Decoder.Filter%d.down_sample.0" % f, 32, 512, 9, pk=False, extra=("pk_wino",))
        conv("Decoder.Filter%d.upsample.0" % f, 512, 32, 9, pk=False, extra=("pk_wino",))
        for g in (1, 2):
            conv("Decoder.Filter%d.F%d.down_sample.0" % (f, g), 32, 512, 9)
        out.extend(("Decoder.Filter%d.fold_down" % f, form) for form in ("raw", "bias", "pk_wino"))
        out.extend(("Decoder.Filter%d.fold_up" % f, form) for form in ("raw", "pk_wino"))
    out.extend([("Encoder.slice.0", "first"), ("Encoder.slice.0", "first_grey"), ("Encoder.slice.0", "bias"),
                ("EncoderStyle.slice1.0", "first"), ("EncoderStyle.slice1.0", "bias"), ("Decoder.slice1", "last"), ("Decoder.slice1", "bias")])
    return sorted(out)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------------
def _pieces(a, rows, negate):
    """a [.., rows, 4 pieces, n]: piece q of row j moves to q ^ mask(j), mask = (j >> 2) & 3, negated (mod 4) for the transform-domain packs."""
    j = np.arange(rows)
    mask = (-(j >> 2) & 3) if negate else ((j >> 2) & 3)
    return a[..., j[:, None], np.arange(4)[None, :] ^ mask[:, None], :]


def slab16(u, bn=32, negate=True):
    """u [Cout][Cin][positions] -> [Cout/bn][Cin/16][positions][bn][16] with the 16-byte pieces swizzled, flat."""
    co, ci, npos = u.shape
    a = u.reshape(co // bn, bn, ci // 16, 4, 4, npos).transpose(0, 2, 5, 1, 3, 4)
    return np.ascontiguousarray(_pieces(a, bn, negate)).reshape(-1)


def slab_f43(u):
    """u [Cout][Cin][36] -> [Cout/32][Cin/8][36][16 rows][4 slots][2 blocks][2 channels], flat."""
    co, ci, npos = u.shape
    a = u.reshape(co // 32, 16, 2, ci // 8, 4, 2, npos).transpose(0, 3, 6, 1, 4, 2, 5)       # [nt][chunk][pos][row][pair][block][c]
    a = a.reshape(co // 32, ci // 8, npos, 16, 4, 4)
    return np.ascontiguousarray(_pieces(a, 16, True)).reshape(-1)


def transform(raw, G, dtype=np.float64):
    """(U, m) [Cout][Cin][positions]: U = G g G^T of every 3 x 3 filter and the same product on absolute values."""
    g = np.asarray(raw).reshape(raw.shape[0], raw.shape[1], 3, 3).astype(dtype)
    G = np.asarray(G, dtype)
    n = G.shape[0]

    def tr(G, g):      # two plain matrix products (einsum does not take long doubles everywhere)
        t = (G[None, None, :, :, None] * g[:, :, None, :, :]).sum(axis=3)            # [o][i][pr][kx]
        return (t[:, :, :, None, :] * G[None, None, None, :, :]).sum(axis=4)         # [o][i][pr][pc]
    return tr(G, g).reshape(g.shape[0], g.shape[1], n * n), tr(np.abs(G), np.abs(g)).reshape(g.shape[0], g.shape[1], n * n)


def pk(raw, bn):
    w = np.asarray(raw)
    return slab16(w.reshape(w.shape[0], w.shape[1], -1), bn, negate=False)


def pk_wino(raw, ups=False):
    u, m = transform(raw, GUPS9 if ups else G23)
    return slab16(u), slab16(m)


def pk_ups_sc(raw, shortcut, dtype=np.longdouble):
    """The 25 five-product positions in extended precision, then block 25 = shortcut / 4 (exact in float32)."""
    u, _ = transform(raw, GUPS5, dtype)
    sc = np.asarray(shortcut).reshape(u.shape[0], u.shape[1], 1).astype(dtype) / 4
    return slab16(np.concatenate([u, sc], axis=2))


def pk_f43(raw, dtype=np.longdouble):
    return slab_f43(transform(raw, g43(dtype), dtype)[0])


def first(raw):
    return np.ascontiguousarray(np.asarray(raw).reshape(64, 3, 9).transpose(2, 1, 0)).reshape(-1)


GREY_N = (3, 4, 29)      # float32 roundings on the path of a W1, W0 and folded-bias element (tests/test_gpu_packs.py derives them)


def first_grey(raw, bias):
    """(v, m, n) of the grey fold, 1216 values: x_c = (g - mean_c) / sd_c, so W1 = sum_c w_c / sd_c, W0 = -sum_c w_c (mean_c / sd_c), and
    bias + sum_taps W0.  The float32 constants widened (as layer_ref.grey_input), every operation on them in float64."""
    mean, sd = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    r = mean.astype(np.float64) / sd.astype(np.float64)
    w = np.asarray(raw, np.float64).reshape(64, 3, 9)
    w1 = (w / sd.astype(np.float64)[None, :, None]).sum(axis=1).T                      # [tap][co]
    m1 = (np.abs(w) / sd.astype(np.float64)[None, :, None]).sum(axis=1).T
    w0 = -(w * r[None, :, None]).sum(axis=1).T
    m0 = (np.abs(w) * r[None, :, None]).sum(axis=1).T
    b = np.asarray(bias, np.float64) + w0.sum(axis=0)
    mb = np.abs(np.asarray(bias, np.float64)) + m0.sum(axis=0)
    v = np.concatenate([w1.reshape(-1), w0.reshape(-1), b])
    m = np.concatenate([m1.reshape(-1), m0.reshape(-1), mb])
    n = np.concatenate([np.full(576, GREY_N[0]), np.full(576, GREY_N[1]), np.full(64, GREY_N[2])]).astype(np.float64)
    return v, m, n


def last(raw):
    w = np.asarray(raw).reshape(3, 64, 9)
    rows = np.zeros((32, 64), w.dtype)
    rows[:27] = w.transpose(2, 0, 1).reshape(27, 64)                                   # row n = 3 tap + rgb
    a = rows.reshape(2, 16, 4, 4, 4)                                                   # [blk][m][chunk][kq][step]
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1, 4)).reshape(-1)                # [blk][chunk][lane = 16 kq + m][step]


# ---- folds (quirk Q2: the predicted filter is used as weight[out = i][in = j] = F[i][j]) -------------------------------------------------------------
FOLD_N = 32      # a 32-term float32 sum


def fold_down(F, wd, bd):
    """((W', m), (b', mb)): W'[o][ci][t] = sum_m F[o][m] Wd[m][ci][t], b'[o] = sum_m F[o][m] bd[m], flat OIHW and [32]."""
    F, wd, bd = np.asarray(F, np.float64).reshape(32, 32), np.asarray(wd, np.float64).reshape(32, -1), np.asarray(bd, np.float64)
    return (((F @ wd).reshape(-1), (np.abs(F) @ np.abs(wd)).reshape(-1)), (F @ bd, np.abs(F) @ np.abs(bd)))


def fold_up(F, wu):
    """(W', m): W'[o][j][t] = sum_m Wu[o][m][t] F[m][j], flat OIHW."""
    F, wu = np.asarray(F, np.float64).reshape(32, 32), np.asarray(wu, np.float64).reshape(-1, 32, 9)
    return (np.einsum("omt,mj->ojt", wu, F).reshape(-1), np.einsum("omt,mj->ojt", np.abs(wu), np.abs(F)).reshape(-1))


# ---- checks ---------------------------------------------------------------------------------------------------------------------------------------
def exact(got, ref):
    got, ref = np.asarray(got, np.float32).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    same = got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    return bool(same), 0.0 if same else float("inf")


def ulp32(x):
    """The spacing of float32 at the (extended-precision) value x: 2^(e - 23) for 2^e <= |x| < 2^(e + 1), 2^-149 below the normal range."""
    _, ex = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.maximum(ex - 24, -149))


def rounded_once(got, u):
    """|got - u| <= (1/2 + 2^-20) ulp32(u), the difference taken in u's precision: (passes, worst |got - u| / ulp32(u))."""
    u = np.asarray(u).reshape(-1)
    got = np.asarray(got, np.float32).reshape(-1)
    if got.shape != u.shape:
        return False, float("inf")
    err = np.abs(got.astype(u.dtype) - u).astype(np.float64) / ulp32(u)
    worst = float(err.max()) if err.size else 0.0
    return bool(worst <= ONCE), worst


def within(got, v, m, n, rel=False):
    """|got - v| <= n 2^-24 m (+ 2^-24 |v| with rel): (passes, worst |got - v| / (2^-24 m)); n a number or per element."""
    got = np.asarray(got, np.float64).reshape(-1)
    if got.shape != np.shape(v):
        return False, float("inf")
    err = np.abs(got - v)
    bound = n * U24 * m + (U24 * np.abs(v) if rel else 0.0)
    ratio = err / np.maximum(U24 * m, 1e-300)
    return bool(np.all(err <= bound)), float(ratio.max()) if err.size else 0.0


# ---- one verdict per buffer: what tests/test_gpu_packs.py asserts and tests/test_pack_ref.py proves able to fail ---------------------------------------
FAMILY = {"raw": "copy", "bias": "copy", "pk": "copy", "first": "copy", "last": "copy", "pk_f43": "once", "pk_ups_sc": "once", "pk_wino": "pack32",
          "pk_ups": "pack32", "first_grey": "grey"}
PACK32_N = 4     # F(2x2) and the nine-product form: two float32 roundings per stage (see tests/test_gpu_packs.py)


def check_buffer(key, form, got, w, k32=PACK32_N, kgrey=None):
    """A checkpoint weight's buffer against the checkpoint dict w: (passes, figure, family).  figure: 0 / inf for the bit-for-bit
    forms, ulps for the rounded-once forms, |got - ref| / (2^-24 m) for the float32 forms."""
    raw = w.get(key + ".weight")
    if form == "raw":
        return exact(got, raw) + ("copy",)
    if form == "bias":
        ref = w[key + ".bias"] if key + ".bias" in w else np.zeros(raw.shape[0], np.float32)
        if key == "Decoder.slice1":
            ref = np.concatenate([ref, np.zeros(1, np.float32)])      # four floats, the fourth zero
        return exact(got, ref) + ("copy",)
    if form == "pk":
        co = raw.shape[0]
        return exact(got, pk(raw, 128 if co >= 128 else 64 if co >= 64 else 32)) + ("copy",)
    if form == "first":
        return exact(got, first(raw)) + ("copy",)
    if form == "last":
        return exact(got, last(raw)) + ("copy",)
    if form == "pk_f43":
        return rounded_once(got, pk_f43(raw)) + ("once",)
    if form == "pk_ups_sc":
        return rounded_once(got, pk_ups_sc(raw, w[key.replace("conv1", "conv_shortcut") + ".weight"])) + ("once",)
    if form in ("pk_wino", "pk_ups"):
        v, m = pk_wino(raw, ups=form == "pk_ups")
        return within(got, v, m, k32) + ("pack32",)
    if form == "first_grey":
        v, m, n = first_grey(raw, w[key + ".bias"])
        return within(got, v, m, n if kgrey is None else np.minimum(n, kgrey)) + ("grey",)
    raise AssertionError("unknown form " + form)


def check_fold(kind, form, got, F, w, f, got_raw=None, kfold=FOLD_N, k32=PACK32_N):
    """A folded KernelFilter buffer of one state set: kind "down" / "up", KernelFilter f (0..2), F the set's own filter [32][32]
    (F1 for down, F2 for up).  raw and bias against the float64 product, 32 2^-24 sum |F||W| + 2^-24 |ref|; bias floats 32..255
    exactly 0; pk_wino against the F(2x2) pack of the set's own folded raw (got_raw).  (passes, figure, family)."""
    p = "Decoder.Filter%d.%s.0." % (f + 1, "down_sample" if kind == "down" else "upsample")
    if form == "pk_wino":
        shape = (32, 512, 3, 3) if kind == "down" else (512, 32, 3, 3)
        v, m = pk_wino(np.asarray(got_raw, np.float32).reshape(shape))
        return within(got, v, m, k32) + ("pack32",)
    if kind == "up":
        return within(got, *fold_up(F, w[p + "weight"]), kfold, rel=True) + ("fold",)
    (v, m), (vb, mb) = fold_down(F, w[p + "weight"], w[p + "bias"])
    if form == "raw":
        return within(got, v, m, kfold, rel=True) + ("fold",)
    got = np.asarray(got, np.float32).reshape(-1)
    ok, fig = within(got[:32], vb, mb, kfold, rel=True)
    return ok and got.size == 256 and not np.any(got[32:]), fig, "fold"

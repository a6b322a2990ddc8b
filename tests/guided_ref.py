"""Reference of the guided delivery stage (include/rerevst_hip.h "Guided delivery"), written from the header and not from the library;
it does not import the package.

Per frame, all float32 HWC BGR PIXEL: the stylized working frame P [H][W][3], the source at the working size X_lo [H][W][3] and at the
delivered size X_hi [DH][DW][3]; radius r in working pixels, eps in the units of a 0..1 image, e = eps * 65025.
    g        = (0.114f B + 0.587f G) + 0.299f R                                  g_lo of X_lo, g_hi of X_hi
    M_r(f)   the mean of f over [y - r, y + r] x [x - r, x + r] clipped to the frame, divided by the pixels actually inside
    a_c      = (M_r(g_lo P_c) - M_r(g_lo) M_r(P_c)) / (M_r(g_lo^2) - M_r(g_lo)^2 + e)
    b_c      = M_r(P_c) - a_c M_r(g_lo)
    A_c, B_c = M_r(a_c), M_r(b_c)
    Q_c      = up(A_c) g_hi + up(B_c)       up: the rrv_resample_taps tables of (H -> DH), (W -> DW), along rows first, then along columns
stage(.., dtype=np.float64) is the reference: every window sum adds its terms one by one in float64 (no running sums, nothing cancels), the
tables' weights are the float32 values the library's tables hold.  stage(.., dtype=np.float32) is the same text with every operation in
float32, sums in plain ascending order: the "naive" evaluation whose error against float64 is the yardstick of the kernels' (NAIVE_ERR).

CASES are the shapes the GPU test runs, inputs() their three kinds of frames, EPS the two regularisers.
Plain module, no pytest."""
import numpy as np

import resample_ref as R

F = np.float32
LUMA = (F(0.114), F(0.587), F(0.299))      # B, G, R
EPS = (1e-4, 1e-2)
KINDS = ("ramp", "noise", "step")
# name: ((H, W), (DH, DW), r): a window larger than the frame and a non-square ratio; several tiles of both kernels with ragged last ones and a
# non-integer ratio; equal size; the limits of both ranges (r = 16, 8 x)
CASES = {
    "a_r1": ((8, 8), (16, 24), 1),
    "a_r4": ((8, 8), (16, 24), 4),
    "a_r9": ((8, 8), (16, 24), 9),
    "b": ((40, 72), (97, 131), 5),
    "c": ((24, 24), (24, 24), 4),
    "d": ((8, 16), (64, 128), 16),
    # the tiles of gf_apply_k (tile() below; tests/test_gpu_guided.py asserts them through rrv_guided_tile)
    "e": ((24, 80), (24, 80), 16),          # tw = 32 at 120,000 B of LDS, equal size
    "f": ((24, 80), (24, 80), 11),          # tw = 64 at 147,840 B, the largest request that fits
    "g": ((24, 80), (30, 90), 16),          # tw = 32 with two-tap rows and columns, seams at 32 and 64, a last tile of 26 columns
    "h_row": ((1, 40), (8, 75), 3),         # a one-pixel axis: the window is the frame on that axis, the anchor clamps
    "h_col": ((40, 1), (75, 8), 3),
    "j": ((17, 33), (33, 65), 2),           # last tiles of one row and one column in both kernels
    "k": ((9, 10), (72, 80), 1),            # 8 x on both axes with the smallest radius
}

# The tile of gf_apply_k, restated from csrc/guided.h: 16 delivered rows by tw columns, tw the widest of 64, 32, 16, 8 whose dynamic LDS fits.
R_MAX = 16
AT_H, CT_H, CT_W = 16, 16, 32
LDS_MAX = 152 * 1024


def span(S, D, T):
    """working samples that T consecutive delivered samples' taps span at most, S -> D with D >= S"""
    return min((T - 1) * S // D + 3, S)


def apply_lds_bytes(r, sy, sx):
    """staged planes [6][sy + 2r][sx + 2r] and their row sums [6][sy + 2r][sx], float32"""
    return (6 * (sy + 2 * r) * (sx + 2 * r) + 6 * (sy + 2 * r) * sx) * 4


def coeff_lds_bytes(r):
    """staged g, P_c [4][16 + 2r][32 + 2r] and the row sums of the eight moments [8][16 + 2r][32], float32"""
    return (4 * (CT_H + 2 * r) * (CT_W + 2 * r) + 8 * (CT_H + 2 * r) * CT_W) * 4


def tile(H, W, DH, DW, r):
    """(tw, sy, sx, apply LDS bytes) of working H x W, delivered DH x DW and radius r; None where no tile fits"""
    sy = span(H, DH, AT_H)
    for tw in (64, 32, 16, 8):
        sx = span(W, DW, tw)
        if apply_lds_bytes(r, sy, sx) <= LDS_MAX:
            return tw, sy, sx, apply_lds_bytes(r, sy, sx)
    return None


def luma(x, dtype=np.float64):
    x = np.asarray(x, F).astype(dtype)
    k = [dtype(c) for c in LUMA]
    return (k[0] * x[..., 0] + k[1] * x[..., 1]) + k[2] * x[..., 2]


def window_count(n, r):
    """[n] samples of [i - r, i + r] inside 0..n-1"""
    i = np.arange(n)
    return np.minimum(i + r, n - 1) - np.maximum(i - r, 0) + 1


def _axis_sum(f, r, axis):
    """sum over [i - r, i + r] clipped, along `axis`, the terms added in ascending order in f's dtype"""
    n = f.shape[axis]
    pad = [(0, 0)] * f.ndim
    pad[axis] = (r, r)
    z = np.pad(f, pad)
    out = np.zeros_like(f)
    for d in range(2 * r + 1):
        out = out + np.take(z, np.arange(d, d + n), axis=axis)
    return out


def box_mean(f, r):
    """M_r of [B][H][W] (or [B][H][W][C]) planes, in f's dtype: row sums, column sums of those, one division by the window's pixel count"""
    H, W = f.shape[1:3]
    cnt = (window_count(H, r)[:, None] * window_count(W, r)[None, :]).astype(f.dtype)
    s = _axis_sum(_axis_sum(f, r, 2), r, 1)
    return s / (cnt[..., None] if f.ndim == 4 else cnt)


def upsample(f, DH, DW):
    """[B][H][W][C] -> [B][DH][DW][C] in f's dtype with the tables' float32 weights: along rows first, then along columns, taps ascending"""
    dt = f.dtype.type
    for axis, D in ((2, DW), (1, DH)):
        first, count, w = R.taps(f.shape[axis], D)
        w = w.astype(F).astype(f.dtype)
        shape = [1] * f.ndim
        shape[axis] = D
        out = np.zeros(f.shape[:axis] + (D,) + f.shape[axis + 1:], f.dtype)
        for j in range(int(count.max())):
            idx = np.minimum(first + j, f.shape[axis] - 1)
            wj = np.where(j < count, w[:, j], dt(0)).reshape(shape)
            out = out + wj * np.take(f, idx, axis=axis)
        f = out
    return f


def coefficients(P, x_lo, r, eps, dtype=np.float64):
    """(a, b) [B][H][W][3] each"""
    P = np.asarray(P, F).astype(dtype)
    g = luma(x_lo, dtype)
    e = dtype(eps) * dtype(65025.0)
    mg, mgg = box_mean(g, r), box_mean(g * g, r)
    mP, mgP = box_mean(P, r), box_mean(g[..., None] * P, r)
    a = (mgP - mg[..., None] * mP) / (mgg - mg * mg + e)[..., None]
    return a, mP - a * mg[..., None]


def stage(P, x_lo, x_hi, r, eps, dtype=np.float64):
    """Q [B][DH][DW][3] in `dtype`"""
    DH, DW = np.shape(x_hi)[1:3]
    a, b = coefficients(P, x_lo, r, eps, dtype)
    A, B = box_mean(a, r), box_mean(b, r)
    return upsample(A, DH, DW) * luma(x_hi, dtype)[..., None] + upsample(B, DH, DW)


def inputs(kind, B, work, dst, seed=0):
    """(P, X_lo, X_hi) float32, frames distinct: smooth ramps (variance far below e: the moments cancel worst), uniform noise, a step edge.
    X_lo is X_hi resampled to the working size, as a scaled call has it."""
    (H, W), (DH, DW) = work, dst
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(DH) / DH, np.arange(DW) / DW, indexing="ij")
    ly, lx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    P, X = np.zeros((B, H, W, 3)), np.zeros((B, DH, DW, 3))
    for b in range(B):
        for c in range(3):
            u, v, o = rng.uniform(0.5, 40.0, 2), rng.uniform(0.5, 40.0, 2), rng.uniform(60.0, 180.0, 2)
            if kind == "ramp":
                X[b, ..., c] = o[0] + u[0] * yy + u[1] * xx
                P[b, ..., c] = o[1] + v[0] * ly - v[1] * lx
            elif kind == "noise":
                X[b, ..., c] = rng.uniform(0.0, 255.0, (DH, DW))
                P[b, ..., c] = rng.uniform(0.0, 255.0, (H, W))
            elif kind == "step":
                k = rng.uniform(0.3, 0.7)
                X[b, ..., c] = np.where(xx + 0.3 * yy < k, o[0] - 50.0, o[0] + 70.0)
                P[b, ..., c] = np.where(lx + 0.3 * ly < k, o[1] + 60.0, o[1] - 55.0) + v[0] * ly
            else:
                raise ValueError(kind)
    x_hi = X.astype(F)
    x_lo = x_hi if (H, W) == (DH, DW) else R.resample(x_hi, H, W).astype(F)
    return P.astype(F), x_lo, x_hi


def naive_error(case, kind, eps):
    """largest |float32 restatement - float64 reference| over one frame of the case's inputs"""
    work, dst, r = CASES[case]
    P, lo, hi = inputs(kind, 1, work, dst)
    return float(np.abs(stage(P, lo, hi, r, eps, F).astype(np.float64) - stage(P, lo, hi, r, eps)).max())


# The yardstick, measured on the CPU with naive_error() and recorded in profiles/guided.txt: the kernels stay within TOL_FACTOR of it per case.
TOL_FACTOR = 4.0
NAIVE_ERR = {
    ("a_r1", "ramp", 0.0001): 5.897e-04,
    ("a_r1", "ramp", 0.01): 3.349e-05,
    ("a_r1", "noise", 0.0001): 1.933e-02,
    ("a_r1", "noise", 0.01): 2.078e-04,
    ("a_r1", "step", 0.0001): 3.840e-03,
    ("a_r1", "step", 0.01): 1.328e-04,
    ("a_r4", "ramp", 0.0001): 3.550e-04,
    ("a_r4", "ramp", 0.01): 4.478e-05,
    ("a_r4", "noise", 0.0001): 5.727e-04,
    ("a_r4", "noise", 0.01): 1.379e-04,
    ("a_r4", "step", 0.0001): 1.665e-03,
    ("a_r4", "step", 0.01): 1.095e-04,
    ("a_r9", "ramp", 0.0001): 4.535e-04,
    ("a_r9", "ramp", 0.01): 6.753e-05,
    ("a_r9", "noise", 0.0001): 1.514e-03,
    ("a_r9", "noise", 0.01): 3.681e-04,
    ("a_r9", "step", 0.0001): 6.031e-05,
    ("a_r9", "step", 0.01): 4.283e-05,
    ("b", "ramp", 0.0001): 4.344e-04,
    ("b", "ramp", 0.01): 4.366e-05,
    ("b", "noise", 0.0001): 9.343e-04,
    ("b", "noise", 0.01): 2.178e-04,
    ("b", "step", 0.0001): 6.049e-03,
    ("b", "step", 0.01): 1.292e-04,
    ("c", "ramp", 0.0001): 5.310e-04,
    ("c", "ramp", 0.01): 3.971e-05,
    ("c", "noise", 0.0001): 3.621e-05,
    ("c", "noise", 0.01): 2.981e-05,
    ("c", "step", 0.0001): 1.951e-03,
    ("c", "step", 0.01): 9.072e-05,
    ("d", "ramp", 0.0001): 3.586e-04,
    ("d", "ramp", 0.01): 7.347e-05,
    ("d", "noise", 0.0001): 1.948e-02,
    ("d", "noise", 0.01): 6.367e-04,
    ("d", "step", 0.0001): 2.827e-04,
    ("d", "step", 0.01): 2.228e-04,
    ("e", "ramp", 0.0001): 3.031e-04,
    ("e", "ramp", 0.01): 7.100e-05,
    ("e", "noise", 0.0001): 5.777e-05,
    ("e", "noise", 0.01): 5.980e-05,
    ("e", "step", 0.0001): 3.315e-03,
    ("e", "step", 0.01): 2.528e-04,
    ("f", "ramp", 0.0001): 4.807e-04,
    ("f", "ramp", 0.01): 4.614e-05,
    ("f", "noise", 0.0001): 4.834e-05,
    ("f", "noise", 0.01): 4.832e-05,
    ("f", "step", 0.0001): 4.057e-02,
    ("f", "step", 0.01): 3.618e-04,
    ("g", "ramp", 0.0001): 2.625e-04,
    ("g", "ramp", 0.01): 6.631e-05,
    ("g", "noise", 0.0001): 1.449e-04,
    ("g", "noise", 0.01): 1.017e-04,
    ("g", "step", 0.0001): 2.848e-03,
    ("g", "step", 0.01): 2.225e-04,
    ("h_row", "ramp", 0.0001): 4.632e-03,
    ("h_row", "ramp", 0.01): 6.659e-05,
    ("h_row", "noise", 0.0001): 3.785e-02,
    ("h_row", "noise", 0.01): 2.531e-04,
    ("h_row", "step", 0.0001): 1.178e-02,
    ("h_row", "step", 0.01): 2.229e-04,
    ("h_col", "ramp", 0.0001): 4.316e-03,
    ("h_col", "ramp", 0.01): 7.589e-05,
    ("h_col", "noise", 0.0001): 6.067e-03,
    ("h_col", "noise", 0.01): 1.721e-04,
    ("h_col", "step", 0.0001): 2.978e-02,
    ("h_col", "step", 0.01): 3.725e-04,
    ("j", "ramp", 0.0001): 8.207e-04,
    ("j", "ramp", 0.01): 3.933e-05,
    ("j", "noise", 0.0001): 1.953e-03,
    ("j", "noise", 0.01): 1.878e-04,
    ("j", "step", 0.0001): 5.297e-03,
    ("j", "step", 0.01): 9.243e-05,
    ("k", "ramp", 0.0001): 1.583e-03,
    ("k", "ramp", 0.01): 3.933e-05,
    ("k", "noise", 0.0001): 8.571e-02,
    ("k", "noise", 0.01): 2.518e-04,
    ("k", "step", 0.0001): 1.127e-02,
    ("k", "step", 0.01): 7.753e-05,
}

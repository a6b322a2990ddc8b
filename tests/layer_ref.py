"""Per-layer float64 references for the activation taps (rrv_debug_copy_tensor_ex) and the error model that bounds
each kernel's own rounding.  Plain module (no pytest): imported by tests/test_gpu_layers.py and tests/test_layer_ref.py.

Teacher forcing: every stage is evaluated in float64 from the GPU's OWN input tap(s), the unfolded checkpoint weights and
the saved state, so a check sees one kernel's error and nothing upstream (Decoder.norm[0]'s amplification of encoder
noise, which is why the end-to-end bounds of state_bounds.py are loose, never enters).

Error model.  Next to its value v every stage carries a magnitude m, the same arithmetic on absolute values:
  conv      v = W * x + b                 m = |W| * |x| + |b|   (folded KernelFilter convs: the absolute folded product)
  relu / lrelu / max-pool / clamp         1-Lipschitz: m unchanged (pooled with the same window)
  + r       v = v + r                     m = m + |r|
  norm      v = clamp((v - mean) rstd)    m = (m + |mean|) rstd
  AdaIN     v = norm(v) std + smean       m = ((m + |mean|) rstd) |std| + |smean|
and the bound is  |gpu - ref| <= K_family 2^-24 m + 2^-24 |ref|  element-wise, one K per kernel family (FAMILIES).

Measured ratios max |gpu - ref| / (2^-24 m) on an MI355X over the shapes of tests/test_gpu_layers.py (three forced kernel
choices, the headline launch and split K) are in MEASURED; each K is set from the largest one of its family (see K).
"""
import numpy as np
import torch
import torch.nn.functional as TF

U = 2.0 ** -24

FAMILIES = ("direct", "f23", "ups", "f43", "splitk")

# max |gpu - ref| / (2^-24 m) per family, over every tap and shape of tests/test_gpu_layers.py on an MI355X (the worst tap):
#   direct  30.7  c11 (conv_first: the grey fold multiplies 1/std into the weights, so its rounding is relative to the
#                 un-normalised pixel, not to |x|; conv_last's pre-clamp output: 1.6)
#   f23      3.7  c31 (F(2x2,3x3); per tap 1.6 .. 3.7; the unsplit KernelFilter down conv 0.39)
#   ups      9.2  xs3 (the upsample-fused conv1: a 2.9 .. 4.8; its fused 1x1 shortcut 8.0 .. 9.2)
#   f43     12.5  c21 (F(4x4,3x3) with the balanced points; per tap 4.4 .. 12.5)
#   splitk   0.22 d (split-K sum: m carries |F1| |W_down| * |x|, far above the partial sums' own magnitude)
MEASURED = {"direct": 30.7, "f23": 3.7, "ups": 9.2, "f43": 12.5, "splitk": 0.22}
# K = 2 x the measured maximum, rounded up (at most 4x it): margin for shapes and images outside the measured set while
# still rejecting the defects tests/test_layer_ref.py injects (the smallest of them, one weight off by 2^-8, is at 2480)
K = {"direct": 62.0, "f23": 8.0, "ups": 19.0, "f43": 25.0, "splitk": 0.5}

# the tap indices of rrv_debug_copy_tensor_ex
TAP_NAMES = ["c11", "p1", "c21", "p2", "c31", "c32", "c33", "p3", "c41",
             "d", "f1", "f2", "f3", "xs4", "a4", "o4", "xs3", "a3", "o3", "xs2", "a2", "o2", "dpart",
             "q11", "q1", "q21", "q2", "q31", "q32", "q33", "qa4", "qa3", "qa2"]
TAP = {n: i for i, n in enumerate(TAP_NAMES)}
TWIN = {"c11": "q11", "p1": "q1", "c21": "q21", "p2": "q2", "c31": "q31", "c32": "q32", "c33": "q33",
        "a4": "qa4", "a3": "qa3", "a2": "qa2"}

# saved-state blob layout: 11 norm layers x (mean, rstd, lo, hi), 6 filters [32][32], 4 x (mean, std)
NORM_CH = [512, 512, 256, 128, 64, 256, 256, 128, 128, 64, 64]
FILTER_NAMES = ["Filter1.F1", "Filter1.F2", "Filter2.F1", "Filter2.F2", "Filter3.F1", "Filter3.F2"]
STYLE_CH = [64, 128, 256, 512]


def parse_state(blob):
    b = np.asarray(blob, np.float32).reshape(-1).astype(np.float64)
    st, o = {"norm": [], "filt": {}, "sty": []}, 0
    for C in NORM_CH:
        st["norm"].append(tuple(b[o + i * C:o + (i + 1) * C] for i in range(4)))
        o += 4 * C
    for n in FILTER_NAMES:
        st["filt"][n] = b[o:o + 1024].reshape(32, 32)
        o += 1024
    for C in STYLE_CH:
        st["sty"].append((b[o:o + C], b[o + C:o + 2 * C]))
        o += 2 * C
    assert o == b.size
    return st


# ---- layouts ----------------------------------------------------------------------------------------------------------

def ring_to_hwc(flat, H, W, C):
    """Ring-layout NHWC image [H+2][W+2][C] -> [H][W][C]; the 1-pixel ring must be exactly 0."""
    a = np.asarray(flat).reshape(H + 2, W + 2, C)
    ring = np.concatenate([a[0].ravel(), a[H + 1].ravel(), a[:, 0].ravel(), a[:, W + 1].ravel()])
    assert not np.any(ring), "nonzero ring: %d entries" % np.count_nonzero(ring)
    return a[1:H + 1, 1:W + 1]


def p8_to_hwc(flat, H, W, C):
    """Channel-chunk-major image [C/8][H+2][W+8][8], pixel x at stored column x + 4 -> [H][W][C]; rows 0 and H+1 and columns
    0..3 and W+4..W+7 must be exactly 0."""
    a = np.asarray(flat).reshape(C // 8, H + 2, W + 8, 8)
    pad = np.concatenate([a[:, 0].ravel(), a[:, H + 1].ravel(), a[:, :, :4].ravel(), a[:, :, W + 4:].ravel()])
    assert not np.any(pad), "nonzero P8 padding: %d entries" % np.count_nonzero(pad)
    return np.ascontiguousarray(a[:, 1:H + 1, 4:W + 4].transpose(1, 2, 0, 3).reshape(H, W, C))


def to_hwc(flat, layout, H, W, C):
    return p8_to_hwc(flat, H, W, C) if layout == 1 else ring_to_hwc(flat, H, W, C)


# ---- float64 operators on output row ranges ------------------------------------------------------------------------------

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _rows(x, r0, r1, ups):
    """Rows [r0, r1) of x (or of its nearest-x2 upsample), zero outside, columns padded by one zero each side: [r, W+2, C]."""
    Hs = x.shape[0] * (2 if ups else 1)
    idx = np.arange(r0, r1)
    ok = (idx >= 0) & (idx < Hs)
    src = np.clip(idx, 0, Hs - 1) // (2 if ups else 1)
    a = np.asarray(x, np.float64)[src]
    if ups:
        a = np.repeat(a, 2, axis=1)
    a = a * ok[:, None, None]
    return np.pad(a, ((0, 0), (1, 1), (0, 0)))


def conv3(x, w, b, y0, y1, ups=False):
    """Rows [y0, y1) of conv3x3(pad 1)(x or up(x)) + b in float64: (v, m) as [y1-y0, W', Cout]."""
    a = _rows(x, y0 - 1, y1 + 1, ups)
    xt = _t(a).permute(2, 0, 1)[None]
    wt = _t(w)
    with torch.no_grad():
        v = TF.conv2d(xt, wt)[0].permute(1, 2, 0).numpy()
        m = TF.conv2d(xt.abs(), wt.abs())[0].permute(1, 2, 0).numpy()
    if b is not None:
        b = np.asarray(b, np.float64)
        v, m = v + b, m + np.abs(b)
    return v, m


def conv1(x, w, y0, y1):
    """Rows [y0, y1) of the bias-free 1x1 convolution x @ w.T: (v, m)."""
    a = np.asarray(x[y0:y1], np.float64)
    w2 = np.asarray(w, np.float64).reshape(w.shape[0], -1)
    return a @ w2.T, np.abs(a) @ np.abs(w2).T


def pool(v, m):
    H2, W2 = v.shape[0] // 2, v.shape[1] // 2
    f = lambda a: a[:2 * H2, :2 * W2].reshape(H2, 2, W2, 2, -1).max(axis=(1, 3))
    return f(v), f(m)


def relu(v, m):
    return np.maximum(v, 0.0), m


def lrelu(v, m):
    return np.where(v >= 0, v, 0.2 * v), m


def norm(v, m, n):
    mean, rstd, lo, hi = n
    return np.minimum(hi, np.maximum(lo, (v - mean) * rstd)), (m + np.abs(mean)) * rstd


def adain(v, m, n, s):
    v, m = norm(v, m, n)
    return v * s[1] + s[0], m * np.abs(s[1]) + np.abs(s[0])


def grey_input(img_u8):
    """image_to_tensor + TransformerNet.RGB2Gray (quirk Q5) in float64 on the constants the float32 network uses: [H,W,3]."""
    MEAN = np.array([0.485, 0.456, 0.406], np.float32).astype(np.float64)
    STD = np.array([0.229, 0.224, 0.225], np.float32).astype(np.float64)
    x = img_u8[..., ::-1].astype(np.float64) / 255.0
    g = x[..., 2:3] * float(np.float32(0.299)) + x[..., 1:2] * float(np.float32(0.587)) + x[..., 0:1] * float(np.float32(0.114))
    return (g - MEAN) / STD


# ---- the stages: one per tap, read from run_encoder / filter_down / transfer_device / resblock_frame / run_last ----------
# (name, launch, inputs, op): `launch` is the position of the producing kernel in a launch's profile (sum_parts excluded),
# the stage's family is read from that kernel's name.  Every op is op(inp, w, st, y0, y1) -> (v, m) for output rows [y0, y1).

def _enc(i):
    return "Encoder.slice.%d" % i


def _enc_stage(i, post, n0=False):
    def op(inp, w, st, y0, y1):
        yy0, yy1 = (2 * y0, 2 * y1) if "pool" in post else (y0, y1)
        v, m = conv3(inp[0], w[_enc(i) + ".weight"], w[_enc(i) + ".bias"], yy0, yy1)
        v, m = relu(v, m)
        if "pool" in post:
            v, m = pool(v, m)
        if n0:
            v, m = norm(v, m, st["norm"][0])      # run_encoder fuses Decoder.norm[0] into conv4_1's epilogue
        return v, m
    return op


def _first(inp, w, st, y0, y1):
    return relu(*conv3(inp[0], w[_enc(0) + ".weight"], w[_enc(0) + ".bias"], y0, y1))


def _down(f):
    """d = lrelu(F1 (down(cur) + b)): filter_down's folded, split-K summed KernelFilter.down_sample."""
    def op(inp, w, st, y0, y1):
        p = "Decoder.Filter%d.down_sample.0." % (f + 1)
        v, m = conv3(inp[0], w[p + "weight"], w[p + "bias"], y0, y1)
        F1 = st["filt"]["Filter%d.F1" % (f + 1)]
        return lrelu(v @ F1.T, m @ np.abs(F1).T)
    return op


def _up(f):
    """f = cur + up(F2 d) (+ Decoder.norm[1] and AdaIN with relu4_1 after Filter3): the folded KernelFilter.upsample."""
    def op(inp, w, st, y0, y1):
        p = "Decoder.Filter%d.upsample.0." % (f + 1)
        F2 = st["filt"]["Filter%d.F2" % (f + 1)]
        d = np.asarray(inp[0], np.float64)
        v, _ = conv3(d @ F2.T, w[p + "weight"], w[p + "bias"], y0, y1)
        _, m = conv3(np.abs(d) @ np.abs(F2).T, np.abs(w[p + "weight"]), w[p + "bias"], y0, y1)
        r = np.asarray(inp[1][y0:y1], np.float64)
        v, m = v + r, m + np.abs(r)
        if f == 2:
            v, m = adain(v, m, st["norm"][1], st["sty"][3])
        return v, m
    return op


RES = {"slice4": (5, 6, 2, 2), "slice3": (7, 8, 3, 1), "slice2": (9, 10, 4, 0)}   # (norm1, norm2, AdaIN norm, style) indices


def _shortcut(blk):
    def op(inp, w, st, y0, y1):
        return conv1(inp[0], w["Decoder.%s.conv_shortcut.weight" % blk], y0, y1)
    return op


def _conv1(blk):
    def op(inp, w, st, y0, y1):
        v, m = conv3(inp[0], w["Decoder.%s.conv1.weight" % blk], w["Decoder.%s.conv1.bias" % blk], y0, y1, ups=True)
        v, m = lrelu(v, m)
        return norm(v, m, st["norm"][RES[blk][0]])
    return op


def _conv2(blk):
    def op(inp, w, st, y0, y1):
        n1, n2, na, s = RES[blk]
        v, m = conv3(inp[0], w["Decoder.%s.conv2.weight" % blk], w["Decoder.%s.conv2.bias" % blk], y0, y1)
        v, m = lrelu(v, m)
        v, m = norm(v, m, st["norm"][n2])
        xs = np.asarray(inp[1], np.float64)[np.arange(y0, y1) // 2]
        xs = np.repeat(xs, 2, axis=1)[:, :v.shape[1]]
        return adain(v + xs, m + np.abs(xs), st["norm"][na], st["sty"][s])
    return op


def _last(inp, w, st, y0, y1):
    return conv3(inp[0], w["Decoder.slice1.weight"], w["Decoder.slice1.bias"], y0, y1)


# name -> (launch position, input taps, op, (H, W, C) of the output from (H, W) of the frame).  "frame": the uint8 input
# through grey_input; "pre": the pre-clamp output (rrv_get_preclamp_image).  f1 / f2 are checked as two kernels in one
# (their d is overwritten by the next filter); d and f3 are teacher-forced on the last filter.
def _g(k, C):
    return lambda H, W: (H // k, W // k, C)


def _gd(k, C):
    return lambda H, W: (H // 8 * 8 // k, W // 8 * 8 // k, C)


STAGES = {
    "c11": (0, ["frame"], _first, _g(1, 64)),
    "p1": (1, ["c11"], _enc_stage(2, ("pool",)), _g(2, 64)),
    "c21": (2, ["p1"], _enc_stage(5, ()), _g(2, 128)),
    "p2": (3, ["c21"], _enc_stage(7, ("pool",)), lambda H, W: (H // 2 // 2, W // 2 // 2, 128)),
    "c31": (4, ["p2"], _enc_stage(10, ()), lambda H, W: (H // 4, W // 4, 256)),
    "c32": (5, ["c31"], _enc_stage(12, ()), lambda H, W: (H // 4, W // 4, 256)),
    "c33": (6, ["c32"], _enc_stage(14, ()), lambda H, W: (H // 4, W // 4, 256)),
    "p3": (7, ["c33"], _enc_stage(16, ("pool",)), lambda H, W: (H // 8, W // 8, 256)),
    "c41": (8, ["p3"], _enc_stage(19, (), n0=True), lambda H, W: (H // 8, W // 8, 512)),
    "d": (13, ["f2"], _down(2), lambda H, W: (H // 8, W // 8, 32)),
    "f3": (14, ["d", "f2"], _up(2), lambda H, W: (H // 8, W // 8, 512)),
    "xs4": (15, ["f3"], _shortcut("slice4"), lambda H, W: (H // 8, W // 8, 256)),
    "a4": (15, ["f3"], _conv1("slice4"), lambda H, W: (H // 8 * 2, W // 8 * 2, 256)),
    "o4": (16, ["a4", "xs4"], _conv2("slice4"), lambda H, W: (H // 8 * 2, W // 8 * 2, 256)),
    "xs3": (17, ["o4"], _shortcut("slice3"), lambda H, W: (H // 8 * 2, W // 8 * 2, 128)),
    "a3": (17, ["o4"], _conv1("slice3"), lambda H, W: (H // 8 * 4, W // 8 * 4, 128)),
    "o3": (18, ["a3", "xs3"], _conv2("slice3"), lambda H, W: (H // 8 * 4, W // 8 * 4, 128)),
    "xs2": (19, ["o3"], _shortcut("slice2"), lambda H, W: (H // 8 * 4, W // 8 * 4, 64)),
    "a2": (19, ["o3"], _conv1("slice2"), lambda H, W: (H // 8 * 8, W // 8 * 8, 64)),
    "o2": (20, ["a2", "xs2"], _conv2("slice2"), lambda H, W: (H // 8 * 8, W // 8 * 8, 64)),
    "pre": (21, ["o2"], _last, lambda H, W: (H // 8 * 8, W // 8 * 8, 3)),
}
# the launch order of one transfer (profile rows without sum_parts): conv_first, 8 encoder convs, (down, up) x 3,
# (conv1 + shortcut, conv2) x 3, conv_last
N_LAUNCHES = 22
FOLDED = ("f1", "f2")      # d of Filter1 / Filter2 is not visible after the launch: checked with d recomputed (two kernels)


def _composite(f):
    """f1 / f2 from their input cur: d recomputed in float64 (its error enters through |W_up F2|), then the up stage."""
    def op(inp, w, st, y0, y1, kd=None, ku=None):
        r0, r1 = max(0, y0 - 1), min(inp[0].shape[0], y1 + 1)
        dv, dm = _down(f)(inp, w, st, r0, r1)
        full_v = np.zeros((inp[0].shape[0],) + dv.shape[1:])
        full_m = np.zeros_like(full_v)
        full_v[r0:r1], full_m[r0:r1] = dv, dm
        v, mu = _up(f)([full_v, inp[0]], w, st, y0, y1)
        p = "Decoder.Filter%d.upsample.0." % (f + 1)
        F2 = st["filt"]["Filter%d.F2" % (f + 1)]
        _, md = conv3(full_m @ np.abs(F2).T, np.abs(w[p + "weight"]), None, y0, y1)
        return v, mu, md
    return op


COMPOSITE = {"f1": (9, 10, ["c41"], _composite(0)), "f2": (11, 12, ["f1"], _composite(1))}   # (down launch, up launch, ...)


def strips(H, full_below=96, band=32):
    """Output row ranges to evaluate: everything for small tensors; else the top and bottom borders and one interior band
    (full width, so the right edge is always in)."""
    if H <= full_below:
        return [(0, H)]
    mid = H // 2 - band // 2
    return [(0, band), (mid, mid + band), (H - band, H)]


def family_of(kernel_name, split):
    """Kernel family of a profile row name ("<kernel>@CinxCout@HxW")."""
    k = kernel_name.split("@")[0]
    if k.startswith("conv_f43"):
        return "f43"
    if k.startswith("conv_upw"):
        return "ups"
    if k.startswith("conv_wino"):
        return "splitk" if split else "f23"
    if k.startswith(("conv_first", "conv_last", "conv_mfma")):
        return "direct"
    raise AssertionError("unknown kernel " + kernel_name)


def check(got, v, m, k):
    """Element-wise |got - v| <= k 2^-24 m + 2^-24 |v|: (passes, worst |got - v| / bound, worst |got - v| / (2^-24 m))."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - v)
    bound = k * U * m + U * np.abs(v)
    ratio = err / np.maximum(U * m, 1e-300)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    return bool(np.all(err <= bound)), worst, float(ratio.max()) if err.size else 0.0

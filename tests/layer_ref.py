"""Per-layer float64 references for the activation taps (rrv_debug_copy_tensor_ex) and the error model that bounds
each kernel's own rounding.  Plain module (no pytest): imported by tests/test_gpu_layers.py and tests/test_layer_ref.py (and the
other layer suites; the windows of the pad / crop entries, crop_windows, are tests/test_gpu_window_layers.py's).

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

Frame mode (Stylization(use_Global=False), FRAME_STAGES below) normalises in place with statistics taken per image, so the raw
tensor a statistic was taken from is gone after the launch.  Each statistic is therefore checked against the float64
statistic of the float64 stage (value v, per-element error bound b of what the GPU held, b = K_f 2^-24 m for a raw
convolution output) over the whole tensor of that image:
  mean      the mean of per-element errors is at most the mean of their bounds:
            |mean_gpu - mean64| <= mean(b) + K_stat 2^-24 |mean64|
  variance  x = v + e with |e| <= b:  var(x) = var(v) + 2 cov(v, e) + var(e),  |cov(v, e)| <= sqrt(var v) sqrt(var e)
            (Cauchy-Schwarz on the centred values) and var(e) <= mean(e^2) <= mean(b^2), so
            |var_gpu - var64| <= 2 sqrt(var64) rms(b) + mean(b^2) + K_stat 2^-24 (var64 + 1e-8),
            var_gpu recovered as 1 / rstd_gpu^2 - 1e-8 (biased, over H x W of the image alone).
The normalised taps are teacher-forced on the GPU's OWN statistics, (v - mean_gpu) rstd_gpu with magnitude
(m + |mean_gpu|) rstd_gpu, so they see the convolution's and pointwise_k's rounding and no statistic's:
  |gpu - ref| <= 2^-24 (K_f m_conv + K_point m_point + |ref|)
with m_conv the convolution's magnitude carried through the later steps' scales only, and m_point the magnitude of every
pointwise_k pass's own result carried the same way.  The families of the frame-mode path:
  stat   the statistics kernels' and blend_sets_k's own rounding.  Never visible alone at a statistic point (its input is
         overwritten), so there the measured figure is the EXCESS (err - mean(b)) / (2^-24 |mean64|) (resp. the variance
         form), 0 where the producer's term covers the error; blend_sets_k's float32 sum against the float64 sum of the
         styles' blobs, relative to the same sum on absolute values, is measured directly.
  point  pointwise_k.  Its input is overwritten in place, so it is never visible alone either: the measured figure is the
         WHOLE error of a normalised tap over 2^-24 m_point (an upper estimate: the convolution's rounding is in it), and the
         bound still carries the convolution's own term with its existing K.
  pred   rect_sums_k + pred_mean_k + fc_filter_k against the reference's form (zero-padded 3 x 3 down_sample convolution,
         mean over H x W, FC with the style half), magnitude: the same arithmetic on absolute values through the FC.
The preparation pass (tests/prep_ref.py) adds pstat (the two-pass and merged statistics against their own raw tap), gemm
(conv_mfma_k raw outputs) and ppred (a tap's mean + the FC); their forms are in that module's docstring.
"""
import numpy as np
import torch
import torch.nn.functional as TF

U = 2.0 ** -24

FAMILIES = ("direct", "f23", "ups", "f43", "splitk", "stat", "point", "pred", "mnorm", "mfilt", "pstat", "gemm", "ppred",
            "once", "pack32", "grey", "fold")      # the last four: the weight packs and folds (tests/pack_ref.py)

# max |gpu - ref| / (2^-24 m) per family, over every tap and shape of tests/test_gpu_layers.py on an MI355X (the worst tap):
#   direct  30.7  c11 (conv_first: the grey fold multiplies 1/std into the weights, so its rounding is relative to the
#                 un-normalised pixel, not to |x|; conv_last's pre-clamp output: 1.6)
#   f23      3.7  c31 (F(2x2,3x3); per tap 1.6 .. 3.7; the unsplit KernelFilter down conv 0.39)
#   ups      9.2  xs3 (the upsample-fused conv1: a 2.9 .. 4.8; its fused 1x1 shortcut 8.0 .. 9.2)
#   f43     12.5  c21 (F(4x4,3x3) with the balanced points; per tap 4.4 .. 12.5)
#   splitk   0.24 d (split-K sum: m carries |F1| |W_down| * |x|, far above the partial sums' own magnitude; 0.22 on the
#                 global path, 0.24 in frame mode at 1032 x 8)
# and over every case of tests/test_gpu_frame_mode_layers.py (frame mode 1 x 8 x 8 .. 16 x 136 x 200, 2 x 640 x 640, the host
# entry's second launch sequence, one grouped multi-style launch; the convolutions stayed inside the figures above with their
# raw epilogues: direct 30.7, f23 3.68, ups 9.02):
#   stat     2.91 blend_sets_k, image 6 of the grouped multi-style launch (a float32 sum of four rounded products: up to 4
#                 by construction; image 0: 1.47).  The statistic points' excess over their producer's term was 0 at every
#                 point of every image (worst: 0.30 of the bound, norm0 at 16 x 8): chan_stat1_k accumulates in float64.
#   point    3.73 a3 at 640 x 640 (the whole error of the tap over the pointwise result's magnitude; a taps 3.6 .. 3.7, c41
#                 3.2, o taps 1.2 .. 1.7)
#   pred     1.21 Filter1.F1 at 8 x 8 (one pixel; every other shape 0.05 .. 0.19)
# and the two families of the masked multi-style walk (tests/mask_layer_ref.py, every case of tests/test_gpu_mask_layers.py):
#   mnorm    3.64 a2, image 15 of 16 x 136 x 200 at S = 4 (mask_norm_k, the whole error of the tap over the pass's own
#                 magnitude, as `point`; a taps 1.9 .. 3.7, f3 2.6, o taps 0.9 .. 1.2)
#   mfilt    0.314 d, image 7 of 16 x 136 x 200 at S = 4 (mask_filter_k alone against its own split-K slices; m carries
#                 |F2|(p) |F1|(p) (sum |slices| + |bias|))
# measured over the cases 1 x 8 x 8 .. 16 x 136 x 200 (S = 1 .. 8); the split-4, split-1, pad / crop and host-entry cases have
# NOT yet contributed a figure.  The convolutions stayed inside their figures: direct 28.1, f23 5.24 against its K of 8, ups 10.2
# against its K of 19.
# and the three families of the preparation pass (tests/prep_ref.py), over every case of tests/test_gpu_prep_layers.py (resident
# 1 x 8 x 8 .. 5 x 136 x 200 at all 14 sync points, 1 x 520 x 520 and 4 x 4104 x 8 at the full-resolution ones, three style sizes,
# two styles, one streamed group at every sync point, five frames in groups of 1, 2 and 3; profiles/prep_layers.txt):
#   pstat    4.24 norm[2] <- o4 at 1 x 8 x 8 (four pixels; the variance recovered from a float32 rstd carries that rstd's 1.5
#                 ulp twice; 3.3 .. 4.2 at every size, the merged statistics 3.99, the style statistics 3.82; the means <= 0.5)
#   gemm     7.95 xs2 at 520 x 520 (conv_mfma_k: one float32 MFMA accumulator per output over all of K, no split; the 1 x 1
#                 shortcuts 5.9 .. 8.0, the 512 -> 32 predictor convolutions up to 6.0)
#   ppred    1.91 Filter3.F2 at 5 x 136 x 200 (a 64-term float32 sum in fc_filter_k; 1.0 .. 1.9)
# The preparation-only instantiations stayed inside the existing figures: f23 2.44 (conv2 raw; the unsplit folded 512 -> 32 and
# 32 -> 512 convolutions below it), ups 5.2 (the nine-product conv_upw<E_LRELU>), point 2.77.
# and over every case of tests/test_gpu_instantiations.py (profiles/instantiations.txt), all inside the figures above, no K touched:
#   a  blended frames 3 x 72 x 104, per-image conv4_1    f23 2.95 (c41 itself 1.7 .. 2.1), f43 7.13 (mode 2, the P8 chain inside the
#                                                        grouped launch), ups 5.93, splitk 0.13, direct 28.0, stat 2.0 (blend_sets_k)
#   b  cached features, per-image pointwise_k            point 1.92 (c41, the whole error over the pass's own magnitude), stat 2.03
#   c  filter_down with per-image weights, 2 frames      split 4 (64 x 5136): splitk 0.215 frame mode, 0.166 blended; unsplit
#                                                        (64 x 16400): d 0.48 / 0.57 as f23; c41 2.4 (f23) / 2.6 (point, frame mode)
#   d  direct-form encoder (conv_mfma_k on 3 x 3 layers) gemm 5.74 (c21, image 4 of 5 x 40 x 56; per tap 3.2 .. 5.7: K = 2304 at most,
#                                                        against 7.95 at K = 4608 in the preparation pass)
# Every negative control (an image on its neighbour's state set) landed at 1.1e3 .. 3.9e4 of its bound.
# and the four families of the weight packs and folds (tests/pack_ref.py), over every buffer of tests/test_gpu_packs.py on
# synthetic_weights(0) (profiles/packs.txt).  Each has a derived cap n, the float32 roundings on an element's path (the docstring of
# tests/test_gpu_packs.py); K is that cap where the measured maximum reaches a quarter of it, else 2 x the measured maximum, rounded up:
#   once     0.5  pack_f43_k and pack_ups5_k, in ulp32 of the extended-precision value: every element is the one rounding of it
#                 (cap 1/2 + 2^-20 for the order of the kernel's float64 evaluation; 0.5 measured on every buffer)
#   pack32   2.60 pack_wino_k, pk_wino of Encoder.slice.10 (cap n = 4, so K = 4; the nine-product form 2.21, the folded
#                 KernelFilters' packs 2.02 .. 2.48, at one set and set-major alike)
#   grey     1.83 pack_first_grey_k (caps 3 / 4 / 29 for W1 / W0 / the folded bias; K = 4 applies under each part's own cap)
#   fold     5.44 fold_up_k, image 1 of the grouped launch (cap n = 32, so K = 11; fold_down_k 4.92, its bias 3.01: a 32-term
#                 float32 sum against sum |F||W|)
# Image 1's folded weights on image 0's filter (the control): ratios 3.0e6 .. 8.4e6, its pack on image 0's folded weights 7e10 and more.
# and over every case of tests/test_gpu_window_layers.py (the windowed launches of the pad / crop entries at 192 x 192, each stage on its
# window alone; profiles/windows.txt), all inside the figures above, no K touched:
#   ups      8.36 xs2 (the fused shortcut, kinds f43_p8 / f43_nhwc at 47 x 49; f23 7.67, blended 6.68); a2 2.7 (f23), 4.42 (both f43 kinds;
#                 the P8 twin written through a window holds the NHWC launch's bits), 2.4 blended with per-image state
#   f23      1.82 o2 (conv_wino_split_k<54,0> windowed; <54,1> with per-image state 1.64)
#   f43      2.74 o2 (conv_f43_k<54,0> and <54,1> windowed: the same figure in both layouts)
#   direct   1.28 pre (conv_last_k on wl, evaluated where its taps stay inside wo)
# The control (image 1 of the blended call on image 0's set): a2 at 1.96e5, o2 at 4.9e5 in ratio.
MEASURED = {"direct": 30.7, "f23": 3.7, "ups": 9.2, "f43": 12.5, "splitk": 0.24, "stat": 2.91, "point": 3.73, "pred": 1.21, "mnorm": 3.64, "mfilt": 0.314,
            "pstat": 4.24, "gemm": 7.95, "ppred": 1.91, "once": 0.5, "pack32": 2.60, "grey": 1.83, "fold": 5.44}
# K = 2 x the measured maximum, rounded up (at most 4x it): margin for shapes and images outside the measured set while
# still rejecting the defects tests/test_layer_ref.py injects (the smallest of them, one weight off by 2^-8, is at 2480)
K = {"direct": 62.0, "f23": 8.0, "ups": 19.0, "f43": 25.0, "splitk": 0.5, "stat": 6.0, "point": 8.0, "pred": 2.5, "mnorm": 8.0, "mfilt": 0.7,
     "pstat": 9.0, "gemm": 16.0, "ppred": 4.0, "once": 0.5 + 2.0 ** -20, "pack32": 4.0, "grey": 4.0, "fold": 11.0}

# the tap indices of rrv_debug_copy_tensor_ex
TAP_NAMES = ["c11", "p1", "c21", "p2", "c31", "c32", "c33", "p3", "c41",
             "d", "f1", "f2", "f3", "xs4", "a4", "o4", "xs3", "a3", "o3", "xs2", "a2", "o2", "dpart",
             "q11", "q1", "q21", "q2", "q31", "q32", "q33", "qa4", "qa3", "qa2", "lm0", "lm1", "lm2", "lm3"]
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


def fold_up(f, d, w, st, y0, y1):
    """up(F2 d) + b: the folded KernelFilter.upsample product alone, (v, m) with the absolute folded product as magnitude."""
    p = "Decoder.Filter%d.upsample.0." % (f + 1)
    F2 = st["filt"]["Filter%d.F2" % (f + 1)]
    d = np.asarray(d, np.float64)
    v, _ = conv3(d @ F2.T, w[p + "weight"], w[p + "bias"], y0, y1)
    _, m = conv3(np.abs(d) @ np.abs(F2).T, np.abs(w[p + "weight"]), w[p + "bias"], y0, y1)
    return v, m


def _up(f):
    """f = cur + up(F2 d) (+ Decoder.norm[1] and AdaIN with relu4_1 after Filter3): the folded KernelFilter.upsample."""
    def op(inp, w, st, y0, y1):
        v, m = fold_up(f, inp[0], w, st, y0, y1)
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
    if k.startswith("conv_mfma<") and k[len("conv_mfma<"):].split(",")[1].strip() == "9":
        return "gemm"       # the direct-form encoder (RRV_DIRECT_LAYERS): conv_mfma_k on a 3 x 3 layer, one float32 accumulator over 9 Cin
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


# ---- the windows of the pad / crop entries (rrv_transfer_frames*, RRV_TF_PAD_CROP) ------------------------------------------------------
# Restated from the comments of transfer_device and conv_params, nothing imported from the library.  A source frame of H x W is reflect-
# padded to padded_size(H) x padded_size(W) on its way into conv_first_k and the crop that starts at (CROP0, CROP0) is delivered, so the
# full-resolution block computes windows only.  A window is (y0, x0, y1, x1) in pixels of its own tensor, y1 / x1 exclusive:
#   wl   what conv_last_k computes: the crop rounded out to its 16 x 16 tiles
#   wo   what slice2.conv2 writes in o2: the crop + one halo pixel, rounded out to 16 (to the 32 x 32 items of conv_f43_k where conv2 runs on it)
#   wa   what the shortcut-fused conv1 really writes in a2 (or its P8 twin): wo + one halo pixel rounded out to 16 is what transfer_device
#        asks for, conv_params rounds that out to the kernel's 32 x 32 items, clipped to the frame rounded up to 32
#   xs   wa halved: what the same launch writes in xs2, at half the resolution
# Every round-out stops at the frame rounded up to the tile; an element of a window beyond the frame itself is never stored.
CROP0 = 64


def padded_size(n):
    """ReshapeTool.process: n + 2 x 64 rounded up to a multiple of 64."""
    return (n + 128 + 63) // 64 * 64


def _grow(lo, hi, halo, lim):
    """[lo, hi) + halo pixels each side, rounded out to 16, inside [0, lim rounded up to 16)."""
    return max(lo - halo, 0) & ~15, min((hi + halo + 15) & ~15, (lim + 15) & ~15)


def _out32(lo, hi, lim):
    return lo & ~31, min((hi + 31) & ~31, (lim + 31) & ~31)


def _axis_windows(n, conv2_f43):
    P = padded_size(n)
    crop = (CROP0, CROP0 + n)
    wl = _grow(*crop, 0, P)
    wo = _grow(*crop, 1, P)
    if conv2_f43:
        wo = _out32(*wo, P)
    wa = _out32(*_grow(*wo, 1, P), P)
    return {"P": P, "crop": crop, "wl": wl, "wo": wo, "wa": wa, "xs": (wa[0] // 2, wa[1] // 2)}


WINDOW_NAMES = ("crop", "wl", "wo", "wa", "xs")


def crop_windows(H, W, conv2_f43):
    """The windows of a pad / crop call on H x W source frames: {"PH", "PW": the padded geometry; "crop", "wl", "wo", "wa", "xs": (y0, x0, y1, x1)}."""
    y, x = _axis_windows(H, conv2_f43), _axis_windows(W, conv2_f43)
    out = {"PH": y["P"], "PW": x["P"]}
    for n in WINDOW_NAMES:
        out[n] = (y[n][0], x[n][0], y[n][1], x[n][1])
    return out


def clip(win, H, W):
    """The part of a window inside an H x W tensor."""
    return max(win[0], 0), max(win[1], 0), min(win[2], H), min(win[3], W)


def inside(a, b):
    """Window a lies in window b (an empty a lies in everything)."""
    return a[2] <= a[0] or a[3] <= a[1] or (b[0] <= a[0] and b[1] <= a[1] and a[2] <= b[2] and a[3] <= b[3])


def reads3(win, H, W):
    """The elements of an H x W input that a 3 x 3 convolution (pad 1) reads for the outputs in `win`; what falls outside the frame is the zero ring."""
    return clip((win[0] - 1, win[1] - 1, win[2] + 1, win[3] + 1), H, W)


def reads_half(win, H, W):
    """The elements of the half-resolution residual that the outputs in `win` of an H x W tensor read: (y // 2, x // 2)."""
    y0, x0, y1, x1 = clip(win, H, W)
    return (y0 // 2, x0 // 2, (y1 + 1) // 2, (x1 + 1) // 2) if y1 > y0 and x1 > x0 else (0, 0, 0, 0)


def pre_checkable(w):
    """The part of wl whose 3 x 3 reads of o2 lie in wo or outside the frame: where the pre-clamp tap of a windowed launch has a reference.  It holds
    the crop (window_faults), not always all of wl: with (CROP0 + n) = 15 (mod 16) wl and wo both end one pixel behind the crop."""
    PH, PW = w["PH"], w["PW"]
    wo, wl = w["wo"], w["wl"]
    lo = lambda v: v if v == 0 else v + 1
    hi = lambda v, lim: v if v >= lim else v - 1
    ok = (lo(wo[0]), lo(wo[1]), hi(wo[2], PH), hi(wo[3], PW))
    return max(wl[0], ok[0]), max(wl[1], ok[1]), min(wl[2], ok[2]), min(wl[3], ok[3])


def window_faults(w):
    """The window rule as conditions on index arithmetic; returns the ones `w` (crop_windows' form) breaks, [] when every consumer reads what
    its producer wrote:
      last   conv_last_k computes every crop pixel, and every o2 element its 3 x 3 taps read for a crop pixel lies in wo or outside the frame
      conv2  every a2 element slice2.conv2 reads for a pixel of wo lies in wa or outside the frame
      res    every xs2 element conv2's upsampled residual reads for a pixel of wo lies in xs"""
    PH, PW = w["PH"], w["PW"]
    bad = []
    if not inside(w["crop"], clip(w["wl"], PH, PW)):
        bad.append("last: a crop pixel outside wl")
    if not inside(reads3(w["crop"], PH, PW), w["wo"]):
        bad.append("last: reads o2 outside wo")
    if not inside(reads3(clip(w["wo"], PH, PW), PH, PW), w["wa"]):
        bad.append("conv2: reads a2 outside wa")
    if not inside(reads_half(w["wo"], PH, PW), w["xs"]):
        bad.append("res: reads xs2 outside its window")
    return bad


def shrink(win, side, tile):
    """`win` with one tile taken off side 0..3 (y0, x0, y1, x1): the negative controls of the window tests."""
    v = list(win)
    v[side] += tile if side < 2 else -tile
    return tuple(v)


def window_mask(win, H, W, layout=0, C=None):
    """Boolean mask of a tap AS STORED that is True on the window's pixels: the ring layout [H+2][W+2][C] keeps pixel (y, x) at (y + 1, x + 1),
    the P8 layout [C/8][H+2][W+8][8] at row y + 1 and column x + 4; layout None: the pre-clamp tap, [H][W][C] with nothing around it."""
    y0, x0, y1, x1 = clip(win, H, W)
    if layout is None:
        m = np.zeros((H, W, C), bool)
        m[y0:y1, x0:x1] = True
    elif layout == 1:
        m = np.zeros((C // 8, H + 2, W + 8, 8), bool)
        m[:, y0 + 1:y1 + 1, x0 + 4:x1 + 4] = True
    else:
        m = np.zeros((H + 2, W + 2, C), bool)
        m[y0 + 1:y1 + 1, x0 + 1:x1 + 1] = True
    return m.reshape(-1)


def window_stage(name, inp, w, st, win):
    """Stage `name` of STAGES on the window `win` of its output alone: (v, m) as [y1-y0][x1-x0][C].  The rows are evaluated at the full width
    of the inputs, so what a column outside the window holds never enters a value inside it beyond the stage's own reads."""
    y0, x0, y1, x1 = win
    v, m = STAGES[name][2](inp, w, st, y0, y1)
    return v[:, x0:x1], m[:, x0:x1]


# ---- frame mode (Stylization(use_Global=False): frame_mode_device) ---------------------------------------------------------
# One launch sequence per up to sixteen images, every image with statistics, predicted filters and folded KernelFilter weights
# of its own in its own state set (rrv_debug_copy_state).  The taps after the launch: c11 .. p3 as in the global path, c41 / a4 /
# a3 / a2 normalised in place, o4 / o3 / o2 normalised + shortcut + normalised + AdaIN in place, d of the last Filter, f1 .. f3.

EPS32 = float(np.float32(1e-8))
NO_LO, NO_HI = float(np.float32(-3.0e38)), float(np.float32(3.0e38))
STAT3 = ["chan_stat1", "chan_stat1_final", "pointwise"]
# the profile rows of one frame-mode launch sequence without sum_parts ("conv": any conv_* row but conv_first / conv_last)
FRAME_SEQ = (["frame_sets_init", "conv_first"] + ["conv"] * 8 + STAT3
             + ["rect_sums", "pred_mean", "fc_filter", "pred_mean", "fc_filter", "conv", "conv"] * 3
             + (["conv"] + STAT3 + ["conv"] + STAT3 + STAT3) * 3 + ["conv_last"])
FRAME_ENC = ("c11", "p1", "c21", "p2", "c31", "c32", "c33", "p3")
FRAME_BLOCKS = (("slice4", "f3", "xs4", "a4", "o4"), ("slice3", "o4", "xs3", "a3", "o3"), ("slice2", "o3", "xs2", "a2", "o2"))
FRAME_STAGES = (FRAME_ENC + ("stat0", "c41", "pred0", "f1", "pred1", "f2", "pred2", "d", "f3", "norm1")
                + tuple(n for _, _, xs, a, o in FRAME_BLOCKS for n in (xs, "stat:" + a, a, "stat2:" + o, "stat3:" + o, o)) + ("pre",))


def frame_families(seq):
    """seq: [(profile row name, followed by sum_parts)] of one frame-mode launch sequence without the sum_parts rows.  Asserts
    that it is FRAME_SEQ (every statistic one chan_stat1 + merge + pointwise, every prediction rectangle sums + predicted
    means + FC, no F(4x4,3x3)) and returns {stage: kernel family} for the convolutions."""
    assert len(seq) == len(FRAME_SEQ), [n for n, _ in seq]
    fams = []
    for (name, split), want in zip(seq, FRAME_SEQ):
        k = name.split("@")[0]
        if want == "conv":
            assert k.startswith("conv_") and not k.startswith(("conv_first", "conv_last")), (name, want)
            f = family_of(name, split)
            assert f != "f43", name
            fams.append(f)
        else:
            assert k == want, (name, want)
            if want in ("conv_first", "conv_last"):
                fams.append("direct")
    keys = (FRAME_ENC + ("c41", "d0", "u0", "d1", "u1", "d2", "u2", "a4", "o4", "a3", "o3", "a2", "o2", "pre"))
    assert len(fams) == len(keys), (len(fams), len(keys))
    return dict(zip(keys, fams))


def check_stat(entry, v, b, kstat):
    """One statistic point: the state set's (mean, rstd, lo, hi) against the float64 statistics of the stage value v [H,W,C]
    with per-element error bound b (module docstring).  Returns (passes, worst fraction of a bound, excess ratio)."""
    mean_g, rstd_g, lo, hi = entry
    C = v.shape[-1]
    v2, b2 = v.reshape(-1, C), np.broadcast_to(b, v.shape).reshape(-1, C)
    mean, var = v2.mean(axis=0), v2.var(axis=0)
    msq = (b2 * b2).mean(axis=0)
    pm, pv = b2.mean(axis=0), 2.0 * np.sqrt(var) * np.sqrt(msq) + msq
    var_g = 1.0 / (rstd_g * rstd_g) - EPS32
    em, ev = np.abs(mean_g - mean), np.abs(var_g - var)
    sm, sv = U * np.abs(mean), U * (var + EPS32)
    bm, bv = pm + kstat * sm, pv + kstat * sv
    ok = np.all(em <= bm) and np.all(ev <= bv) and np.all(lo == NO_LO) and np.all(hi == NO_HI)
    worst = max(float((em / np.maximum(bm, 1e-300)).max()), float((ev / np.maximum(bv, 1e-300)).max()))
    excess = max(float(((em - pm) / np.maximum(sm, 1e-300)).max()), float(((ev - pv) / sv).max()), 0.0)
    return bool(ok), worst, excess


def predict_filter(x, w, name, smean):
    """FilterPredictor.forward of the frame-mode model in float64 from the tap x [H,W,512] the Filter reads and the style half
    smean [32] the GPU cached: (filter [32,32], magnitude)."""
    p = "Decoder.%s." % name
    cv, cm = conv3(x, w[p + "down_sample.0.weight"], w[p + "down_sample.0.bias"], 0, x.shape[0])
    sm = np.asarray(smean, np.float64)
    vec = np.concatenate([cv.reshape(-1, 32).mean(axis=0), sm])
    mag = np.concatenate([cm.reshape(-1, 32).mean(axis=0), np.abs(sm)])
    W, bias = np.asarray(w[p + "FC.weight"], np.float64), np.asarray(w[p + "FC.bias"], np.float64)
    return (W @ vec + bias).reshape(32, 32), (np.abs(W) @ mag + np.abs(bias)).reshape(32, 32)


def _up2(a, H, W):
    return np.repeat(np.repeat(np.asarray(a, np.float64), 2, axis=0), 2, axis=1)[:H, :W]


def frame_checks(get, w, st, smean, fam, k=None, names=None):
    """Every frame-mode stage (or `names`, of FRAME_STAGES) of one image.  get(name): the tap [H][W][C] ("frame": grey_input of
    the frame, "pre": the pre-clamp output); st: the image's parsed state set; smean [6][32]: the style half of the filter
    predictions; fam: frame_families().  Returns [(stage, family or None, passes, worst fraction of its bound, ratio)]:
    `ratio` is the family's measured figure (module docstring); family None: a composite of two kernels, no figure."""
    k = K if k is None else k
    out = []

    def want(n):
        return names is None or n in names

    def plain(name, got, v, m, f):
        ok, worst, ratio = check(got, v, m, k[f])
        out.append((name, f, ok, worst, ratio))

    def stat(name, entry, v, b):
        out.append((name, "stat") + check_stat(entry, v, b, k["stat"]))

    def forced(name, got, v, mc, mp, f):        # a tap behind pointwise_k, teacher-forced on the GPU's statistics
        err = np.abs(np.asarray(got, np.float64) - v)
        bound = U * (k[f] * mc + k["point"] * mp + np.abs(v))
        out.append((name, "point", bool(np.all(err <= bound)), float((err / np.maximum(bound, 1e-300)).max()),
                    float((err / np.maximum(U * mp, 1e-300)).max())))

    for name in FRAME_ENC:
        if not want(name):
            continue
        _, inputs, op, _ = STAGES[name]
        got, inp = get(name), [get(i) for i in inputs]
        for y0, y1 in strips(got.shape[0]):
            v, m = op(inp, w, st, y0, y1)
            plain(name, got[y0:y1], v, m, fam[name])
    if want("stat0") or want("c41"):
        p3 = get("p3")
        v, m = _enc_stage(19, ())([p3], w, st, 0, p3.shape[0])
        n0 = st["norm"][0]
        if want("stat0"):
            stat("stat0", n0, v, k[fam["c41"]] * U * m)
        if want("c41"):
            vn, mn = norm(v, m, n0)
            forced("c41", get("c41"), vn, m * n0[1], mn, fam["c41"])
    cur = ("c41", "f1", "f2")
    for f in range(3):
        if want("pred%d" % f):
            x = get(cur[f])
            for g in (1, 2):
                name = "Filter%d.F%d" % (f + 1, g)
                v, m = predict_filter(x, w, name, smean[2 * f + g - 1])
                plain("pred%d.F%d" % (f, g), st["filt"][name], v, m, "pred")
        if f < 2 and want("f%d" % (f + 1)):
            x = get(cur[f])
            v, mu, md = _composite(f)([x], w, st, 0, x.shape[0])
            err = np.abs(get("f%d" % (f + 1)).astype(np.float64) - v)
            bound = U * (k[fam["d%d" % f]] * md + k[fam["u%d" % f]] * mu + np.abs(v))
            out.append(("f%d" % (f + 1), None, bool(np.all(err <= bound)), float((err / bound).max()), 0.0))
    if want("d"):
        x = get("f2")
        plain("d", get("d"), *_down(2)([x], w, st, 0, x.shape[0]), fam["d2"])
    if want("f3"):
        x = get("f2")
        plain("f3", get("f3"), *_up(2)([get("d"), x], w, st, 0, x.shape[0]), fam["u2"])
    if want("norm1"):       # the identity entry frame_sets_init_k writes, exactly
        mean, rstd, lo, hi = st["norm"][1]
        ok = np.all(mean == 0.0) and np.all(rstd == 1.0) and np.all(lo == NO_LO) and np.all(hi == NO_HI)
        out.append(("norm1", "stat", bool(ok), 0.0 if ok else np.inf, 0.0))
    for blk, xin, xs, a, o in FRAME_BLOCKS:
        n1, n2, na, si = RES[blk]
        pre = "Decoder.%s." % blk
        if want(xs):
            x = get(xin)
            plain(xs, get(xs), *conv1(x, w[pre + "conv_shortcut.weight"], 0, x.shape[0]), fam[a])
        if want("stat:" + a) or want(a):
            x = get(xin)
            v, m = lrelu(*conv3(x, w[pre + "conv1.weight"], w[pre + "conv1.bias"], 0, 2 * x.shape[0], ups=True))
            e1 = st["norm"][n1]
            if want("stat:" + a):
                stat("stat:" + a, e1, v, k[fam[a]] * U * m)
            if want(a):
                vn, mn = norm(v, m, e1)
                forced(a, get(a), vn, m * e1[1], mn, fam[a])
            del v, m
        if want("stat2:" + o) or want("stat3:" + o) or want(o):
            at = get(a)
            H2, W2 = at.shape[:2]
            v, m = lrelu(*conv3(at, w[pre + "conv2.weight"], w[pre + "conv2.bias"], 0, H2))
            e2, ea, (s_mean, s_std) = st["norm"][n2], st["norm"][na], st["sty"][si]
            if want("stat2:" + o):
                stat("stat2:" + o, e2, v, k[fam[o]] * U * m)
            xsu = _up2(get(xs), H2, W2)
            hv = (v - e2[0]) * e2[1] + xsu                        # norm2 + the upsampled shortcut, on the GPU's statistics
            mc = m * e2[1]                                        # the convolution's magnitude through the scales
            mh = (m + np.abs(e2[0])) * e2[1] + np.abs(xsu)        # the first pointwise pass's own result
            del v, m
            if want("stat3:" + o):
                stat("stat3:" + o, ea, hv, U * (k[fam[o]] * mc + k["point"] * mh + np.abs(hv)))
            if want(o):
                sc = ea[1] * np.abs(s_std)
                vo = (hv - ea[0]) * ea[1] * s_std + s_mean
                mo = (mh + np.abs(ea[0])) * sc + np.abs(s_mean)   # the second pass's own result
                forced(o, get(o), vo, mc * sc, mh * sc + mo, fam[o])
    if want("pre"):
        o2 = get("o2")
        got = get("pre")
        for y0, y1 in strips(got.shape[0]):
            plain("pre", got[y0:y1], *_last([o2], w, st, y0, y1), fam["pre"])
    return out


def cached_c41(p3, w, st):
    """c41 of a cached relu4_1 feature in a grouped launch (transfer_device with x.feats): conv4_1 + ReLU of the caching call's p3,
    stored raw, then pointwise_k's Decoder.norm[0] of the image's OWN set, clamp((x - mean) rstd, lo, hi).  Two kernels in one, as
    COMPOSITE: (v, mc, mp) with mc the convolution's magnitude times rstd and mp the normalisation's own magnitude."""
    v, m = _enc_stage(19, ())([p3], w, st, 0, p3.shape[0])
    n0 = st["norm"][0]
    vn, mp = norm(v, m, n0)
    return vn, m * n0[1], mp


def check2(got, v, mc, mp, kc, kp):
    """|got - v| <= 2^-24 (kc mc + kp mp + |v|) element-wise: (passes, worst fraction of the bound, worst |got - v| / (2^-24 mp))."""
    err = np.abs(np.asarray(got, np.float64) - v)
    bound = U * (kc * mc + kp * mp + np.abs(v))
    return (bool(np.all(err <= bound)), float((err / np.maximum(bound, 1e-300)).max()),
            float((err / np.maximum(U * mp, 1e-300)).max()))


def blend_ref(blobs, wts):
    """blend_sets_k in float64: sum_s w[s] state_s and the same sum on absolute values (w as the float32 the kernel holds)."""
    wts = np.asarray(wts, np.float32).astype(np.float64)
    b = np.stack([np.asarray(x, np.float32).astype(np.float64) for x in blobs])
    return wts @ b, np.abs(wts) @ np.abs(b)


# ---- clamp ends on every channel ----------------------------------------------------------------------------------------------------------
# With the golden states the clamps of norm() touch 2e-4 .. 2e-3 of the values, so a kernel that stages lo / hi of the wrong channel for
# some lanes, or swaps the ends, is seen only where the few clamping channels happen to lie.  clamp_state() builds a state whose ends cut
# into every channel at every norm point; clamp_conditions() says whether they do.
CLAMP_Q = (30.0, 70.0)      # the percentiles of a channel's pre-clamp value that become lo and hi
NORM_OFF = [4 * sum(NORM_CH[:n]) for n in range(len(NORM_CH))]
# norm point -> (the taps its kernel reads, the tap it writes, the style entry of the AdaIN behind it or None)
NORM_POINTS = {0: (("p3",), "c41", None), 1: (("d", "f2"), "f3", 3)}
for _blk, _xin, _xs, _a, _o in FRAME_BLOCKS:
    NORM_POINTS[RES[_blk][0]] = ((_xin,), _a, None)
    NORM_POINTS[RES[_blk][1]] = ((_a,), None, None)           # norm2: its clamped value lives only inside conv2's epilogue
    NORM_POINTS[RES[_blk][2]] = ((_a, _xs), _o, RES[_blk][3])
ATOM = 0.5      # a channel with more than this share of its pre-clamp values on ONE value cannot have 0.2 at lo, at hi and inside


def norm_pre(n, get, w, st):
    """The pre-clamp value (v - mean) rstd at norm point n of one image in float64, [H][W][C], from the taps get(name) its kernel reads
    (NORM_POINTS) and, for the AdaIN norm of a residual block, norm2's ends in st."""
    mean, rstd = st["norm"][n][:2]
    if n == 0:
        p3 = get("p3")
        v = _enc_stage(19, ())([p3], w, st, 0, p3.shape[0])[0]
    elif n == 1:
        d = get("d")
        v = fold_up(2, d, w, st, 0, d.shape[0])[0] + np.asarray(get("f2"), np.float64)
    else:
        blk, xin, xs, a, _ = next(b for b in FRAME_BLOCKS if n in RES[b[0]][:3])
        pre = "Decoder.%s." % blk
        if n == RES[blk][0]:
            x = get(xin)
            v = lrelu(*conv3(x, w[pre + "conv1.weight"], w[pre + "conv1.bias"], 0, 2 * x.shape[0], ups=True))[0]
        else:
            t = get(a)
            v = lrelu(*conv3(t, w[pre + "conv2.weight"], w[pre + "conv2.bias"], 0, t.shape[0]))[0]
            if n == RES[blk][2]:
                v = norm(v, v, st["norm"][RES[blk][1]])[0] + _up2(get(xs), t.shape[0], t.shape[1])
    return (v - mean) * rstd


def clamp_shares(pre, lo, hi):
    """Per channel, over every pixel of every image in pre (a list of [H][W][C]), as float32 compares them: the share of pre-clamp values
    at or below lo, at or above hi, and strictly inside; which channels are not constant; the share of a channel's commonest value
    (ReLU's zeros at Decoder.norm[0]): (at_lo, at_hi, inside, live, atom)."""
    flat = np.concatenate([np.asarray(p).reshape(-1, p.shape[-1]) for p in pre]).astype(np.float32)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    at_lo, at_hi = (flat <= lo).mean(axis=0), (flat >= hi).mean(axis=0)
    inside = ((flat > lo) & (flat < hi)).mean(axis=0)
    srt = np.sort(flat, axis=0)
    run = np.ones(flat.shape[1], np.int64)
    best = run.copy()
    for r in range(1, srt.shape[0]):
        run = np.where(srt[r] == srt[r - 1], run + 1, 1)
        best = np.maximum(best, run)
    return at_lo, at_hi, inside, flat.max(axis=0) > flat.min(axis=0), best / flat.shape[0]


def clamp_conditions(shares, floor, masks=None):
    """The norm points and channels that miss the conditions: on every channel that is not constant the share at lo and the share at hi
    are at least `floor`, and so is the share strictly inside unless more than ATOM of the channel sits on one value (then lo and hi
    fall on that value whatever the percentiles).  masks: {norm point: (live, atom)} to use instead of the shares' own (the
    construction's, for shares taken from another forward of the same frames).  Returns [(norm point, channel, shares)]."""
    bad = []
    for n, (at_lo, at_hi, inside, live, atom) in sorted(shares.items()):
        if masks is not None:
            live, atom = masks[n]
        miss = live & ((at_lo < floor) | (at_hi < floor) | ((inside < floor) & (atom <= ATOM)))
        bad.extend((n, int(c), (float(at_lo[c]), float(at_hi[c]), float(inside[c]))) for c in np.nonzero(miss)[0])
    return bad


def clamp_state(weights, blob, frames):
    """The float64 stages free-running over `frames` (uint8 [H][W][3] each) with blob's means, rstds, filters and style statistics; at each
    of the 11 norm points lo[c], hi[c] become the 30th and 70th percentile of channel c's pre-clamp value over all frames, rounded to
    float32, and the forward goes on with the values clamped so.  A channel whose pre-clamp value is constant keeps the blob's ends.
    Returns (the new blob, {norm point: clamp_shares of the construction})."""
    w = weights
    new = np.array(blob, np.float32, copy=True).reshape(-1)
    st = parse_state(new)
    shares = {}
    taps = []
    for f in frames:
        x = grey_input(f)
        for name in FRAME_ENC:
            x = STAGES[name][2]([x], w, st, 0, STAGES[name][3](*f.shape[:2])[0])[0]
        taps.append({"p3": x})

    def point(n):
        mean, rstd, lo0, hi0 = st["norm"][n]
        pre = [norm_pre(n, t.__getitem__, w, st) for t in taps]
        flat = np.concatenate([p.reshape(-1, p.shape[-1]) for p in pre])
        live = flat.max(axis=0) > flat.min(axis=0)
        lo = np.where(live, np.percentile(flat, CLAMP_Q[0], axis=0).astype(np.float32).astype(np.float64), lo0)
        hi = np.where(live, np.percentile(flat, CLAMP_Q[1], axis=0).astype(np.float32).astype(np.float64), hi0)
        C = NORM_CH[n]
        new[NORM_OFF[n] + 2 * C:NORM_OFF[n] + 3 * C], new[NORM_OFF[n] + 3 * C:NORM_OFF[n] + 4 * C] = lo, hi
        st["norm"][n] = (mean, rstd, lo, hi)
        shares[n] = clamp_shares(pre, lo, hi)
        out, sty = NORM_POINTS[n][1:]
        for t, p in zip(taps, pre):
            v = np.minimum(hi, np.maximum(lo, p))
            if out is not None:
                t[out] = v if sty is None else v * st["sty"][sty][1] + st["sty"][sty][0]

    point(0)
    for t in taps:
        t["f1"] = _composite(0)([t["c41"]], w, st, 0, t["c41"].shape[0])[0]
        t["f2"] = _composite(1)([t["f1"]], w, st, 0, t["f1"].shape[0])[0]
        t["d"] = _down(2)([t["f2"]], w, st, 0, t["f2"].shape[0])[0]
    point(1)
    for blk, xin, xs, _, _ in FRAME_BLOCKS:
        for t in taps:
            t[xs] = conv1(t[xin], w["Decoder.%s.conv_shortcut.weight" % blk], 0, t[xin].shape[0])[0]
        for n in RES[blk][:3]:
            point(n)
    assert sorted(shares) == list(range(len(NORM_CH)))
    assert np.array_equal(np.delete(new, _ends()), np.delete(np.asarray(blob, np.float32).reshape(-1), _ends()))      # only lo and hi moved
    return new, shares


def _ends():
    return np.concatenate([np.arange(NORM_OFF[n] + 2 * C, NORM_OFF[n] + 4 * C) for n, C in enumerate(NORM_CH)])

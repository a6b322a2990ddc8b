"""float64 numpy reference of the resampler (include/rerevst_hip.h "Scaling"), written from the header's formulas and not from the
library; it does not import the package.

One axis, S source and D destination samples: s = S / D, support = max(s, 1); output i has
    c = s (i + 0.5),  lo = max(int(c - support + 0.5), 0),  n = min(int(c + support + 0.5), S) - lo
    w_j = tri((lo + j - c + 0.5) / support) / sum_j of the same,  tri(t) = max(0, 1 - |t|)
in double.  resample() applies both axes in float64 to the float32 source pixel values; source_pixels() gives those values for each
input form through the existing conversions (yuv_in_ref, yuv16_ref, chroma_ref), float32 with one rounding per operation.
Plain module, no pytest."""
import numpy as np

import chroma_ref
import view_ref as V
import yuv16_ref
import yuv_in_ref

F = np.float32
TAPS = 16
MEAN = np.array([0.485, 0.456, 0.406], F)      # RGB order
STD = np.array([0.229, 0.224, 0.225], F)


def tri(t):
    return np.maximum(0.0, 1.0 - np.abs(t))


def taps(S, D):
    """(first [D] int, count [D] int, w [D][TAPS] float64, zero beyond count) of one axis"""
    s = S / D
    support = max(s, 1.0)
    first, count, w = np.zeros(D, np.int64), np.zeros(D, np.int64), np.zeros((D, TAPS))
    for i in range(D):
        c = s * (i + 0.5)
        lo = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), S) - lo
        assert 1 <= n <= TAPS, (S, D, i, n)
        wj = tri((lo + np.arange(n) - c + 0.5) / support)
        first[i], count[i], w[i, :n] = lo, n, wj / wj.sum()
    return first, count, w


def axis_matrix(S, D):
    """the [D][S] float64 matrix of one axis"""
    first, count, w = taps(S, D)
    m = np.zeros((D, S))
    for i in range(D):
        m[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
    return m


def resample(px, H, W):
    """float64 [B][H][W][C] of source values [B][SH][SW][C]"""
    px = np.asarray(px, np.float64)
    my, mx = axis_matrix(px.shape[1], H), axis_matrix(px.shape[2], W)
    return np.einsum("ys,bsxc->byxc", my, np.einsum("xs,bysc->byxc", mx, px))


def tolerance(SH, SW, H, W):
    """|got - ref| bound of a float32 evaluation: one rounding per tap and axis, the weights' own rounding and the source value's, at
    the scale of a pixel value: (n_y + n_x + 6) 2^-24 255"""
    return (taps(SH, H)[1].max() + taps(SW, W)[1].max() + 6) * 2.0 ** -24 * 255.0


# ---- the eight input forms of the first kernel: (name, view_ref layout, numpy dtype, space), YUV forms for each chroma format
FORMS = (("u8_hwc", V.LAY_HWC_BGR, np.uint8, "pixel"), ("u8_chw", V.LAY_CHW_RGB, np.uint8, "pixel"),
         ("f32_hwc", V.LAY_HWC_BGR, np.float32, "unit"), ("f32_chw", V.LAY_CHW_RGB, np.float32, "norm"),
         ("i420", V.LAY_I420, np.uint8, "pixel"), ("nv12", V.LAY_NV12, np.uint8, "pixel"),
         ("i420_16", V.LAY_I420_16, np.uint16, "pixel"), ("p016", V.LAY_P016, np.uint16, "pixel"))
YUV_LAYOUTS = (V.LAY_I420, V.LAY_NV12, V.LAY_I420_16, V.LAY_P016)
BITS = 10                                              # the handle's default depth of the uint16 layouts
_CHROMA_NAMES = {(V.LAY_I420, "420"): "i420", (V.LAY_NV12, "420"): "nv12", (V.LAY_I420_16, "420"): "i420p10", (V.LAY_P016, "420"): "p010",
                 (V.LAY_I420, "422"): "i422", (V.LAY_NV12, "422"): "nv16", (V.LAY_I420_16, "422"): "i422p10", (V.LAY_P016, "422"): "p210",
                 (V.LAY_I420, "444"): "i444", (V.LAY_NV12, "444"): "nv24", (V.LAY_I420_16, "444"): "i444p10", (V.LAY_P016, "444"): "p410"}


def planes(layout, H, W, chroma="420"):
    """[(row length, rows)] per plane: view_ref.planes with the chroma format of a YUV layout"""
    if layout not in YUV_LAYOUTS or chroma == "420":
        return V.planes(layout, H, W)
    return chroma_ref.plane_table(H, W, layout in (V.LAY_I420, V.LAY_I420_16), chroma)


def ragged(dtype, layout, H, W, chroma="420"):
    """view_ref.ragged; for a 4:2:2 / 4:4:4 layout the same rule on that format's planes (pitch = row length + 5, chroma + 3, planes
    reversed with 11-element gaps, 3 in front, frame_stride = extent + 7)"""
    if layout not in YUV_LAYOUTS or chroma == "420":
        return V.ragged(dtype, layout, H, W)
    pl = planes(layout, H, W, chroma)
    off, pitch, at = [0, 0, 0], [0, 0, 0], 3
    for k in reversed(range(len(pl))):
        ln, rows = pl[k]
        pitch[k] = ln + (3 if k > 0 else 5)
        off[k] = at
        at += (rows - 1) * pitch[k] + ln + 11
    ext = max(off[k] + (rows - 1) * pitch[k] + ln for k, (ln, rows) in enumerate(pl))
    return dict(dtype=dtype, layout=layout | chroma_ref.FLAG[chroma], frame_stride=ext + 7, plane_offset=off, pitch=pitch)


def extent(view, layout, H, W, chroma="420"):
    return max(view["plane_offset"][k] + (rows - 1) * view["pitch"][k] + ln for k, (ln, rows) in enumerate(planes(layout, H, W, chroma)))


def gather(canvas, view, layout, B, H, W, chroma="420"):
    """view_ref.gather for any chroma format: [B][frame elements], the planes of a frame one after another"""
    canvas = np.asarray(canvas).reshape(-1)
    pl = planes(layout, H, W, chroma)
    out = np.empty((B, sum(ln * rows for ln, rows in pl)), canvas.dtype)
    for b in range(B):
        at = 0
        for k, (ln, rows) in enumerate(pl):
            for r in range(rows):
                src = b * view["frame_stride"] + view["plane_offset"][k] + r * view["pitch"][k]
                out[b, at:at + ln] = canvas[src:src + ln]
                at += ln
    return out


def random_canvas(rng, layout, dtype, space, n):
    """n random elements of a canvas in an input form: bytes and codes over their whole range (the P form with random low bits), float
    values over the range of their space (pixel values in 0..255: the scale the tolerance is stated at)"""
    if dtype == np.uint8:
        return rng.integers(0, 256, n).astype(np.uint8)
    if dtype == np.uint16:
        code = rng.integers(0, 2 ** BITS, n)
        if layout == V.LAY_P016:
            code = (code << (16 - BITS)) | rng.integers(0, 2 ** (16 - BITS), n)
        return code.astype(np.uint16)
    px = rng.uniform(0.0, 255.0, n).astype(F)
    if space == "unit":
        return np.divide(px, F(255), dtype=F)
    if space == "norm":
        return np.divide(np.subtract(np.divide(px, F(255), dtype=F), F(0.45), dtype=F), F(0.225), dtype=F)
    return px


def source_pixels(frames, layout, dtype, space, B, H, W, chroma="420"):
    """float32 [B][H][W][3] BGR PIXEL values of contiguous frames [B][frame elements] in an input form: what the first kernel derives
    from each source pixel.  uint8 (float)px; float32 PIXEL v, UNIT v * 255, NORM (v * std + mean) * 255, each operation rounded to
    float32; the YUV layouts through the existing references with the BT.601 limited-range matrix (the handle's default)."""
    frames = np.asarray(frames)
    if layout in YUV_LAYOUTS:
        if chroma != "420":
            return chroma_ref.bgr_ref(frames, H, W, _CHROMA_NAMES[layout, chroma])
        if layout in (V.LAY_I420, V.LAY_NV12):
            return yuv_in_ref.bgr_ref(frames, H, W, yuv_in_ref.input_matrix64("bt601", False).astype(F), "i420" if layout == V.LAY_I420 else "nv12")
        name = "i420" if layout == V.LAY_I420_16 else "p016"
        return yuv16_ref.bgr_ref(frames, H, W, yuv16_ref.input_matrix64("bt601", False, BITS).astype(F), name, BITS)
    if layout == V.LAY_CHW_RGB:
        v = frames.reshape(B, 3, H, W).transpose(0, 2, 3, 1).astype(F)      # [B][H][W][RGB]
    else:
        v = frames.reshape(B, H, W, 3).astype(F)[..., ::-1]                 # BGR -> RGB
    if space == "unit":
        v = np.multiply(v, F(255), dtype=F)
    elif space == "norm":
        v = np.multiply(np.add(np.multiply(v, STD, dtype=F), MEAN, dtype=F), F(255), dtype=F)
    return np.ascontiguousarray(v[..., ::-1])

"""Driver-side logic of the reference's test/generate_real_video.py, restated for the
drop-in: reflect padding / cropping (ReshapeTool, :61-83, :167), the global-feature
sampling schedule (:129-148) and the frame -> rank sharding used for multi-GPU runs.
Host-side, negligible cost; numpy only.
"""
import collections

import numpy as np

from ._lib import LAY_I420, LAY_NV12, LAY_I420_16, LAY_P016, LAY_422, LAY_444, YUV_BT601, YUV_BT709     # constants only: nothing here loads the shared library


def padded_size(n):
    """ReshapeTool.process (:66-76): n+128 rounded up to a multiple of 64."""
    m = n + 128
    if m % 64 != 0:
        m += 64 - m % 64
    return m


class ReshapeTool():
    """Same behaviour as the reference class: the padded size is fixed by the first frame."""

    def __init__(self):
        self.record_H = 0
        self.record_W = 0

    def process(self, img):
        H, W, C = img.shape
        if self.record_H == 0 and self.record_W == 0:
            self.record_H, self.record_W = padded_size(H), padded_size(W)
        return reflect_pad(img, self.record_H, self.record_W)


def reflect_pad(img, PH, PW):
    """cv2.copyMakeBorder(img, 64, PH-64-H, 64, PW-64-W, cv2.BORDER_REFLECT) (:81-82).
    BORDER_REFLECT repeats the edge pixel (fedcba|abcdefgh|hgfedcb) = numpy 'symmetric'."""
    H, W = img.shape[:2]
    return np.pad(img, ((64, PH - 64 - H), (64, PW - 64 - W), (0, 0)), mode="symmetric")


def sample_indices(frame_num, interval=8):
    """Frames fed to add() (:129-143): s*interval for s < (frame_num-1)//interval, then the last."""
    return [s * interval for s in range((frame_num - 1) // interval)] + [frame_num - 1]


def sample_indices_multistyle(frame_num, interval=16):
    """VideoStylization.SeqNormPrePare ("Multi-style Interpolation/test.py":72-85): cached features
    s*interval for s < (frame_num-1)//interval + 1, then the last frame — AGAIN when it was already sampled."""
    return [s * interval for s in range((frame_num - 1) // interval + 1)] + [frame_num - 1]


def ramp_weights(i, frame_num, n_styles=2, blend="pair"):
    """Per-frame style weights of the multi-style driver loop (test.py:127-131): for two styles exactly the
    reference's [w, 1-w] with w = i/(frame_num-1).  The reference only ever ramps TWO styles; for more this build chains
    the same ramp through the styles in reverse order (the reference ramps from style 1 towards style 0): the video
    starts on the last style and ends on style 0.  blend="pair": two neighbouring styles at a time (piecewise linear);
    blend="all": a smooth partition of unity (normalised Gaussian bumps of width 1.5 styles around the same position),
    so EVERY style has a non-zero weight in every frame — what bench.py's 4-style configuration uses.  Weights sum to 1."""
    w = i / (frame_num - 1.0) if frame_num > 1 else 1.0
    if n_styles == 1:
        return [1.0]
    if n_styles == 2:
        return [w, 1.0 - w]
    pos = (1.0 - w) * (n_styles - 1)           # 0 -> style 0, n_styles-1 -> the last style
    if blend == "all":
        b = [float(np.exp(-((pos - k) / 1.5) ** 2)) for k in range(n_styles)]
        t = sum(b)
        return [v / t for v in b]
    lo = min(int(pos), n_styles - 2)
    f = pos - lo
    out = [0.0] * n_styles
    out[lo], out[lo + 1] = 1.0 - f, f
    return out


def resize_bilinear(img, size):
    """cv2.resize(img, (w, h)) with the default INTER_LINEAR geometry (half-pixel centres, edge clamp) used for the
    style images (test.py:53: 384x384).  cv2 evaluates it in 11-bit fixed point, so single grey levels may differ."""
    w, h = size
    H, W = img.shape[:2]
    ys = np.clip((np.arange(h) + 0.5) * (H / h) - 0.5, 0, H - 1)
    xs = np.clip((np.arange(w) + 0.5) * (W / w) - 0.5, 0, W - 1)
    y0, x0 = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    f = img.astype(np.float64)
    top = f[y0][:, x0] * (1 - fx) + f[y0][:, x1] * fx
    bot = f[y1][:, x0] * (1 - fx) + f[y1][:, x1] * fx
    return np.clip(np.rint(top * (1 - fy) + bot * fy), 0, 255).astype(np.uint8)


def guided_upsample(stylized, source_lo, source_hi, radius=4, eps=1e-3):
    """What guided delivery computes (transfer_frames(.., out_size="source", guide="source"); include/rerevst_hip.h "Guided delivery"), in
    float64 numpy: the stylized working frame [H][W][3] upsampled to the size of source_hi [DH][DW][3] along the edges of the source's
    luma, source_lo [H][W][3] being the source at the working size.  All BGR in 0..255; radius in working pixels, eps in the units of a
    0..1 image.  Returns float64 [DH][DW][3], not clamped.  (Fast guided filter, He & Sun 2015: fit stylized = a * luma + b in every
    window, average and upsample a and b, apply them to the full-resolution luma.)"""
    P, lo, hi = (np.asarray(v, np.float64) for v in (stylized, source_lo, source_hi))
    H, W = P.shape[:2]
    DH, DW = hi.shape[:2]
    if lo.shape[:2] != (H, W) or DH < H or DW < W or DH > 8 * H or DW > 8 * W or not 1 <= int(radius) <= 16 or not eps > 0:
        raise ValueError("guided_upsample: source_lo has the stylized frame's size, source_hi 1..8 times it per axis, radius is 1..16, eps > 0")
    r, e = int(radius), eps * 65025.0
    k = [float(np.float32(c)) for c in (0.114, 0.587, 0.299)]

    def luma(x):
        return (k[0] * x[..., 0] + k[1] * x[..., 1]) + k[2] * x[..., 2]

    def box_mean(f):      # the mean over [y - r, y + r] x [x - r, x + r] clipped to the frame
        c = np.pad(np.cumsum(np.cumsum(f, 0), 1), [(1, 0), (1, 0)] + [(0, 0)] * (f.ndim - 2))
        y0, y1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r, H - 1) + 1
        x0, x1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r, W - 1) + 1
        s = c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]
        n = ((y1 - y0)[:, None] * (x1 - x0)[None, :]).astype(np.float64)
        return s / (n[..., None] if f.ndim == 3 else n)

    def up(f):            # half-pixel bilinear with edge clamp, the tables of rrv_resample_taps for an upscale
        for axis, S, D in ((1, W, DW), (0, H, DH)):
            c = np.clip((np.arange(D) + 0.5) * (S / D) - 0.5, 0, S - 1)
            i0 = np.floor(c).astype(np.int64)
            i1, t = np.minimum(i0 + 1, S - 1), (c - i0).reshape([-1 if a == axis else 1 for a in range(f.ndim)])
            f = np.take(f, i0, axis) * (1 - t) + np.take(f, i1, axis) * t
        return f
    g = luma(lo)
    mg, mP = box_mean(g), box_mean(P)
    a = (box_mean(g[..., None] * P) - mg[..., None] * mP) / (box_mean(g * g) - mg * mg + e)[..., None]
    b = mP - a * mg[..., None]
    return up(box_mean(a)) * luma(hi)[..., None] + up(box_mean(b))


def composite(stylized, source, strength=None, matte=None, keep=None):
    """What compositing computes (transfer_frames(.., strength=, matte=, keep=); include/rerevst_hip.h "Compositing"), restated in numpy
    with every operation on float32 arrays, so the GPU result equals it bit for bit.  stylized and source: [B][H][W][3] or [H][W][3], BGR
    in 0..255, of one size.  strength: None (1), a number or one per frame, in 0..1.  matte: None, or [B or 1][H][W] ([H][W]) float32 in
    0..1 or uint8 in 0..255.  keep: None, "colour" / "color" (the source's colours, the stylized luminance) or "luma" (the reverse).
    Returns float32 of the inputs' shape, not clamped."""
    P, S = np.asarray(stylized, np.float32), np.asarray(source, np.float32)
    if P.shape != S.shape or P.ndim not in (3, 4) or P.shape[-1] != 3:
        raise ValueError("composite: stylized and source are [B][H][W][3] or [H][W][3] arrays of one shape")
    if keep not in (None, "colour", "color", "luma"):
        raise ValueError("composite: keep must be None, 'colour' ('color') or 'luma', got %r" % (keep,))
    batched = P.ndim == 4
    if not batched:
        P, S = P[None], S[None]
    B, H, W = P.shape[:3]
    f = np.float32
    alpha = np.broadcast_to(np.asarray(1.0 if strength is None else strength, f).reshape(-1), (B,)).reshape(B, 1, 1)
    if not np.all((alpha >= 0) & (alpha <= 1)):
        raise ValueError("composite: strength must lie in 0..1")
    if matte is not None:
        m = np.asarray(matte)
        m = m[None] if m.ndim == 2 else m
        if m.dtype not in (np.float32, np.uint8) or m.ndim != 3 or m.shape[0] not in (1, B) or m.shape[1:] != (H, W):
            raise ValueError("composite: matte is float32 or uint8 [B or 1][H][W] at the frames' size")
        alpha = alpha * (m if m.dtype == np.float32 else m.astype(f) / f(255.0))

    def luma(v):
        return (f(0.114) * v[..., 0] + f(0.587) * v[..., 1]) + f(0.299) * v[..., 2]

    if keep is None:
        C = P
    elif keep == "luma":
        C = P + (luma(S) - luma(P))[..., None]
    else:
        C = S + (luma(P) - luma(S))[..., None]
    alpha = np.broadcast_to(alpha, (B, H, W))[..., None].astype(f)
    out = (f(1.0) - alpha) * S + alpha * C
    assert out.dtype == np.float32
    return out if batched else out[0]


# ===== the YUV formats by name: the one table framework.py and the drivers read =====
# layout: RRV_LAY_* of include/rerevst_hip.h; bits: the code depth; dtype: of a sample (uint16 above 8 bits); planar: [Y][Cb][Cr], else [Y][CbCr];
# chroma: "420" (a chroma sample per 2 x 2 block), "422" (per horizontal pixel pair) or "444" (per pixel).
# "i420pNN" / "i422pNN" / "i444pNN": planar, the code in the low bits (ffmpeg yuv420pNNle .., Y4M C420pNN ..); "p0NN" / "p2NN" / "p4NN":
# semi-planar, the code in the high bits (ffmpeg p0NNle / p2NNle / p4NNle, hardware decoders / encoders and capture cards).
YuvFormat = collections.namedtuple("YuvFormat", "layout bits dtype planar chroma")
CHROMA_FLAGS = {"420": 0, "422": LAY_422, "444": LAY_444}
CHROMA_SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}      # (sx, sy): chroma sample (y >> sy, x >> sx)
YUV_FORMATS = {name: YuvFormat(layout | CHROMA_FLAGS[chroma], bits, np.dtype(np.uint8 if bits == 8 else np.uint16), planar, chroma)
               for name, layout, bits, planar, chroma in (
    ("i420", LAY_I420, 8, True, "420"), ("nv12", LAY_NV12, 8, False, "420"),
    ("i420p10", LAY_I420_16, 10, True, "420"), ("i420p12", LAY_I420_16, 12, True, "420"), ("i420p16", LAY_I420_16, 16, True, "420"),
    ("p010", LAY_P016, 10, False, "420"), ("p012", LAY_P016, 12, False, "420"), ("p016", LAY_P016, 16, False, "420"),
    ("i422", LAY_I420, 8, True, "422"), ("nv16", LAY_NV12, 8, False, "422"),
    ("i422p10", LAY_I420_16, 10, True, "422"), ("i422p12", LAY_I420_16, 12, True, "422"), ("i422p16", LAY_I420_16, 16, True, "422"),
    ("p210", LAY_P016, 10, False, "422"), ("p212", LAY_P016, 12, False, "422"), ("p216", LAY_P016, 16, False, "422"),
    ("i444", LAY_I420, 8, True, "444"), ("nv24", LAY_NV12, 8, False, "444"),
    ("i444p10", LAY_I420_16, 10, True, "444"), ("i444p12", LAY_I420_16, 12, True, "444"), ("i444p16", LAY_I420_16, 16, True, "444"),
    ("p410", LAY_P016, 10, False, "444"), ("p412", LAY_P016, 12, False, "444"), ("p416", LAY_P016, 16, False, "444"))}
YUV_FORMAT_NAMES = ("'i420', 'nv12', 'i420p10' / 'p12' / 'p16' or 'p010' / 'p012' / 'p016' (4:2:2: 'i422', 'nv16', 'i422pNN', 'p210' / 'p212' / 'p216'; "
                    "4:4:4: 'i444', 'nv24', 'i444pNN', 'p410' / 'p412' / 'p416')")      # as the refusals list them
YUV_STANDARDS = {"bt601": (YUV_BT601, 0.299, 0.114), "bt709": (YUV_BT709, 0.2126, 0.0722)}      # (RRV_YUV_*, Kr, Kb); Kg = 1 - Kr - Kb
YUV_DEPTHS = (8, 10, 12, 16)


def _yuv_depth(bits):
    if bits not in YUV_DEPTHS:
        raise ValueError("bits must be 8, 10, 12 or 16, got %r" % (bits,))
    return int(bits)


def yuv_matrix(standard="bt601", full_range=False, bits=8):
    """rrv_yuv_matrix[_depth] on the host: float32 [3][4], rows Y, Cb, Cr, columns the coefficients of R, G, B and an offset.  Full range:
    Y = Kr R + Kg G + Kb B, Cb = 128 + (B - Y) / (2 (1 - Kb)), Cr = 128 + (R - Y) / (2 (1 - Kr)); limited range: Y' = 16 + 219/255 Y
    and the chroma differences times 224/255.  bits = 10, 12, 16: d-bit codes — the limited matrix times 2^(d-8); full range
    (2^d - 1)/255 in place of 1 and 2^(d-1) in place of 128.  Evaluated in double, each coefficient rounded once to float32."""
    d = _yuv_depth(bits)
    _, kr, kb = YUV_STANDARDS[standard]
    k = np.array([kr, 1.0 - kr - kb, kb], np.float64)
    s, top = float(1 << (d - 8)), float((1 << d) - 1)
    ys, cs = (top / 255.0, top / 255.0) if full_range else (219.0 / 255.0 * s, 224.0 / 255.0 * s)
    m = np.zeros((3, 4), np.float64)
    m[0, :3] = ys * k
    m[1, :3] = cs * (np.array([0.0, 0.0, 1.0]) - k) / (2.0 * (1.0 - kb))
    m[2, :3] = cs * (np.array([1.0, 0.0, 0.0]) - k) / (2.0 * (1.0 - kr))
    m[:, 3] = (0.0 if full_range else 16.0 * s, 128.0 * s, 128.0 * s)
    return m.astype(np.float32)


def _chroma(chroma):
    c = str(chroma)
    if c not in CHROMA_SHIFTS:
        raise ValueError("chroma must be '420', '422' or '444', got %r" % (chroma,))
    return c


def chroma_plane_size(H, W, chroma="420"):
    """(CH, CW) of an H x W frame's chroma planes: ceil(H/2) x ceil(W/2) for "420", H x ceil(W/2) for "422", H x W for "444"."""
    sx, sy = CHROMA_SHIFTS[_chroma(chroma)]
    return (int(H) + sy) >> sy, (int(W) + sx) >> sx


def yuv_frame_bytes(H, W, bits=8, chroma="420"):
    """Bytes of one H x W frame in a planar or semi-planar YUV format: H*W luma samples and two chroma planes of CH x CW samples
    (chroma_plane_size: ceil(H/2) x ceil(W/2) for 4:2:0, H x ceil(W/2) for 4:2:2, H x W for 4:4:4); bits = 10, 12, 16: the same samples in
    uint16, twice the bytes.  yuv_frame_bytes(H, W, chroma=..) is also the SAMPLE count of a frame at any depth: the last axis of the
    arrays the YUV formats take and return."""
    CH, CW = chroma_plane_size(H, W, chroma)
    return (int(H) * int(W) + 2 * CH * CW) * (1 if _yuv_depth(bits) == 8 else 2)


def bgr_to_yuv420(img, m, layout="i420", bits=8, chroma="420"):
    """The GPU's YUV 4:2:0 conversion (include/rerevst_hip.h, the rrv_*_yuv entries) in numpy float32, for frames that come from files:
    img [..][H][W][3] BGR, float32 in 0..255 or uint8; m the twelve matrix floats; returns uint8 [..][yuv_frame_bytes(H, W)] in
    "i420" ([Y][Cb][Cr]) or "nv12" ([Y][CbCr]).  Every product and sum is a float32 operation in the kernel's order, so on the float32
    output of a transfer entry this gives the bytes of its YUV form.  bits = 10, 12, 16 (m a matrix of that depth): uint16 samples
    [..][H*W + 2*CH*CW], codes clamped to 0..2^bits - 1; "i420" keeps the code in the low bits (RRV_LAY_I420_16, yuv420p10le), "nv12" in
    the high bits (RRV_LAY_P016, p010le: code << (16 - bits)).  chroma = "422": a chroma sample per horizontal pixel pair, (l + r) * 0.5f of
    the unclamped components, a last odd column paired with itself; "444": every pixel's own components ([..][yuv_frame_bytes(H, W,
    chroma=chroma)] samples); layout still names the plane order ("i420": planar, "nv12": semi-planar)."""
    if layout not in ("i420", "nv12"):
        raise ValueError("layout must be 'i420' or 'nv12', got %r" % (layout,))
    d = _yuv_depth(bits)
    chroma = _chroma(chroma)
    f = np.asarray(img).astype(np.float32)
    m = np.asarray(m, np.float32).reshape(3, 4)
    H, W = f.shape[-3:-1]
    lead = f.shape[:-3]
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    zero, top, quarter = np.float32(0), np.float32((1 << d) - 1), np.float32(0.25)
    comp = [((m[k, 0] * r + m[k, 1] * g) + m[k, 2] * b) + m[k, 3] for k in range(3)]
    if d == 8:
        byte = lambda v: np.rint(np.minimum(np.maximum(v, zero), top)).astype(np.uint8)
    else:
        shift = np.uint16(16 - d if layout == "nv12" else 0)
        byte = lambda v: np.left_shift(np.rint(np.minimum(np.maximum(v, zero), top)).astype(np.uint16), shift)
    y0, x0 = np.arange(0, H, 2), np.arange(0, W, 2)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)          # a row / column past the frame: its nearest one inside
    planes = [byte(comp[0]).reshape(lead + (H * W,))]
    samples = []
    for c in comp[1:]:
        if chroma == "444":
            mean = c
        elif chroma == "422":
            mean = (c[..., x0] + c[..., x1]) * np.float32(0.5)
        else:
            rows0, rows1 = c[..., y0, :], c[..., y1, :]
            mean = ((rows0[..., x0] + rows0[..., x1]) + (rows1[..., x0] + rows1[..., x1])) * quarter
        samples.append(byte(mean))
    if layout == "i420":
        planes += [c.reshape(lead + (-1,)) for c in samples]
    else:
        planes.append(np.stack(samples, axis=-1).reshape(lead + (-1,)))
    return np.concatenate(planes, axis=-1)


def yuv_input_matrix(standard="bt601", full_range=False, bits=8):
    """rrv_yuv_input_matrix[_depth] on the host, the inverse of yuv_matrix's transform: float32 [3][4], rows R, G, B, columns the coefficients
    of Y, Cb, Cr and an offset.  Limited range: Y' = (Y - 16) 255/219, C' = (C - 128) 255/224 (full range: Y' = Y, C' = C - 128);
    R = Y' + 2(1-Kr) Cr', B = Y' + 2(1-Kb) Cb', G = Y' - (2 Kb (1-Kb) / Kg) Cb' - (2 Kr (1-Kr) / Kg) Cr', the offsets folded into column 3.
    bits = 10, 12, 16 (s = 2^(d-8)): limited range Y' = (Y / s - 16) 255/219, C' = (C / s - 128) 255/224; full range Y' = 255/(2^d - 1) Y,
    C' = 255/(2^d - 1) (C - 2^(d-1)).  Evaluated in double, each coefficient rounded once to float32."""
    d = _yuv_depth(bits)
    _, kr, kb = YUV_STANDARDS[standard]
    kg = 1.0 - kr - kb
    s, top = float(1 << (d - 8)), float((1 << d) - 1)
    ys, cs, y0 = (255.0 / top, 255.0 / top, 0.0) if full_range else (255.0 / 219.0 / s, 255.0 / 224.0 / s, 16.0 * s)
    c0 = 128.0 * s
    cb = (0.0, -(2.0 * kb * (1.0 - kb) / kg), 2.0 * (1.0 - kb))
    cr = (2.0 * (1.0 - kr), -(2.0 * kr * (1.0 - kr) / kg), 0.0)
    n = np.zeros((3, 4), np.float64)
    for k in range(3):
        n[k] = (ys, cs * cb[k], cs * cr[k], -(ys * y0) - c0 * (cs * cb[k]) - c0 * (cs * cr[k]))
    return n.astype(np.float32)


def yuv420_to_bgr(buf, H, W, n, layout="i420", bits=8, chroma="420"):
    """The GPU's YUV 4:2:0 input conversion (include/rerevst_hip.h, the rrv_*_from_yuv entries) in numpy float32: buf uint8
    [..][yuv_frame_bytes(H, W)] in "i420" or "nv12", n the twelve floats of the input matrix; returns float32 [..][H][W][3] BGR, the PIXEL
    frame the first kernel sees.  Pixel (y, x) takes Y[y][x] and the chroma sample (y >> 1, x >> 1); every product and sum is a
    float32 operation in the kernel's order; the value is clamped to 0..255 and not rounded.  bits = 10, 12, 16 (n a matrix of that
    depth): buf uint16 [..][H*W + 2*CH*CW]; "i420" samples are the codes, "nv12" samples carry the code in the high bits
    (sample >> (16 - bits), the low bits ignored).  chroma = "422" / "444": the chroma sample is (y, x >> 1) / (y, x), and buf has
    yuv_frame_bytes(H, W, chroma=chroma) samples."""
    if layout not in ("i420", "nv12"):
        raise ValueError("layout must be 'i420' or 'nv12', got %r" % (layout,))
    d = _yuv_depth(bits)
    chroma = _chroma(chroma)
    fs = yuv_frame_bytes(H, W, chroma=chroma)
    buf = np.asarray(buf)
    dt = np.uint8 if d == 8 else np.uint16
    if buf.dtype != dt or buf.shape[-1] != fs:
        raise ValueError("a %d x %d %s frame at %d bits is %d %s samples, got %s %s" % (H, W, layout, d, fs, np.dtype(dt).name, buf.dtype, buf.shape))
    if d != 8 and layout == "nv12":
        buf = np.right_shift(buf, np.uint16(16 - d))
    n = np.asarray(n, np.float32).reshape(3, 4)
    lead = buf.shape[:-1]
    CH, CW = chroma_plane_size(H, W, chroma)
    sx, sy = CHROMA_SHIFTS[chroma]
    y = buf[..., :H * W].reshape(lead + (H, W)).astype(np.float32)
    if layout == "i420":
        cb = buf[..., H * W:H * W + CH * CW].reshape(lead + (CH, CW))
        cr = buf[..., H * W + CH * CW:].reshape(lead + (CH, CW))
    else:
        pairs = buf[..., H * W:].reshape(lead + (CH, CW, 2))
        cb, cr = pairs[..., 0], pairs[..., 1]
    rows, cols = np.arange(H) >> sy, np.arange(W) >> sx
    cb = cb[..., rows, :][..., cols].astype(np.float32)
    cr = cr[..., rows, :][..., cols].astype(np.float32)
    zero, top = np.float32(0), np.float32(255)
    rgb = [np.minimum(np.maximum(((n[k, 0] * y + n[k, 1] * cb) + n[k, 2] * cr) + n[k, 3], zero), top) for k in range(3)]
    return np.stack(rgb[::-1], axis=-1)


# ===== shots: the signature, the distance between frames, the rule that finds the cuts, the shots file (INTEGRATION.md "Shots") =====
def shot_signature(frame):
    """The shot signature of one frame (include/rerevst_hip.h "Shots"; Stylization.shot_signatures computes it on the GPU for the frame's
    thumbnail), restated in numpy: frame [H][W][3] BGR in the PIXEL space, any real dtype, H, W >= 4 -> uint32 [16][32], a 32-bin luma
    histogram for each cell of a 4 x 4 grid.  Integers from the first step on, so the GPU equals it word for word:
    c8 = clamp(rint(v), 0, 255) per channel (half to even; NaN and everything not above 0 give 0, +inf gives 255),
    Y = (29 B8 + 150 G8 + 77 R8 + 128) >> 8, bin = Y >> 3, and pixel (y, x) lies in cell ((4 y) // H, (4 x) // W)."""
    v = np.asarray(frame, np.float32)
    if v.ndim != 3 or v.shape[2] != 3 or v.shape[0] < 4 or v.shape[1] < 4:
        raise ValueError("shot_signature: frame is [H][W][3] with H, W >= 4, got %s" % (v.shape,))
    H, W = v.shape[:2]
    with np.errstate(invalid="ignore"):
        c8 = np.where(v > 0, np.minimum(np.rint(v), np.float32(255)), np.float32(0)).astype(np.int64)
    Y = (29 * c8[..., 0] + 150 * c8[..., 1] + 77 * c8[..., 2] + 128) >> 8
    cell = ((4 * np.arange(H)) // H)[:, None] * 4 + ((4 * np.arange(W)) // W)[None, :]
    return np.bincount((cell * 32 + (Y >> 3)).ravel(), minlength=512).reshape(16, 32).astype(np.uint32)


def shot_distances(sigs, sizes=None):
    """sigs [N][16][32] (shot_signature / Stylization.shot_signatures) -> float64 D[N], D[0] = 0: D[f] is the mean over the 16 cells of
    sum_k |sig[f][c][k] - sig[f-1][c][k]| / (2 n_c), n_c the cell's pixel count (its counts' sum): 0 for equal histograms, 1 when no cell's
    histograms overlap.  sizes: optional, one (H, W) per frame; a change of frame size gives D[f] = 1 (as do signatures whose cells hold
    different pixel counts: they come from thumbnails of different sizes)."""
    s = np.asarray(sigs).astype(np.int64)
    if s.ndim != 3 or s.shape[1:] != (16, 32):
        raise ValueError("shot_distances: sigs is [N][16][32], got %s" % (s.shape,))
    N = s.shape[0]
    if sizes is not None and len(sizes) != N:
        raise ValueError("shot_distances: %d sizes for %d signatures" % (len(sizes), N))
    D = np.zeros(N, np.float64)
    if N < 2:
        return D
    n = s.sum(axis=2)                                                     # [N][16]
    if (n < 1).any():
        raise ValueError("shot_distances: a cell without pixels: not a signature")
    D[1:] = (np.abs(s[1:] - s[:-1]).sum(axis=2) / (2.0 * n[1:])).mean(axis=1)
    changed = (n[1:] != n[:-1]).any(axis=1)
    if sizes is not None:
        changed |= np.array([tuple(sizes[f]) != tuple(sizes[f - 1]) for f in range(1, N)])
    D[1:][changed] = 1.0
    return D


def size_changes(sizes):
    """the frames f >= 1 whose size differs from frame f - 1's: the cuts no rule may drop (a shot's sampled frames share one size)"""
    return [f for f in range(1, len(sizes)) if tuple(sizes[f]) != tuple(sizes[f - 1])]


def detect_cuts(D, threshold=0.35, ratio=3.0, window=8, min_len=8, forced=()):
    """The first frame of every shot, starting with 0, from the distances of shot_distances.  Scanning upwards, frame f >= 1 starts a shot when
    D[f] >= threshold, and D[f] >= ratio * median(D[g] for g in [max(1, f - window), min(N - 1, f + window)], g != f) (no such g: this
    condition holds), and f - previous_cut >= min_len.  forced: frames that start a shot whatever the rule says (size_changes: the driver
    passes them, so a size change is always a cut).
    The four defaults are design parameters that nobody has tuned on real footage: a hard cut between shots of different brightness or
    layout clears them by a wide margin, dissolves, fades and flash frames are outside what the rule sees."""
    D = np.asarray(D, np.float64)
    N = len(D)
    forced = set(int(f) for f in forced)
    cuts = [0]
    for f in range(1, N):
        if f in forced:
            cuts.append(f)
            continue
        if D[f] < threshold or f - cuts[-1] < min_len:
            continue
        near = [D[g] for g in range(max(1, f - window), min(N - 1, f + window) + 1) if g != f]
        if not near or D[f] >= ratio * float(np.median(near)):
            cuts.append(f)
    return cuts


def shots_from_cuts(cuts, n):
    """[(lo, hi)] of the shots of an n-frame video whose first frames are `cuts` (sorted, starting with 0): shot k is the frames lo .. hi - 1"""
    cuts = [int(c) for c in cuts]
    return [(c, cuts[k + 1] if k + 1 < len(cuts) else int(n)) for k, c in enumerate(cuts)]


def check_shots(shots, n):
    """a list of (lo, hi) pairs as [(int, int)]; ValueError unless they tile 0 .. n - 1 in order, none empty"""
    out = [(int(lo), int(hi)) for lo, hi in shots]
    if not out or out[0][0] != 0 or out[-1][1] != n or any(lo >= hi for lo, hi in out) or any(out[k][1] != out[k + 1][0] for k in range(len(out) - 1)):
        raise ValueError("shots must tile the frames 0..%d in order, each (lo, hi) with lo < hi, got %r" % (n - 1, out))
    return out


def write_shots(path, cuts):
    """The shots file: text, one first-frame index per line, `#` comments."""
    with open(path, "w") as f:
        f.write("# first frame of every shot, one per line\n")
        for c in cuts:
            f.write("%d\n" % int(c))


def read_shots(path, n):
    """The first-frame indices of a shots file for an n-frame video (write_shots; text, one index per line, `#` starts a comment, blank
    lines are skipped).  ValueError, in words, for a line that is no integer and for a list that is unsorted, repeated, out of range or
    missing 0."""
    cuts = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            text = line.split("#", 1)[0].strip()
            if not text:
                continue
            try:
                cuts.append(int(text))
            except ValueError:
                raise ValueError("%s, line %d: %r is not a frame index" % (path, no, text)) from None
    for a, b in zip(cuts, cuts[1:]):
        if b == a:
            raise ValueError("%s: frame %d is listed twice" % (path, a))
        if b < a:
            raise ValueError("%s: the list is not sorted (%d follows %d)" % (path, b, a))
    for c in cuts:
        if not 0 <= c < n:
            raise ValueError("%s: frame %d is out of range, the video has %d frames" % (path, c, n))
    if not cuts or cuts[0] != 0:
        raise ValueError("%s: the first shot starts at frame 0, which the list is missing" % path)
    return cuts


# ===== picture area: the line profile, the rule that finds the bars, the window as text (INTEGRATION.md "Picture area") =====
def picture_profile(frame, threshold=10):
    """The line profile of one frame (include/rerevst_hip.h "Picture area"; Stylization.picture_profiles computes it on the GPU), restated in
    numpy: frame [H][W][3] BGR in the PIXEL space, any real dtype, H, W >= 8 -> uint32 [H + W]: row_cnt[H], the lit pixels of every row,
    then col_cnt[W], of every column.  Integers from the rounding on, so the GPU equals it word for word: c8 = clamp(rint(v), 0, 255) per
    channel (half to even; NaN and everything not above 0 give 0, +inf gives 255), Y = (29 B8 + 150 G8 + 77 R8 + 128) >> 8, and a pixel is
    lit iff Y > threshold (0..254).  The default of 10 is ffmpeg cropdetect's default of 24 on limited-range codes, moved to the full-range
    values the first kernel produces; nobody has tuned it on real footage."""
    v = np.asarray(frame, np.float32)
    if v.ndim != 3 or v.shape[2] != 3 or v.shape[0] < 8 or v.shape[1] < 8:
        raise ValueError("picture_profile: frame is [H][W][3] with H, W >= 8, got %s" % (v.shape,))
    threshold = int(threshold)
    if not 0 <= threshold <= 254:
        raise ValueError("picture_profile: threshold must be in 0..254, got %d" % threshold)
    with np.errstate(invalid="ignore"):
        c8 = np.where(v > 0, np.minimum(np.rint(v), np.float32(255)), np.float32(0)).astype(np.int64)
    lit = ((29 * c8[..., 0] + 150 * c8[..., 1] + 77 * c8[..., 2] + 128) >> 8) > threshold
    return np.concatenate([lit.sum(axis=1), lit.sum(axis=0)]).astype(np.uint32)


def _centre_run(picture, gap):
    """[lo, hi) of the run of picture lines around the centre line n // 2, grown outwards past gaps of fewer than `gap` lines; None if the
    centre line is not picture"""
    n = len(picture)
    c = n // 2
    if not picture[c]:
        return None
    lo = hi = c
    miss = 0
    for i in range(c - 1, -1, -1):
        if picture[i]:
            lo, miss = i, 0
        else:
            miss += 1
            if miss >= gap:
                break
    miss = 0
    for i in range(c + 1, n):
        if picture[i]:
            hi, miss = i, 0
        else:
            miss += 1
            if miss >= gap:
                break
    return lo, hi + 1


def detect_picture(profs, H, W, line=0.02, vote=0.1, dark=0.05, gap=4, min_bar=4, min_keep=0.5):
    """The active picture area (y0, x0, h, w) of H x W frames from their line profiles profs [N][H + W] (picture_profile /
    Stylization.picture_profiles / scan_frames): the window inside letterbox and pillarbox bars, or the whole frame (0, 0, H, W).
      1  A frame votes iff sum(row_cnt) >= dark * H * W: dark frames and fades say nothing about bars.  No voters: the whole frame.
      2  Row y is picture iff row_cnt[y] > line * W in at least max(1, ceil(vote * voters)) voting frames; column x likewise with line * H.
      3  Per axis the run of picture lines that contains the centre line n // 2 (not picture: the whole frame), grown outwards in each
         direction past gaps of fewer than `gap` non-picture lines and stopped at the first gap of `gap` lines: subtitles and logos inside
         a bar are separated from the picture by dark lines, stay in the bar and are passed through from the source.
      4  A bar thinner than min_bar lines is dropped: that side goes to the frame's edge.
      5  The low edge is rounded up to even, the high edge down to even unless it is the frame's edge (the window rule of the entries).
      6  A window that keeps less than min_keep of either axis (or fewer than 8 lines, the entries' minimum) gives the whole frame.
    The six defaults and the profile's threshold of 10 are design parameters that nobody has tuned on real footage; 10 is ffmpeg
    cropdetect's default of 24 on limited-range codes, moved to the full-range values the first kernel produces."""
    H, W = int(H), int(W)
    p = np.asarray(profs)
    if p.ndim == 1:
        p = p[None]
    if p.ndim != 2 or p.shape[1] != H + W:
        raise ValueError("detect_picture: profs is [N][H + W] = [N][%d], got %s" % (H + W, p.shape,))
    whole = (0, 0, H, W)
    p = p.astype(np.int64)
    rows, cols = p[:, :H], p[:, H:]
    voting = rows.sum(axis=1) >= dark * H * W
    voters = int(voting.sum())
    if voters == 0:
        return whole
    need = max(1, int(np.ceil(vote * voters)))
    window = []
    for cnt, n, across in ((rows[voting], H, W), (cols[voting], W, H)):
        run = _centre_run((cnt > line * across).sum(axis=0) >= need, int(gap))
        if run is None:
            return whole
        lo, hi = run
        if lo < min_bar:
            lo = 0
        if n - hi < min_bar:
            hi = n
        lo += lo & 1
        if hi != n:
            hi -= hi & 1
        if hi - lo < min_keep * n or hi - lo < 8:
            return whole
        window.append((lo, hi - lo))
    (y0, h), (x0, w) = window
    return (y0, x0, h, w)


def check_picture(picture, H, W):
    """(y0, x0, h, w) as ints; ValueError naming the field unless it is a window of an H x W frame by the rule of rrv_picture_check: y0, x0
    even and >= 0; h, w >= 8; y0 + h <= H, x0 + w <= W; h even unless y0 + h == H; w even unless x0 + w == W"""
    try:
        y0, x0, h, w = (int(v) for v in picture)
    except (TypeError, ValueError):
        raise ValueError("picture is (y0, x0, h, w), got %r" % (picture,)) from None
    for name, o, n, full in (("y0", y0, h, H), ("x0", x0, w, W)):
        size = "h" if name == "y0" else "w"
        if o < 0 or o & 1:
            raise ValueError("picture: %s must be even and at least 0, got %d" % (name, o))
        if n < 8:
            raise ValueError("picture: %s must be at least 8, got %d" % (size, n))
        if o + n > full:
            raise ValueError("picture: %s reaches beyond the frame (%s + %s = %d > %d)" % (size, name, size, o + n, full))
        if n & 1 and o + n != full:
            raise ValueError("picture: %s must be even unless the window reaches the frame's edge, got %d" % (size, n))
    return y0, x0, h, w


def format_picture(picture):
    """(y0, x0, h, w) -> "WxH+X+Y", the geometry text of ffmpeg's crop filter and of --picture"""
    y0, x0, h, w = (int(v) for v in picture)
    return "%dx%d+%d+%d" % (w, h, x0, y0)


def parse_picture(text):
    """"WxH+X+Y" -> (y0, x0, h, w); ValueError in words for anything else (the window rule is check_picture's, against a frame size)"""
    import re
    m = re.fullmatch(r"\s*(\d+)x(\d+)\+(\d+)\+(\d+)\s*", str(text))
    if not m:
        raise ValueError("picture: %r is not WxH+X+Y (for instance 1920x804+0+138)" % (text,))
    w, h, x0, y0 = (int(g) for g in m.groups())
    return y0, x0, h, w


def shard_range(frame_num, rank, world):
    """Contiguous block of frames owned by `rank`."""
    lo = frame_num * rank // world
    hi = frame_num * (rank + 1) // world
    return lo, hi


def stylize_video(model, frames, style, rank=0, world=1, broadcast=None, interval=8, chunk=32):
    """generate_real_video.py main flow on one rank of `world`.

    `frames`: list of uint8 BGR HWC arrays (the whole video; only the sampled frames and
    this rank's shard are touched).  `broadcast(blob, src)` ships the state blob from rank 0
    (an RCCL broadcast in bench.py / dist.py; None for single GPU).  Returns
    {frame index: float32 BGR HWC stylized frame cropped back to the input size}.
    """
    n = len(frames)
    use_global = getattr(model, "use_Global", True)
    if not use_global:                           # frame mode: per-frame statistics, no saved state to compute or ship
        model.prepare_style(style)
        blob = None
    elif rank == 0:
        model.prepare_style(style)
        model.clean()
        for i in sample_indices(n, interval):
            model.add(frames[i])                 # unpadded, as the reference does
        model.compute()
        blob = model.get_state()
    else:
        blob = None
    if world > 1 and use_global:
        blob = broadcast(blob, 0)
        if rank != 0:
            model.set_state(blob)
    tool = ReshapeTool()
    lo, hi = shard_range(n, rank, world)
    out = {}
    on_device = getattr(model, "transfer_frames", None)     # pad / crop inside the first / last kernel
    same = all(f.shape == frames[lo].shape for f in frames[lo:hi]) if hi > lo else False
    if on_device is not None and same:
        for c0 in range(lo, hi, chunk):
            idx = list(range(c0, min(hi, c0 + chunk)))
            styled = on_device([frames[i] for i in idx])
            for j, i in enumerate(idx):
                out[i] = styled[j]
        return out
    # the host-buffer batch entry pipelines sub-batches (copy in / kernels / copy out) inside one call
    batch = getattr(model, "transfer_batch", None)     # a model with only the reference's per-frame transfer() works too
    if batch is None:
        batch = lambda fs: np.stack([model.transfer(f) for f in fs])
    for c0 in range(lo, hi, chunk):
        idx = list(range(c0, min(hi, c0 + chunk)))
        styled = batch([tool.process(frames[i]) for i in idx])
        for j, i in enumerate(idx):
            H, W, _ = frames[i].shape
            out[i] = styled[j, 64:64 + H, 64:64 + W, :]
    return out


def stylize_video_multistyle(model, frames, styles, weights_of=None, interval=16, style_size=(384, 384)):
    """"Multi-style Interpolation/test.py" main flow (VideoStylization :40-111 + the driver loop :114-131) on a model
    with the multi-style call surface (MultiStyleStylization, or the oracle's MultiStylization):
    styles resized to 384x384 (:53) -> prepare_style; every frame padded (ChangeShapeTool) and encoded ONCE, the
    feature cached (:87-101; in HBM here, on disk in the reference); every `interval`-th cached feature plus the last
    one again -> add_patch -> compute_norm (:72-85); then per frame the decoder alone with the blended state of
    weight vector weights_of(i, n) (default: the reference's ramp) and the crop (:110).
    Returns {frame index: float32 BGR HWC stylized frame}."""
    n = len(frames)
    S = len(styles)
    if weights_of is None:
        weights_of = lambda i, num: ramp_weights(i, num, S)
    model.prepare_style([resize_bilinear(s, style_size) if style_size and tuple(s.shape[:2]) != tuple(style_size[::-1]) else s for s in styles])
    tool = ReshapeTool()
    feats = [model.generate_content_features(tool.process(f)) for f in frames]
    model.clean()
    for i in sample_indices_multistyle(n, interval):
        model.add_patch(feats[i])
    model.compute_norm()
    out = {}
    for i, f in enumerate(frames):
        H, W, _ = f.shape
        out[i] = model.transfer(feats[i], weights_of(i, n))[64:64 + H, 64:64 + W, :]
    return out

"""Reference of the YUV 4:2:2 and 4:4:4 forms, 8 to 16 bits (include/rerevst_hip.h: RRV_LAY_422 / RRV_LAY_444 on the four YUV layouts),
written from the header on its own and not shared with rerevst-code_amd/video.py: numpy float32, one ufunc per operation (numpy rounds
each to float32, so nothing is contracted into a fused multiply-add), in the order the header states.  d = bits, top = 2^d - 1.

  chroma   (sx, sy) = (1, 1) for "420", (1, 0) for "422", (0, 0) for "444"; CW = ceil(W / 2^sx), CH = ceil(H / 2^sy)
  frame    frame_samples = H*W + 2*CH*CW; planar [Y][Cb][Cr] or semi-planar [Y][CbCr interleaved: CH rows of CW pairs]
  output   c_k = ((m[k][0]*R + m[k][1]*G) + m[k][2]*B) + m[k][3]            k = Y, Cb, Cr
           Y code = rint(min(max(c_0, 0), top)), half to even; a chroma code the same of
             "420"  ((tl + tr) + (bl + br)) * 0.25f     "422"  (l + r) * 0.5f     "444"  the pixel's own c_k
           of the unclamped c_1 / c_2, a pixel outside the frame (odd last row / column) replaced by its nearest one inside
           sample = code (8 bits, and the uint16 planar forms) or code << (16 - d) (the uint16 semi-planar P forms)
  input    code = sample, or sample >> (16 - d) for the P forms; pixel (y, x) takes Y[y][x] and chroma sample (y >> sy, x >> sx)
           v_k = ((n[k][0]*Y + n[k][1]*Cb) + n[k][2]*Cr) + n[k][3]          k = R, G, B
           px_k = min(max(v_k, 0), 255)                                      not rounded to an integer
  matrices BT.601 / BT.709 as the header gives them, float64 rounded once to float32 by the callers
Plain module, no pytest."""
import numpy as np

F = np.float32
SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
FLAG = {"420": 0, "422": 0x10, "444": 0x20}
LAY_I420, LAY_NV12, LAY_I420_16, LAY_P016 = 2, 3, 8, 9
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}

# format name -> (RRV_LAY_* value, planar, chroma, bits): the sixteen new names and, for the cross-format cases, the 4:2:0 ones
FORMATS = {}
for _c in ("420", "422", "444"):
    FORMATS["i" + _c] = (LAY_I420 | FLAG[_c], True, _c, 8)
    FORMATS[{"420": "nv12", "422": "nv16", "444": "nv24"}[_c]] = (LAY_NV12 | FLAG[_c], False, _c, 8)
    for _d in (10, 12, 16):
        FORMATS["i%sp%d" % (_c, _d)] = (LAY_I420_16 | FLAG[_c], True, _c, _d)
        FORMATS["p%s%d" % ({"420": "0", "422": "2", "444": "4"}[_c], _d)] = (LAY_P016 | FLAG[_c], False, _c, _d)
# the eight new layouts by the header's names
LAYOUTS = {"RRV_LAY_I422": 18, "RRV_LAY_NV16": 19, "RRV_LAY_I422_16": 24, "RRV_LAY_P216": 25,
           "RRV_LAY_I444": 34, "RRV_LAY_NV24": 35, "RRV_LAY_I444_16": 40, "RRV_LAY_P416": 41}
NEW_FORMATS = [n for n, f in FORMATS.items() if f[2] != "420"]


def chroma_size(H, W, chroma):
    sx, sy = SHIFTS[chroma]
    return (H + sy) >> sy, (W + sx) >> sx


def frame_samples(H, W, chroma):
    CH, CW = chroma_size(H, W, chroma)
    return H * W + 2 * CH * CW


def plane_table(H, W, planar, chroma):
    """[(row length in elements, rows)] of the planes of an H x W frame"""
    CH, CW = chroma_size(H, W, chroma)
    return [(W, H), (CW, CH), (CW, CH)] if planar else [(W, H), (2 * CW, CH)]


def contiguous_view(H, W, planar, chroma):
    """(frame_stride, [plane offsets], [pitches]) of the contiguous frame, in elements"""
    CH, CW = chroma_size(H, W, chroma)
    fs = H * W + 2 * CH * CW
    if planar:
        return fs, [0, H * W, H * W + CH * CW], [W, CW, CW]
    return fs, [0, H * W], [W, 2 * CW]


def _shift(fmt):
    _, planar, _, bits = FORMATS[fmt]
    return 0 if planar or bits == 8 else 16 - bits


def matrix64(standard, full_range, bits):
    """float64 [3][4]: rows Y, Cb, Cr; columns the coefficients of R, G, B and an offset, to d-bit codes"""
    kr, kb = K[standard]
    k = [kr, 1.0 - kr - kb, kb]
    s, top = float(2 ** (bits - 8)), float(2 ** bits - 1)
    ys, cs = (top / 255.0, top / 255.0) if full_range else (219.0 / 255.0 * s, 224.0 / 255.0 * s)
    m = np.zeros((3, 4))
    for c in range(3):
        m[0, c] = ys * k[c]
        m[1, c] = cs * ((1.0 if c == 2 else 0.0) - k[c]) / (2.0 * (1.0 - kb))
        m[2, c] = cs * ((1.0 if c == 0 else 0.0) - k[c]) / (2.0 * (1.0 - kr))
    m[0, 3] = 0.0 if full_range else 16.0 * s
    m[1, 3] = m[2, 3] = 128.0 * s
    return m


def input_matrix64(standard, full_range, bits):
    """float64 [3][4]: rows R, G, B; columns the coefficients of Y, Cb, Cr and an offset, from d-bit codes (the inverse of matrix64)"""
    kr, kb = K[standard]
    kg = 1.0 - kr - kb
    s, top = float(2 ** (bits - 8)), float(2 ** bits - 1)
    ys, cs, y0 = (255.0 / top, 255.0 / top, 0.0) if full_range else (255.0 / 219.0 / s, 255.0 / 224.0 / s, 16.0 * s)
    c0 = 128.0 * s
    of_cb = [0.0, -(2.0 * kb * (1.0 - kb) / kg), 2.0 * (1.0 - kb)]
    of_cr = [2.0 * (1.0 - kr), -(2.0 * kr * (1.0 - kr) / kg), 0.0]
    n = np.zeros((3, 4))
    for k in range(3):
        n[k, 0] = ys
        n[k, 1] = cs * of_cb[k]
        n[k, 2] = cs * of_cr[k]
        n[k, 3] = -(ys * y0) - c0 * n[k, 1] - c0 * n[k, 2]
    return n


def M(fmt, standard="bt601", full_range=False):
    return matrix64(standard, full_range, FORMATS[fmt][3]).astype(F)


def N(fmt, standard="bt601", full_range=False):
    return input_matrix64(standard, full_range, FORMATS[fmt][3]).astype(F)


def _components(img, m):
    f = np.asarray(img).astype(F)
    m = np.asarray(m, dtype=F).reshape(3, 4)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    out = []
    for k in range(3):
        acc = np.add(np.multiply(m[k, 0], r, dtype=F), np.multiply(m[k, 1], g, dtype=F), dtype=F)
        acc = np.add(acc, np.multiply(m[k, 2], b, dtype=F), dtype=F)
        out.append(np.add(acc, m[k, 3], dtype=F))
    return out


def _subsample(c, chroma):
    """the unrounded chroma samples [B][CH][CW] of the component plane c [B][H][W]"""
    H, W = c.shape[1:]
    if chroma == "444":
        return c
    x0 = np.arange(0, W, 2)
    x1 = np.minimum(x0 + 1, W - 1)
    if chroma == "422":
        return np.multiply(np.add(c[:, :, x0], c[:, :, x1], dtype=F), F(0.5), dtype=F)
    y0 = np.arange(0, H, 2)
    y1 = np.minimum(y0 + 1, H - 1)
    top = np.add(c[:, y0][:, :, x0], c[:, y0][:, :, x1], dtype=F)
    bot = np.add(c[:, y1][:, :, x0], c[:, y1][:, :, x1], dtype=F)
    return np.multiply(np.add(top, bot, dtype=F), F(0.25), dtype=F)


def yuv_ref(img, fmt, m=None):
    """[B][frame_samples] samples (uint8, or uint16 above 8 bits) of float32 BGR PIXEL frames [B][H][W][3]: what an entry stores"""
    _, planar, chroma, bits = FORMATS[fmt]
    y, cb, cr = _components(img, M(fmt) if m is None else m)
    q = lambda v: np.rint(np.minimum(np.maximum(v, F(0)), F(2 ** bits - 1))).astype(np.uint32)
    B = y.shape[0]
    dt = np.uint8 if bits == 8 else np.uint16
    y, cb, cr = [(p << _shift(fmt)).astype(dt) for p in (q(y), q(_subsample(cb, chroma)), q(_subsample(cr, chroma)))]
    if planar:
        return np.concatenate([y.reshape(B, -1), cb.reshape(B, -1), cr.reshape(B, -1)], axis=1)
    return np.concatenate([y.reshape(B, -1), np.stack([cb, cr], axis=3).reshape(B, -1)], axis=1)


def planes(buf, H, W, fmt):
    """code planes (Y [B][H][W], Cb, Cr [B][CH][CW]) of samples [B][frame_samples]"""
    _, planar, chroma, bits = FORMATS[fmt]
    buf = np.asarray(buf)
    assert buf.dtype == (np.uint8 if bits == 8 else np.uint16) and buf.ndim == 2 and buf.shape[1] == frame_samples(H, W, chroma), (buf.dtype, buf.shape)
    if _shift(fmt):
        buf = buf >> np.uint16(_shift(fmt))
    B = buf.shape[0]
    CH, CW = chroma_size(H, W, chroma)
    y = buf[:, :H * W].reshape(B, H, W)
    if planar:
        return y, buf[:, H * W:H * W + CH * CW].reshape(B, CH, CW), buf[:, H * W + CH * CW:].reshape(B, CH, CW)
    c = buf[:, H * W:].reshape(B, CH, CW, 2)
    return y, c[..., 0], c[..., 1]


def bgr_ref(buf, H, W, fmt, n=None):
    """float32 [B][H][W][3] BGR PIXEL frames of YUV samples [B][frame_samples]: the frame the first kernel sees"""
    sx, sy = SHIFTS[FORMATS[fmt][2]]
    y, cb, cr = planes(buf, H, W, fmt)
    n = np.asarray(N(fmt) if n is None else n, dtype=F).reshape(3, 4)
    rows, cols = np.arange(H) >> sy, np.arange(W) >> sx
    Y = y.astype(F)
    Cb = cb[:, rows][:, :, cols].astype(F)
    Cr = cr[:, rows][:, :, cols].astype(F)
    px = []
    for k in range(3):
        acc = np.add(np.multiply(n[k, 0], Y, dtype=F), np.multiply(n[k, 1], Cb, dtype=F), dtype=F)
        acc = np.add(acc, np.multiply(n[k, 2], Cr, dtype=F), dtype=F)
        acc = np.add(acc, n[k, 3], dtype=F)
        px.append(np.minimum(np.maximum(acc, F(0)), F(255)))
    return np.ascontiguousarray(np.stack([px[2], px[1], px[0]], axis=3))


def random_samples(seed, B, H, W, fmt):
    """random codes over the whole 0..2^d - 1 range (both clamps of the input conversion fire); the P forms carry random low bits"""
    _, _, chroma, bits = FORMATS[fmt]
    rng = np.random.default_rng(seed)
    code = rng.integers(0, 2 ** bits, (B, frame_samples(H, W, chroma)), dtype=np.uint32)
    sh = _shift(fmt)
    low = rng.integers(0, 2 ** sh, code.shape, dtype=np.uint32) if sh else 0
    return ((code << sh) | low).astype(np.uint8 if bits == 8 else np.uint16)

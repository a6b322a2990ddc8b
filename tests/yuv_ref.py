"""Reference of the 8-bit YUV 4:2:0 output forms (include/rerevst_hip.h, the rrv_*_yuv entries), written on its own and not
shared with rerevst-code_amd/video.py: numpy float32, one ufunc per operation (numpy rounds each to float32, so nothing is
contracted into a fused multiply-add), in the order the header states.

    c_k = ((m[k][0]*R + m[k][1]*G) + m[k][2]*B) + m[k][3]
    Y   = rint(min(max(c_0, 0), 255))                                      one byte per pixel
    Cb  = rint(min(max(((tl + tr) + (bl + br)) * 0.25f, 0), 255)) of c_1   one byte per 2 x 2 block; Cr the same of c_2
a block pixel outside the frame (odd height / width) = its nearest block pixel inside.  Plain module, no pytest."""
import numpy as np

F = np.float32


def frame_bytes(H, W):
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def components(frames, m):
    """float32 [3][B][H][W]: the unrounded, unclamped c_0, c_1, c_2 of float32 BGR frames [B][H][W][3]."""
    f = np.ascontiguousarray(frames)
    assert f.dtype == np.float32 and f.ndim == 4 and f.shape[3] == 3, (f.dtype, f.shape)
    m = np.asarray(m, dtype=F).reshape(3, 4)
    R, G, B = f[..., 2], f[..., 1], f[..., 0]
    out = []
    for k in range(3):
        acc = np.add(np.multiply(m[k, 0], R, dtype=F), np.multiply(m[k, 1], G, dtype=F), dtype=F)
        acc = np.add(acc, np.multiply(m[k, 2], B, dtype=F), dtype=F)
        out.append(np.add(acc, m[k, 3], dtype=F))
    return np.stack(out)


def to_byte(v):
    assert v.dtype == np.float32
    return np.rint(np.minimum(np.maximum(v, F(0)), F(255))).astype(np.uint8)


def subsample(c):
    """float32 [B][CH][CW]: the 2 x 2 means of [B][H][W], an odd last row / column replicated"""
    B, H, W = c.shape
    p = np.pad(c, ((0, 0), (0, H % 2), (0, W % 2)), mode="edge")
    tl, tr, bl, br = p[:, 0::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 0::2], p[:, 1::2, 1::2]
    return np.multiply(np.add(np.add(tl, tr, dtype=F), np.add(bl, br, dtype=F), dtype=F), F(0.25), dtype=F)


def yuv_ref(frames, m, layout="i420"):
    """uint8 [B][frame_bytes(H, W)] in "i420" ([Y][Cb][Cr]) or "nv12" ([Y][Cb Cr interleaved]) of float32 BGR frames [B][H][W][3]."""
    assert layout in ("i420", "nv12")
    c = components(frames, m)
    B = c.shape[1]
    y = to_byte(c[0]).reshape(B, -1)
    cb, cr = to_byte(subsample(c[1])), to_byte(subsample(c[2]))
    if layout == "i420":
        return np.concatenate([y, cb.reshape(B, -1), cr.reshape(B, -1)], axis=1)
    return np.concatenate([y, np.stack([cb, cr], axis=3).reshape(B, -1)], axis=1)


def matrix64(standard, full_range):
    """The float64 [3][4] matrix of a standard ("bt601" | "bt709") and range, from the formulas."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[standard]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    y = [kr, kg, kb]
    m = np.zeros((3, 4))
    for c in range(3):
        m[0, c] = ys * y[c]
        m[1, c] = cs * ((1.0 if c == 2 else 0.0) - y[c]) / (2.0 * (1.0 - kb))
        m[2, c] = cs * ((1.0 if c == 0 else 0.0) - y[c]) / (2.0 * (1.0 - kr))
    m[:, 3] = [0.0 if full_range else 16.0, 128.0, 128.0]
    return m


def yuv_ref64(frames, m64):
    """The same quantities in float64 (no rounding until the byte): (Y [B][H][W], Cb, Cr [B][CH][CW]) BEFORE clamp and rint."""
    f = np.asarray(frames, np.float64)
    rgb1 = np.concatenate([f[..., ::-1], np.ones(f.shape[:3] + (1,))], axis=3)
    c = np.einsum("kc,bhwc->kbhw", np.asarray(m64, np.float64), rgb1)
    B, H, W = c.shape[1:]
    p = np.pad(c, ((0, 0), (0, 0), (0, H % 2), (0, W % 2)), mode="edge")
    mean = (p[:, :, 0::2, 0::2] + p[:, :, 0::2, 1::2] + p[:, :, 1::2, 0::2] + p[:, :, 1::2, 1::2]) / 4.0
    return c[0], mean[1], mean[2]

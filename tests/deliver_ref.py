"""Reference of the delivery stage (include/rerevst_hip.h "Scaling, output size"), written from the header and not from the library;
it does not import the package.

The working frames are float32 [B][H][W][3] BGR PIXEL values.  The resampled value v of the DH x DW frame is the input resampler's
(resample_ref.resample: the rrv_resample_taps tables of (H -> DH) and (W -> DW), rows first, then columns), here in float64.  From v
    float32 PIXEL   v                                   float32 UNIT   v / 255
    float32 NORM    (v / 255 - mean_c) / std_c          the normalised delivered pixel, c the RGB channel
    uint8           rint(min(max(v, 0), 255)), half to even
    YUV             chroma_ref.yuv_ref of the delivered float32 PIXEL frame (the last kernel's store, word for word)
The float forms are compared with the float64 value within a derived tolerance; the integer forms bit for bit with the reference
conversion of the float32 PIXEL frame the same kernel family delivers (which the float test ties to the float64 value).

Tolerances, t = resample_ref.tolerance(H, W, DH, DW) the bound of the float32 resampler at the scale of a pixel value:
    PIXEL   t
    UNIT    t / 255 + 2^-24                              one rounding of the division, the result at most 1
    NORM    (t / 255 + 2^-23) / 0.224 + 2^-23            one rounding each for the division, the subtraction (both below 1, together
                                                         2^-23), and the division by std (the smallest is 0.224; the result is below 4)
Plain module, no pytest."""
import numpy as np

import chroma_ref
import resample_ref as R

F = np.float32
MEAN = np.array([0.485, 0.456, 0.406])      # RGB order
STD = np.array([0.229, 0.224, 0.225])
SPACES = ("pixel", "unit", "norm")
# working -> delivered: odd delivered size (chroma ceil and edge replication); ratio 8 up; downscale with many taps; several tiles with a
# ragged last one; identity
SHAPES = (((16, 24), (37, 53)), ((16, 24), (128, 192)), ((72, 96), (33, 47)), ((40, 200), (50, 300)), ((64, 72), (64, 72)))


def tolerance(space, H, W, DH, DW):
    t = R.tolerance(H, W, DH, DW)
    if space == "pixel":
        return t
    if space == "unit":
        return t / 255.0 + 2.0 ** -24
    if space == "norm":
        return (t / 255.0 + 2.0 ** -23) / 0.224 + 2.0 ** -23
    raise ValueError(space)


def float_ref(px, DH, DW, space="pixel", chw=False):
    """float64 delivered frames of float32 BGR PIXEL working frames [B][H][W][3]: [B][DH][DW][3] BGR, or (chw) [B][3][DH][DW] RGB"""
    v = R.resample(np.asarray(px, F), DH, DW)[..., ::-1]      # RGB
    if space == "unit":
        v = v / 255.0
    elif space == "norm":
        v = (v / 255.0 - MEAN) / STD
    elif space != "pixel":
        raise ValueError(space)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2) if chw else v[..., ::-1])


def to_uint8(img):
    """rint(min(max(v, 0), 255)), half to even: driver.to_uint8"""
    return np.clip(np.rint(np.asarray(img, F)), 0, 255).astype(np.uint8)


def u8_ref(img, chw=False):
    """uint8 frames of delivered float32 BGR PIXEL frames [B][DH][DW][3]: HWC BGR, or (chw) [B][3][DH][DW] RGB"""
    q = to_uint8(img)
    return np.ascontiguousarray(q[..., ::-1].transpose(0, 3, 1, 2)) if chw else q


def yuv_ref(img, fmt):
    """[B][frame samples] of delivered float32 BGR PIXEL frames in the YUV format `fmt` (a chroma_ref.FORMATS name), BT.601 limited range"""
    return chroma_ref.yuv_ref(np.asarray(img, F), fmt)

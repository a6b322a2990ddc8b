"""numpy reference of strided image views (include/rerevst_hip.h rrv_image_view), written from the header's plane table; it does not
import the package.

A view is a dict(dtype, layout, frame_stride, plane_offset[3], pitch[3]); every stride is in ELEMENTS of the frame's dtype.  Frame b of
a 1-D canvas starts at b * frame_stride, row r of plane k at plane_offset[k] + r * pitch[k] from there.

  layout          planes (row length in elements x rows)
  HWC_BGR (0)     one: 3W x H
  CHW_RGB (1)     R, G, B: W x H each
  I420 (2, 8)     Y: W x H; Cb, Cr: CW x CH each
  NV12 (3, 9)     Y: W x H; CbCr interleaved: 2 CW x CH            CH = (H+1)//2, CW = (W+1)//2

gather(canvas, view, B, H, W) returns the B frames the view addresses in the contiguous form the other entries take ([B][frame
elements], frame b's planes one after another with no gaps); scatter(frames, view, canvas) writes such frames through the view into a
copy of the canvas and touches nothing else.
"""
import numpy as np

DT_U8, DT_F32, DT_U16 = 0, 1, 2
LAY_HWC_BGR, LAY_CHW_RGB, LAY_I420, LAY_NV12, LAY_I420_16, LAY_P016 = 0, 1, 2, 3, 8, 9
NP_DTYPES = {DT_U8: np.uint8, DT_F32: np.float32, DT_U16: np.uint16}
LAYOUTS = (LAY_HWC_BGR, LAY_CHW_RGB, LAY_I420, LAY_NV12, LAY_I420_16, LAY_P016)


def planes(layout, H, W):
    """[(row length, rows)] per plane"""
    CH, CW = (H + 1) // 2, (W + 1) // 2
    if layout == LAY_HWC_BGR:
        return [(3 * W, H)]
    if layout == LAY_CHW_RGB:
        return [(W, H)] * 3
    if layout in (LAY_I420, LAY_I420_16):
        return [(W, H), (CW, CH), (CW, CH)]
    if layout in (LAY_NV12, LAY_P016):
        return [(W, H), (2 * CW, CH)]
    raise ValueError(layout)


def frame_elems(layout, H, W):
    return sum(ln * rows for ln, rows in planes(layout, H, W))


def contiguous(dtype, layout, H, W):
    """the strides of the contiguous form: planes packed in order, rows packed, frames packed"""
    off, pitch, at = [0, 0, 0], [0, 0, 0], 0
    for k, (ln, rows) in enumerate(planes(layout, H, W)):
        off[k], pitch[k] = at, ln
        at += ln * rows
    return dict(dtype=dtype, layout=layout, frame_stride=at, plane_offset=off, pitch=pitch)


def extent(view, H, W):
    """one past the last element a frame addresses"""
    return max(view["plane_offset"][k] + (rows - 1) * view["pitch"][k] + ln for k, (ln, rows) in enumerate(planes(view["layout"], H, W)))


def ragged(dtype, layout, H, W, lead=3):
    """The 'ragged' view of the GPU tests: pitch = row length + 5 (chroma planes + 3), the planes in REVERSED order with 11-element gaps
    (and `lead` elements in front), frame_stride = extent + 7: everything starts misaligned."""
    pl = planes(layout, H, W)
    off, pitch, at = [0, 0, 0], [0, 0, 0], lead
    yuv = layout not in (LAY_HWC_BGR, LAY_CHW_RGB)
    for k in reversed(range(len(pl))):
        ln, rows = pl[k]
        pitch[k] = ln + (3 if yuv and k > 0 else 5)
        off[k] = at
        at += (rows - 1) * pitch[k] + ln + 11
    v = dict(dtype=dtype, layout=layout, frame_stride=0, plane_offset=off, pitch=pitch)
    v["frame_stride"] = extent(v, H, W) + 7
    return v


def canvas_elems(view, B, H, W):
    return (B - 1) * view["frame_stride"] + extent(view, H, W)


def _rows(view, b, H, W):
    """(canvas start, contiguous start, length) of every row of frame b"""
    at = 0
    for k, (ln, rows) in enumerate(planes(view["layout"], H, W)):
        for r in range(rows):
            yield b * view["frame_stride"] + view["plane_offset"][k] + r * view["pitch"][k], at, ln
            at += ln


def gather(canvas, view, B, H, W):
    canvas = np.asarray(canvas).reshape(-1)
    out = np.empty((B, frame_elems(view["layout"], H, W)), canvas.dtype)
    for b in range(B):
        for src, dst, ln in _rows(view, b, H, W):
            out[b, dst:dst + ln] = canvas[src:src + ln]
    return out


def scatter(frames, view, canvas):
    """frames: [B][frame elements] (any shape with B leading that flattens to it) for H x W given by view['size']"""
    H, W = view["size"]
    frames = np.asarray(frames)
    B = frames.shape[0]
    frames = frames.reshape(B, -1)
    out = np.array(canvas, copy=True).reshape(-1)
    assert frames.shape[1] == frame_elems(view["layout"], H, W) and frames.dtype == out.dtype
    for b in range(B):
        for dst, src, ln in _rows(view, b, H, W):
            out[dst:dst + ln] = frames[b, src:src + ln]
    return out


PIX, UNIT, NORM = 0, 1, 2


def check_table(H, W):
    """The accept / refuse table of rrv_image_view_check for H x W frames (odd H and W): (name, view, space, B, refused as input,
    refused as output, the field a refusal names)."""
    t = []
    CW = (W + 1) // 2

    def add(name, v, in_refused, out_refused, field=None, B=1, space=PIX, **change):
        v = dict(v, plane_offset=list(v["plane_offset"]), pitch=list(v["pitch"]))
        for key, val in change.items():
            if isinstance(val, tuple):
                v[key][val[0]] = val[1]
            else:
                v[key] = val
        t.append((name, v, space, B, in_refused, out_refused, field))

    hwc = ragged(DT_U8, LAY_HWC_BGR, H, W)
    chw = ragged(DT_F32, LAY_CHW_RGB, H, W)
    i420 = ragged(DT_U8, LAY_I420, H, W)
    nv12 = ragged(DT_U8, LAY_NV12, H, W)
    p016 = ragged(DT_U16, LAY_P016, H, W)
    for name, v in (("hwc", hwc), ("chw", chw), ("i420", i420), ("nv12", nv12), ("p016", p016)):
        add("ragged_" + name, v, False, False, B=3)
    add("pitch_exact", hwc, False, False, pitch=(0, 3 * W))
    add("pitch_one_short_hwc", hwc, True, True, "pitch[0]", pitch=(0, 3 * W - 1))
    add("pitch_one_short_chroma_nv12", nv12, True, True, "pitch[1]", pitch=(1, 2 * CW - 1))
    add("pitch_one_short_chroma_i420", i420, True, True, "pitch[2]", pitch=(2, CW - 1))
    add("negative_pitch", chw, True, True, "pitch[1]", pitch=(1, -W))
    add("negative_offset", chw, True, True, "plane_offset[2]", plane_offset=(2, -1))
    add("negative_frame_stride", hwc, True, True, "frame_stride", frame_stride=-1)
    # upper bounds: a pitch fits 31 bits, an offset and the frame stride 40 (nothing in the checks or in the kernels can wrap)
    add("pitch_2_31", hwc, True, True, "pitch[0]", pitch=(0, 2 ** 31))
    add("pitch_2_31_minus_1", hwc, False, False, pitch=(0, 2 ** 31 - 1))
    add("pitch_near_2_63", chw, True, True, "pitch[2]", pitch=(2, 2 ** 62))
    add("offset_above_2_40", chw, True, True, "plane_offset[0]", plane_offset=(0, 2 ** 40 + 1))
    add("frame_stride_above_2_40", hwc, True, True, "frame_stride", B=2, frame_stride=2 ** 40 + 1)
    add("frame_stride_2_40", hwc, False, False, B=2, frame_stride=2 ** 40)
    add("unused_entries_ignored", hwc, False, False, plane_offset=(2, -5), pitch=(1, -7))
    add("unused_third_plane_nv12", nv12, False, False, plane_offset=(2, -5), pitch=(2, -1))
    # overlaps: fine to read, refused to write
    add("grey_broadcast_chw", chw, False, True, "plane_offset", plane_offset=(1, chw["plane_offset"][0]))
    add("three_equal_planes_chw", dict(chw, plane_offset=[4, 4, 4]), False, True, "plane_offset")
    add("planes_overlap_by_one", chw, False, True, "plane_offset", plane_offset=(1, chw["plane_offset"][2] + (H - 1) * chw["pitch"][2] + W - 1))
    add("row_interleaved_i420", dict(i420, plane_offset=[0, W, W + CW], pitch=[W + 60, 2 * (W + 60), 2 * (W + 60)]), False, True, "plane_offset")
    add("yv12_swapped_offsets", dict(i420, plane_offset=[i420["plane_offset"][0], i420["plane_offset"][2], i420["plane_offset"][1]]), False, False)
    ext = extent(hwc, H, W)
    add("frame_stride_inside_last_plane_B2", hwc, False, True, "frame_stride", B=2, frame_stride=ext - 1)
    add("frame_stride_at_extent_B2", hwc, False, False, B=2, frame_stride=ext)
    add("frame_stride_zero_B1", hwc, False, False, B=1, frame_stride=0)
    add("frame_stride_zero_B2", hwc, False, True, "frame_stride", B=2, frame_stride=0)
    # descriptors
    add("u16_hwc", dict(hwc, dtype=DT_U16), True, True, "desc")
    add("u16_chw", dict(chw, dtype=DT_U16), True, True, "desc")
    add("u8_p016", dict(p016, dtype=DT_U8), True, True, "desc")
    add("f32_nv12", dict(nv12, dtype=DT_F32), True, True, "desc")
    add("u8_unit", hwc, True, True, "desc", space=UNIT)
    add("nv12_norm", nv12, True, True, "desc", space=NORM)
    add("f32_norm_chw", chw, False, False, space=NORM)
    add("layout_5", dict(hwc, layout=5), True, True, "desc")
    return t

"""Host-side mirror of the reference drop-in boundary ``Stylization``
(test/framework.py:56-118): same method names, argument meaning and return types, so a
``generate_real_video.py``-style driver runs unchanged.  All compute happens in
librerevst_hip.so on one MI355X; this class only marshals numpy buffers through the C ABI.
"""
import collections
import ctypes as C
import re

import numpy as np

from . import _lib
from .video import YUV_FORMATS, YUV_FORMAT_NAMES, YUV_STANDARDS, _yuv_depth, check_picture, chroma_plane_size, yuv_frame_bytes  # noqa: F401  (the YUV format table lives there)
from .weights import weight_table, load_checkpoint


class RRVError(RuntimeError):
    pass


def pinned_empty(shape, dtype=np.float32):
    """A numpy array in page-locked host memory (rrv_host_alloc): the host-buffer entries DMA straight from / into
    it instead of staging through the library's own pinned buffers.  Freed when the last view of it dies."""
    import weakref
    lib = _lib.load()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    ptr = C.c_void_p()
    if lib.rrv_host_alloc(max(n, 1), C.byref(ptr)) != 0:
        raise MemoryError("rrv_host_alloc(%d) failed" % n)
    buf = (C.c_char * max(n, 1)).from_address(ptr.value)
    weakref.finalize(buf, lib.rrv_host_free, ptr)
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def _u8_image(img, what):
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("%s must be uint8 HWC BGR with 3 channels, got %s %s" % (what, a.dtype, a.shape))
    return a


class _OutputPool:
    """Output arrays of the host entries come out of recycled page-locked blocks: the reference's call surface returns a
    fresh array per frame (framework.py:40-49), and a fresh pageable 5 MB array costs ~0.2 ms of page faults plus a
    staging copy per call — a tenth of a one-frame transfer().  A block goes back to the pool when the LAST array that
    views it dies (numpy collapses the base of every derived view onto the lease object below), so a recycled block is
    never visible to the caller.  Bounded: beyond `cap_bytes` of blocks handed out or parked, arrays are plain numpy."""
    cap_bytes = 2 << 30
    keep_per_size = 8

    def __init__(self):
        import threading
        self.free = {}            # nbytes -> [address]
        self.live = 0             # bytes of blocks in existence (handed out + parked)
        self.lock = threading.RLock()     # finalizers run on whichever thread drops the last reference (re-entrant: a GC pass inside empty())

    def _give_back(self, lib, addr, nbytes):
        with self.lock:
            lst = self.free.setdefault(nbytes, [])
            if len(lst) < self.keep_per_size:
                lst.append(addr)
                return
            self.live -= nbytes
        lib.rrv_host_free(C.c_void_p(addr))

    def empty(self, shape, dtype=np.float32):
        import weakref
        dt = np.dtype(dtype)
        count = int(np.prod(shape))
        nbytes = max(count * dt.itemsize, 1)
        lib = _lib.load()
        with self.lock:
            lst = self.free.get(nbytes)
            addr = lst.pop() if lst else None
            if addr is None:
                for size in sorted(self.free, reverse=True):          # over the cap: parked blocks of other sizes go first
                    while self.free[size] and self.live + nbytes > self.cap_bytes:
                        lib.rrv_host_free(C.c_void_p(self.free[size].pop()))
                        self.live -= size
                if self.live + nbytes > self.cap_bytes:
                    return np.empty(shape, dtype=dt)
                self.live += nbytes               # reserved before the allocation (released below if it fails)
        if addr is None:
            ptr = C.c_void_p()
            if lib.rrv_host_alloc(nbytes, C.byref(ptr)) != 0:
                with self.lock:
                    self.live -= nbytes
                return np.empty(shape, dtype=dt)
            addr = ptr.value
        lease = (C.c_char * nbytes).from_address(addr)
        weakref.finalize(lease, self._give_back, lib, addr, nbytes)
        return np.frombuffer(lease, dtype=dt, count=count).reshape(shape)


def _u8_frames(frames, what):
    """equally sized uint8 BGR frames (a list, or one [B][H][W][3] array) as one C-contiguous [B][H][W][3] array"""
    if isinstance(frames, np.ndarray) and frames.ndim == 4 and frames.dtype == np.uint8 and frames.shape[3] == 3:
        return np.ascontiguousarray(frames)
    return np.stack([_u8_image(f, what) for f in frames])


_outputs = _OutputPool()

_OUT_DTYPES = (np.dtype(np.float32), np.dtype(np.uint8))


def _out_u8(dtype):
    """True for uint8 output (the library's *_u8 entries), False for float32; any other dtype is refused."""
    dt = np.dtype(dtype)
    if dt not in _OUT_DTYPES:
        raise ValueError("dtype must be np.float32 or np.uint8, got %s" % dt)
    return dt == np.uint8


def _stylized_size(H, W, pad_crop=False):
    """(Ho, Wo) of a stylized H x W frame: the frame's own size in the pad / crop geometry (transfer_frames, pad_crop=True); otherwise the
    max pools floor it to multiples of 8, as in the reference"""
    return (H, W) if pad_crop else (H // 8 * 8, W // 8 * 8)


def _output(shape, dtype, out, out_format="bgr"):
    """(output array, uint8?) of a host entry; shape: [..][Ho][Wo][3], the stylized frames as BGR.  float32 BGR in 0..255 as the
    reference returns it, or uint8: the same values rounded half to even on the GPU (== driver.to_uint8 of the float output, bit for
    bit).  A given `out` selects the format by its own dtype; otherwise `dtype` does and the array comes from the page-locked pool.
    out_format a YUV format name: [..][yuv_frame_bytes(Ho, Wo, chroma=the format's)] samples of the format's dtype, whatever `dtype` says."""
    if out_format != "bgr":
        shape, odt = tuple(shape[:-3]) + (yuv_frame_bytes(shape[-3], shape[-2], chroma=YUV_FORMATS[out_format].chroma),), YUV_FORMATS[out_format].dtype
        if out is None:
            out = _outputs.empty(shape, odt)
        elif out.dtype != odt or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous %s array of shape %r" % (odt.name, shape))
        return out, odt == np.uint8
    if out is None:
        u8 = _out_u8(dtype)
        return _outputs.empty(shape, np.uint8 if u8 else np.float32), u8
    if out.dtype not in _OUT_DTYPES or out.shape != tuple(shape) or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 or uint8 array of shape %r" % (tuple(shape),))
    return out, out.dtype == np.uint8


# ===== YUV 4:2:0 input and output (the rrv_*_yuv / rrv_*_from_yuv entries; include/rerevst_hip.h states the arithmetic) =====
# The formats by name, their depths and yuv_frame_bytes: video.YUV_FORMATS (imported above).
def _yuv_torch_dtypes(fmt):
    """torch dtypes of a YUV tensor in format `fmt`, the preferred one first: torch.uint8 at 8 bits; above, torch.uint16 where this
    torch has it, and torch.int16 holding the same bits (x.view(torch.int16))"""
    import torch
    if YUV_FORMATS[fmt].bits == 8:
        return (torch.uint8,)
    return ((torch.uint16,) if hasattr(torch, "uint16") else ()) + (torch.int16,)


def yuv_planes(buf, H, W, layout="i420", bits=8):
    """Views (Y [..][H][W], Cb, Cr [..][CH][CW]) of uint8 frames [..][yuv_frame_bytes(H, W)] as transfer_batch / transfer_frames /
    transfer_tensor(out_format / out_layout = "i420" | "nv12") return them (a numpy array or a torch tensor).  Nothing is copied:
    for "nv12" the chroma views are strided (every second byte of the interleaved plane).  bits = 10, 12, 16 (or a layout name that
    carries the depth: "i420p10", "p010", ..): uint16 samples [..][yuv_frame_bytes(H, W)], the same planes; the samples are returned
    as stored ("p010": the code in the high bits).  A 4:2:2 / 4:4:4 name ("i422", "nv16", "p210", "i444p10", ..) gives chroma planes of
    chroma_plane_size(H, W, chroma): [..][H][CW] / [..][H][W]."""
    if layout not in YUV_FORMATS:
        raise ValueError("layout must be %s, got %r" % (YUV_FORMAT_NAMES, layout))
    fmt = YUV_FORMATS[layout]
    bits = _yuv_depth(bits) if fmt.bits == 8 else fmt.bits
    if getattr(buf.dtype, "itemsize", None) is not None and buf.dtype.itemsize != (1 if bits == 8 else 2):
        raise ValueError("%d-bit samples are %d bytes each, got %s" % (bits, 1 if bits == 8 else 2, buf.dtype))
    H, W = int(H), int(W)
    CH, CW = chroma_plane_size(H, W, fmt.chroma)
    if buf.shape[-1] != yuv_frame_bytes(H, W, chroma=fmt.chroma):
        raise ValueError("a %d x %d %r frame has %d samples, got %d" % (H, W, layout, yuv_frame_bytes(H, W, chroma=fmt.chroma), buf.shape[-1]))
    lead = tuple(buf.shape[:-1])
    y = buf[..., :H * W].reshape(lead + (H, W))
    if fmt.planar:
        return y, buf[..., H * W:H * W + CH * CW].reshape(lead + (CH, CW)), buf[..., H * W + CH * CW:].reshape(lead + (CH, CW))
    c = buf[..., H * W:].reshape(lead + (CH, CW, 2))
    return y, c[..., 0], c[..., 1]


def _lib_matrix(entry, standard, full_range, bits):
    if standard not in YUV_STANDARDS:
        raise ValueError("standard must be 'bt601' or 'bt709', got %r" % (standard,))
    m = np.empty((3, 4), np.float32)
    if getattr(_lib.load(), entry)(YUV_STANDARDS[standard][0], int(bool(full_range)), _yuv_depth(bits), m.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise ValueError("%s refused %r" % (entry, standard))
    return m


def yuv_matrix(standard="bt601", full_range=False, bits=8):
    """rrv_yuv_matrix[_depth]: the float32 [3][4] matrix (rows Y, Cb, Cr; columns R, G, B, offset) of a standard and range, to codes of
    `bits` bits (8, 10, 12, 16); needs no GPU."""
    return _lib_matrix("rrv_yuv_matrix_depth", standard, full_range, bits)


def yuv_input_matrix(standard="bt601", full_range=False, bits=8):
    """rrv_yuv_input_matrix[_depth]: the float32 [3][4] matrix (rows R, G, B; columns Y, Cb, Cr, offset) that reads YUV codes of `bits`
    bits (8, 10, 12, 16) of a standard and range, the inverse of yuv_matrix's transform; needs no GPU."""
    return _lib_matrix("rrv_yuv_input_matrix_depth", standard, full_range, bits)


def _yuv_size(in_format, size):
    if in_format not in YUV_FORMATS:
        raise ValueError("in_format must be 'bgr', %s, got %r" % (YUV_FORMAT_NAMES, in_format))
    if size is None or len(size) != 2:
        raise ValueError("%r frames need size=(H, W): the buffer does not carry it" % (in_format,))
    H, W = int(size[0]), int(size[1])
    if H < 8 or W < 8:
        raise ValueError("frames must be at least 8 x 8 pixels, got %d x %d" % (H, W))
    return H, W


def yuv_frames_args(frames, in_format, size):
    """Check YUV 4:2:0 input frames (transfer_batch / transfer_frames / add with in_format "i420" | "nv12", or the uint16 formats
    "i420p10" | "i420p12" | "i420p16" | "p010" | "p012" | "p016") without touching the GPU: `frames` is a uint8 (uint16) array
    [B][yuv_frame_bytes(H, W)] (or a list of [yuv_frame_bytes] arrays, or one such array) for size=(H, W).  Returns (C-contiguous
    [B][frame samples], H, W); raises ValueError for a missing size, a dtype other than the format's or a wrong sample count."""
    H, W = _yuv_size(in_format, size)
    a = np.asarray(frames) if isinstance(frames, np.ndarray) else np.stack([np.asarray(f) for f in frames])
    if a.ndim == 1:
        a = a[None]
    fb = yuv_frame_bytes(H, W, chroma=YUV_FORMATS[in_format].chroma)
    dt = YUV_FORMATS[in_format].dtype
    if a.dtype != dt or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != fb:
        raise ValueError("%r frames of %d x %d are %s [B][%d], got %s %s" % (in_format, H, W, dt.name, fb, a.dtype, a.shape))
    return np.ascontiguousarray(a), H, W


# ===== torch tensors (rrv_transfer_image_device) =====
_SPACES = {"pixel": _lib.SP_PIXEL, "unit": _lib.SP_UNIT, "norm": _lib.SP_NORM}
_LAYOUTS = {"nhwc": _lib.LAY_HWC_BGR, "nchw": _lib.LAY_CHW_RGB}     # nhwc: BGR (cv2's convention), nchw: RGB (torch's)
TENSOR_BATCH_MAX = 64        # images per rrv_transfer_image_device call; transfer_tensor splits larger batches


# what Stylization.transfer_tensor passes to the library, as tensor_io_args() works it out
# in_view / out_view: the rrv_image_view of a strided x / out that is passed as it is (None: contiguous frames)
TensorIO = collections.namedtuple("TensorIO", "x in_desc out_desc out_shape out_dtype B H W batched in_view out_view", defaults=(None, None))


def _on_device(t, what, device):
    if t.device.type != "cuda" or t.device.index != int(device):
        raise ValueError("%s must be a tensor on cuda:%d (the handle's device), got %s" % (what, int(device), t.device))


def _image_desc(dtype, sp, lay, what):
    import torch
    if lay in YUV_FORMATS and YUV_FORMATS[lay].bits > 8:      # (the caller has checked the dtype against _yuv_torch_dtypes)
        return _lib.ImageDesc(_lib.DT_U16, YUV_FORMATS[lay].layout, _SPACES[sp])
    if dtype == torch.uint8:
        if sp != "pixel":
            raise ValueError("%s: uint8 images are in the 'pixel' space (0..255), not %r" % (what, sp))
        dt = _lib.DT_U8
    elif dtype == torch.float32:
        dt = _lib.DT_F32
    else:
        raise ValueError("%s must be torch.uint8 or torch.float32, got %s" % (what, dtype))
    return _lib.ImageDesc(dt, _LAYOUTS[lay] if lay in _LAYOUTS else YUV_FORMATS[lay].layout, _SPACES[sp])


# ===== strided image views (rrv_image_view; include/rerevst_hip.h states the rules) =====
_ELEM_BYTES = {_lib.DT_U8: 1, _lib.DT_F32: 4, _lib.DT_U16: 2}


def _view_planes(layout, H, W):
    """[(row length in elements, rows)] of the planes of an H x W frame in `layout` ("nhwc", "nchw" or a YUV format name)"""
    if layout == "nhwc":
        return [(3 * W, H)]
    if layout == "nchw":
        return [(W, H)] * 3
    CH, CW = chroma_plane_size(H, W, YUV_FORMATS[layout].chroma)
    return [(W, H), (CW, CH), (CW, CH)] if YUV_FORMATS[layout].planar else [(W, H), (2 * CW, CH)]


def _make_view(desc, frame_stride, plane_offset, pitch):
    v = _lib.ImageView()
    v.desc, v.frame_stride = desc, int(frame_stride)
    for k in range(3):
        v.plane_offset[k] = int(plane_offset[k]) if k < len(plane_offset) else 0
        v.pitch[k] = int(pitch[k]) if k < len(pitch) else 0
    return v


def _contiguous_view(desc, H, W):
    v = _lib.ImageView()
    if _lib.load().rrv_image_view_contiguous(desc, int(H), int(W), C.byref(v)) != 0:
        raise ValueError("no entry takes dtype %d, layout %d, space %d" % (desc.dtype, desc.layout, desc.space))
    return v


def image_view_of(t, layout, size=None):
    """The rrv_image_view of a torch tensor [B,3,H,W] / [3,H,W] (layout "nchw") or [B,H,W,3] / [H,W,3] ("nhwc"), or None when its
    strides do not fit one: pure stride arithmetic, CPU tensors included.  "nchw" fits when stride(-1) == 1, stride(-2) >= W and the
    channel and batch strides are >= 0 (a channel stride of 0, from expand, reads a grey image as R = G = B); "nhwc" when
    stride(-1) == 1, stride(-2) == 3 and stride(-3) >= 3 W.  Strides are in elements, as the library's are.  The descriptor carries
    the layout, the tensor's dtype (uint8 / float32) and the "pixel" space; the caller sets the space.
    A YUV format name ("nv12", "i422", "p210", "i444p10", ..) with size=(H, W): t is [B, frame samples] or [frame samples] of the format's
    dtype with stride(-1) == 1 and a batch stride >= 0 (every second frame of a buffer, a frame repeated by expand); the planes lie as in
    the contiguous frame, frames t.stride(0) apart."""
    if layout in YUV_FORMATS and size is not None:
        fmt = YUV_FORMATS[layout]
        H, W = (int(v) for v in size)
        if t.dim() not in (1, 2) or t.stride(-1) != 1 or t.shape[-1] != yuv_frame_bytes(H, W, chroma=fmt.chroma) or (t.dim() == 2 and t.stride(0) < 0):
            return None
        if str(t.dtype) not in (("torch.uint8",) if fmt.bits == 8 else ("torch.uint16", "torch.int16")):
            return None
        v = _contiguous_view(_lib.ImageDesc(_lib.DT_U8 if fmt.bits == 8 else _lib.DT_U16, fmt.layout, _lib.SP_PIXEL), H, W)
        v.frame_stride = int(t.stride(0)) if t.dim() == 2 else 0
        return v
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'nchw' (RGB) or 'nhwc' (BGR), or a YUV format name with size=(H, W), got %r" % (layout,))
    if t.dim() not in (3, 4):
        return None
    st, shp = tuple(t.stride()), tuple(t.shape)
    if t.dim() == 3:
        st, shp = (0,) + st, (1,) + shp
    names = {"torch.uint8": _lib.DT_U8, "torch.float32": _lib.DT_F32}
    desc = _lib.ImageDesc(names.get(str(t.dtype), -1), _LAYOUTS[layout], _lib.SP_PIXEL)
    if layout == "nchw":
        (_, ch, H, W), (sb, sc, sh, sw) = shp, st
        if ch != 3 or sw != 1 or sh < W or sc < 0 or sb < 0:
            return None
        return _make_view(desc, sb, (0, sc, 2 * sc), (sh, sh, sh))
    (_, H, W, ch), (sb, sh, sw, sc) = shp, st
    if ch != 3 or sc != 1 or sw != 3 or sh < 3 * W or sb < 0:
        return None
    return _make_view(desc, sb, (0,), (sh,))


def _strided_view(t, layout, desc):
    """image_view_of for a tensor that is not contiguous, with the call's descriptor; None: the tensor is copied / refused as before"""
    if not hasattr(t, "stride"):
        return None
    v = image_view_of(t, layout)
    if v is not None:
        v.desc = desc
    return v


class ImageView():
    """A pitched surface in device memory: frames of `size` = (H, W) in `layout` — a YUV format name ("nv12", "p010", "i420", ..: a
    hardware decoder's or encoder's surface with a row pitch above the width, an aligned height, the chroma plane at its own offset;
    YV12 is "i420" with the two chroma offsets swapped) or "nchw" / "nhwc" — inside `storage`, a 1-D tensor of the format's dtype.
    pitch: elements from one row of a plane to the next, one number per plane or one for all; plane_offset: elements from a frame's
    start to row 0 of each plane (default: the planes follow each other, each rows x pitch long); frame_stride: elements from frame
    b to frame b + 1; frames: how many.  All in elements of storage's dtype, as torch strides are.  Raises ValueError when the last
    addressed element lies beyond storage.numel() or the library's rrv_image_view_check refuses the view (as an input; an output is
    checked again when it is used as one: its planes must not overlap).  Stylization.transfer_tensor(view, out=view2, ..) and
    add_tensor(view) take it; nothing is copied."""

    def __init__(self, storage, layout, size, pitch, plane_offset=None, frame_stride=0, frames=1):
        import torch
        if layout not in _LAYOUTS and layout not in YUV_FORMATS:
            raise ValueError("layout must be 'nchw', 'nhwc', %s, got %r" % (YUV_FORMAT_NAMES, layout))
        H, W = (int(v) for v in size)
        if H < 1 or W < 1 or int(frames) < 1:
            raise ValueError("an ImageView holds at least one frame of at least 1 x 1 pixels")
        if storage.dim() != 1 or not storage.is_contiguous():      # the view is addressed from data_ptr() in unit elements
            raise ValueError("storage must be a contiguous 1-D tensor, got shape %s, strides %s" % (tuple(storage.shape), tuple(storage.stride())))
        if layout in YUV_FORMATS:
            if storage.dtype not in _yuv_torch_dtypes(layout):
                raise ValueError("an %r surface is %s, got %s" % (layout, " or ".join(str(t) for t in _yuv_torch_dtypes(layout)), storage.dtype))
            dt = _lib.DT_U8 if YUV_FORMATS[layout].bits == 8 else _lib.DT_U16
            lay = YUV_FORMATS[layout].layout
        else:
            if storage.dtype not in (torch.uint8, torch.float32):
                raise ValueError("storage must be torch.uint8 or torch.float32, got %s" % (storage.dtype,))
            dt, lay = (_lib.DT_U8 if storage.dtype == torch.uint8 else _lib.DT_F32), _LAYOUTS[layout]
        planes = _view_planes(layout, H, W)
        pitch = [int(pitch)] * len(planes) if np.isscalar(pitch) else [int(v) for v in pitch]
        if len(pitch) != len(planes):
            raise ValueError("%r has %d planes, got %d pitches" % (layout, len(planes), len(pitch)))
        if plane_offset is None:
            plane_offset = [sum(pitch[j] * planes[j][1] for j in range(k)) for k in range(len(planes))]
        plane_offset = [int(v) for v in plane_offset]
        if len(plane_offset) != len(planes):
            raise ValueError("%r has %d planes, got %d plane offsets" % (layout, len(planes), len(plane_offset)))
        self.storage, self.layout, self.H, self.W, self.frames = storage, layout, H, W, int(frames)
        self.view = _make_view(_lib.ImageDesc(dt, lay, _lib.SP_PIXEL), frame_stride, plane_offset, pitch)
        if _lib.load().rrv_image_view_check(C.byref(self.view), self.frames, H, W, 0) != 0:
            raise ValueError("the library refuses this view of %d %d x %d %r frames: pitch %r, plane_offset %r, frame_stride %d (every "
                             "stride is >= 0 and a pitch at least a row long)" % (self.frames, H, W, layout, pitch, plane_offset, int(frame_stride)))
        end = (self.frames - 1) * int(frame_stride) + max(o + (rows - 1) * p + ln for o, p, (ln, rows) in zip(plane_offset, pitch, planes))
        if end > storage.numel():
            raise ValueError("the view addresses %d elements, storage holds %d" % (end, storage.numel()))

    def window(self, y0, x0, h, w):
        """The view of the window (y0, x0, h, w) of every frame (rrv_picture_view; include/rerevst_hip.h "Picture area"): an ImageView of
        h x w frames in the same storage, plane offsets moved, pitches and the frame stride kept.  The window follows video.check_picture's
        rule (even origin, at least 8 x 8, even sizes unless it reaches the frame's edge), so that no chroma sample straddles its edge."""
        y0, x0, h, w = check_picture((y0, x0, h, w), self.H, self.W)
        win = _lib.ImageView()
        if _lib.load().rrv_picture_view(C.byref(self.view), self.H, self.W, C.byref(_lib.Picture(y0, x0, h, w)), C.byref(win)) != 0:
            raise ValueError("the library refuses the window (%d, %d, %d, %d) of %d x %d frames" % (y0, x0, h, w, self.H, self.W))
        o = object.__new__(ImageView)
        o.storage, o.layout, o.H, o.W, o.frames, o.view = self.storage, self.layout, h, w, self.frames, win
        return o

    def with_space(self, space, what):
        """a copy of the library struct with the call's value space ('pixel' for uint8 and the YUV formats)"""
        v = _lib.ImageView.from_buffer_copy(self.view)
        if space != "pixel" and v.desc.dtype != _lib.DT_F32:
            raise ValueError("%s: %s images are in the 'pixel' space (0..255), not %r" % (what, "integer", space))
        v.desc.space = _SPACES[space]
        return v


def _check_out_layout(out_layout, out_space):
    """the output side of both tensor_io_args forms, before the input is looked at: True for an 'i420' / 'nv12' output"""
    if out_space not in _SPACES:
        raise ValueError("out_space must be one of %s, got %r" % (sorted(_SPACES), out_space))
    yuv = out_layout in YUV_FORMATS         # uint8 [B][yuv_frame_bytes] in the "pixel" space
    if out_layout not in _LAYOUTS and not yuv:
        raise ValueError("out_layout must be 'nchw' (RGB), 'nhwc' (BGR), %s, got %r" % (YUV_FORMAT_NAMES, out_layout))
    if yuv and out_space != "pixel":
        raise ValueError("an %r output is in the 'pixel' space, not %r" % (out_layout, out_space))
    return yuv


def _yuv_in_pixel_space(layout, space):
    if space != "pixel":
        raise ValueError("an %r input is in the 'pixel' space, not %r" % (layout, space))


def _check_in_names(space, layout, size, yuv=True):
    """the checks of a tensor input that do not look at the tensor: a YUV format name (where the entry reads YUV: `yuv`) with its space and
    size=(H, W), else the space and layout of an image tensor"""
    if yuv and layout in YUV_FORMATS:
        _yuv_in_pixel_space(layout, space)
        _yuv_size(layout, size)
        return
    if space not in _SPACES:
        raise ValueError("space must be one of %s, got %r" % (sorted(_SPACES), space))
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'nchw' (RGB) or 'nhwc' (BGR), got %r" % (layout,))


def _tensor_out_args(device, B, H, W, batched, out_space, out_dtype, out_layout, pad_crop, out):
    """(out_desc, out_shape, out_dtype) of B stylized H x W input frames: shared by tensor_io_args and yuv_tensor_io_args"""
    import torch
    yuv = out_layout in YUV_FORMATS
    Ho, Wo = _stylized_size(H, W, pad_crop)
    out_shape = (B, yuv_frame_bytes(Ho, Wo, chroma=YUV_FORMATS[out_layout].chroma)) if yuv else (B, 3, Ho, Wo) if out_layout == "nchw" else (B, Ho, Wo, 3)
    if not batched:
        out_shape = out_shape[1:]
    if out is not None:
        _on_device(out, "out", device)
        out_dtype = out.dtype
        if tuple(out.shape) != out_shape:
            raise ValueError("out must be a contiguous tensor of shape %s, got %s" % (out_shape, tuple(out.shape)))
    out_dtype = (_yuv_torch_dtypes(out_layout)[0] if yuv else torch.float32) if out_dtype is None else out_dtype
    if yuv and out_dtype not in _yuv_torch_dtypes(out_layout):
        raise ValueError("an %r output is %s, got %s" % (out_layout, " or ".join(str(t) for t in _yuv_torch_dtypes(out_layout)), out_dtype))
    desc = _image_desc(out_dtype, out_space, out_layout, "out")
    view = None
    if out is not None and not out.is_contiguous():      # a window of a larger canvas: written in place where its strides fit a view
        view = None if yuv else _strided_view(out, out_layout, desc)
        if view is None or _lib.load().rrv_image_view_check(C.byref(view), B, Ho, Wo, 1) != 0:
            raise ValueError("out must be a contiguous tensor of shape %s, or one whose strides fit an image view (rows of unit "
                             "element stride, planes and frames that do not overlap), got strides %s" % (out_shape, tuple(out.stride())))
    return desc, out_shape, out_dtype, view


def tensor_io_args(x, device, *, space="pixel", out_space="pixel", out_dtype=None, layout="nchw", out_layout=None,
                   pad_crop=False, out=None):
    """Check the arguments of Stylization.transfer_tensor against a handle on HIP device `device` (an ordinal) without touching the
    GPU, and work out the call (_tensor_io states the checks).  A non-contiguous `x` is made contiguous: what the entries without a
    view form (prepare_style_tensor) need.  tensor_view_io_args is the form that keeps a strided `x`."""
    return _tensor_io(x, device, False, space=space, out_space=out_space, out_dtype=out_dtype, layout=layout, out_layout=out_layout,
                      pad_crop=pad_crop, out=out)


def tensor_view_io_args(x, device, **kw):
    """tensor_io_args for the callers that pass image views on (transfer_tensor, add_tensor): a non-contiguous `x` whose strides fit a
    view (image_view_of) is returned as it is, in_view holding its strides; any other is made contiguous."""
    return _tensor_io(x, device, True, **kw)


def _tensor_io(x, device, views, *, space="pixel", out_space="pixel", out_dtype=None, layout="nchw", out_layout=None,
               pad_crop=False, out=None):
    """Check the arguments of Stylization.transfer_tensor against a handle on HIP device `device` (an ordinal) without
    touching the GPU, and work out the call: raises ValueError for a tensor that is not on that device, a channel count
    other than 3, a dtype the space does not allow (uint8 is "pixel" only; otherwise float32), an unknown space or
    layout, or an `out` of the wrong shape, dtype, device or layout.  A non-contiguous `x` is made contiguous — unless `views` is set
    (the callers that pass views on: transfer_tensor and add_tensor) and its strides fit an image view (image_view_of): it is then
    returned as it is, in_view holding its strides.  A non-contiguous `out` must fit a view the library accepts as an output
    (out_view), else ValueError."""
    _check_in_names(space, layout, None, yuv=False)
    out_layout = layout if out_layout is None else out_layout
    _check_out_layout(out_layout, out_space)
    _on_device(x, "x", device)
    in_desc = _image_desc(x.dtype, space, layout, "x")
    if x.dim() not in (3, 4):
        raise ValueError("x must be [B,3,H,W] or [3,H,W] ('nhwc': [B,H,W,3] or [H,W,3]), got shape %s" % (tuple(x.shape),))
    batched = x.dim() == 4
    shp = tuple(x.shape) if batched else (1,) + tuple(x.shape)
    B, H, W = (shp[0], shp[2], shp[3]) if layout == "nchw" else shp[:3]
    if (shp[1] if layout == "nchw" else shp[3]) != 3:
        raise ValueError("x must have 3 channels (%s), got shape %s" % (layout, tuple(x.shape)))
    if B < 1:
        raise ValueError("x holds no image")
    out_desc, out_shape, out_dtype, out_view = _tensor_out_args(device, B, H, W, batched, out_space, out_dtype, out_layout, pad_crop, out)
    in_view = None
    if not x.is_contiguous():      # a crop, a pitched or an expanded tensor goes by view, with no copy; anything else is copied
        in_view = _strided_view(x, layout, in_desc) if views else None
        if in_view is None:
            x = x.contiguous()
    return TensorIO(x=x, in_desc=in_desc, out_desc=out_desc, out_shape=out_shape, out_dtype=out_dtype, B=B, H=H, W=W,
                    batched=batched, in_view=in_view, out_view=out_view)


def yuv_tensor_io_args(x, device, layout, size, *, out_space="pixel", out_dtype=None, out_layout=None, pad_crop=False, out=None):
    """tensor_io_args for a YUV 4:2:0 input tensor (transfer_tensor(layout="i420" | "nv12" | "i420p10" | "p010" | .., size=(H, W))): x is
    a uint8 (the uint16 formats: torch.uint16, or torch.int16 holding the same bits) tensor [B][yuv_frame_bytes(H, W)] (or
    [yuv_frame_bytes]) on cuda:`device`; out_layout defaults to `layout` (YUV in, YUV out).  The
    output side is tensor_io_args'.  The result's in_desc is the RRV_LAY_* value of the input layout.  Raises ValueError as
    tensor_io_args does, and for a missing size or a wrong byte count."""
    import torch
    H, W = _yuv_size(layout, size)
    out_layout = layout if out_layout is None else out_layout
    _check_out_layout(out_layout, out_space)
    _on_device(x, "x", device)
    fb = yuv_frame_bytes(H, W, chroma=YUV_FORMATS[layout].chroma)
    if x.dtype not in _yuv_torch_dtypes(layout) or x.dim() not in (1, 2) or x.shape[-1] != fb or (x.dim() == 2 and x.shape[0] < 1):
        raise ValueError("an %r tensor of %d x %d frames is %s [B, %d] or [%d], got %s %s" % (
            layout, H, W, " or ".join(str(t) for t in _yuv_torch_dtypes(layout)), fb, fb, x.dtype, tuple(x.shape)))
    batched = x.dim() == 2
    B = x.shape[0] if batched else 1
    out_desc, out_shape, out_dtype, out_view = _tensor_out_args(device, B, H, W, batched, out_space, out_dtype, out_layout, pad_crop, out)
    return TensorIO(x=x if x.is_contiguous() else x.contiguous(), in_desc=YUV_FORMATS[layout].layout, out_desc=out_desc, out_shape=out_shape,
                    out_dtype=out_dtype, B=B, H=H, W=W, batched=batched, out_view=out_view)


# The two sides of a tensor call as Stylization._source / _target resolve them.  desc: the rrv_image_desc; view: the rrv_image_view of a
# strided side, None for packed frames; ptr: the address of frame 0; step: bytes from one frame to the next; tensor: the tensor that names
# the device; layout: the layout name ("nchw", "nhwc" or a YUV format); result: what the call returns (`out` itself, or the fresh tensor).
_Source = collections.namedtuple("_Source", "desc view ptr B H W batched tensor layout step")
_Target = collections.namedtuple("_Target", "desc view ptr result layout step")


def _whole_view(side, H, W):
    """the rrv_image_view of a side for the entries that take views: its own, or the contiguous view of packed H x W frames"""
    return side.view if side.view is not None else _contiguous_view(side.desc, H, W)


def _chunks(B, *sides, chunk=TENSOR_BATCH_MAX):
    """B frames in calls of at most `chunk`: (first frame, frames, the address of the first frame on each side = (base, step in bytes))"""
    for b0 in range(0, B, chunk):
        yield (b0, min(chunk, B - b0), *(C.c_void_p(ptr + b0 * step) for ptr, step in sides))


# ===== JPEG output (the rrv_jpeg_* entries; include/rerevst_hip.h "JPEG output" states the format) =====
def jpeg_args(quality=90, chroma="420", restart=None):
    """The rrv_jpeg of the jpeg_* keywords: quality 1..100, chroma "420" / "422" / "444" (or the number), restart the MCUs per restart
    interval (1..65535; None: the library's choice, one MCU row)"""
    try:
        q = int(quality)
        ok = q == quality and not isinstance(quality, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok or not 1 <= q <= 100:
        raise ValueError("jpeg_quality must be an integer in 1..100, got %r" % (quality,))
    if str(chroma) not in ("420", "422", "444") or isinstance(chroma, bool):
        raise ValueError("jpeg_chroma must be '420', '422' or '444', got %r" % (chroma,))
    if restart is None:
        r = 0
    else:
        try:
            r = int(restart)
            ok = r == restart and not isinstance(restart, bool)
        except (TypeError, ValueError):
            ok = False
        if not ok or not 1 <= r <= 65535:
            raise ValueError("jpeg_restart must be None or an integer in 1..65535 (MCUs per restart interval), got %r" % (restart,))
    return _lib.Jpeg(q, int(str(chroma)), r)


def _jpeg_alone(style_weights, style_masks, what):
    if style_weights is not None or style_masks is not None:
        raise ValueError("%s does not combine with style_weights / style_masks: JPEG output is for the global and the frame model" % what)


def jpeg_tables(quality):
    """(luma, chroma): the two uint16 [64] quantisation tables of a quality, natural order (rrv_jpeg_tables; no GPU)"""
    j = jpeg_args(quality)
    lu, ch = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    u16 = C.POINTER(C.c_uint16)
    if _lib.load().rrv_jpeg_tables(j.quality, lu.ctypes.data_as(u16), ch.ctypes.data_as(u16)) != 0:
        raise ValueError("rrv_jpeg_tables refused quality %r" % (quality,))
    return lu, ch


def jpeg_plan(H, W, chroma="420", restart=None):
    """dict(mcu_cols, mcu_rows, interval, blocks, header_bytes, bound) of an H x W frame (rrv_jpeg_plan, rrv_jpeg_bound; no GPU)"""
    j = jpeg_args(90, chroma, restart)
    v = [C.c_int(0) for _ in range(5)]
    n = C.c_size_t(0)
    lib = _lib.load()
    if lib.rrv_jpeg_plan(int(H), int(W), j.chroma, j.restart, *(C.byref(x) for x in v)) != 0 or lib.rrv_jpeg_bound(int(H), int(W), j.chroma, j.restart, C.byref(n)) != 0:
        raise ValueError("JPEG frames are 1..65535 pixels per side, got %r x %r" % (H, W))
    return dict(zip(("mcu_cols", "mcu_rows", "interval", "blocks", "header_bytes"), (x.value for x in v)), bound=n.value)


def jpeg_slot_bytes(H, W, chroma="420", restart=None, cap=None):
    """the slot size of a jpeg_cap= keyword: None is two bytes per pixel plus the header (never more than the bound); a number must hold the header"""
    plan = jpeg_plan(H, W, chroma, restart)
    if cap is None:
        return min(2 * int(H) * int(W) + plan["header_bytes"] + 2, plan["bound"])
    if isinstance(cap, bool) or int(cap) != cap or int(cap) < plan["header_bytes"] + 2:
        raise ValueError("jpeg_cap must be an integer of at least the header and EOI (%d bytes), got %r" % (plan["header_bytes"] + 2, cap))
    return int(cap)


def jpeg_frames(data, sizes):
    """the frames of an encode as a list of bytes: data uint8 [B][cap], sizes int32 [B] (tensors or arrays).  A frame that did not fit raises."""
    data, sizes = (np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in (data, sizes))
    short = [(b, -int(n)) for b, n in enumerate(sizes) if n < 0]
    if short:
        raise ValueError("jpeg_cap = %d bytes is too small: frame %d needs %d (frames that did not fit: %s)"
                         % (data.shape[1], short[0][0], short[0][1], [b for b, _ in short]))
    return [data[b, :int(n)].tobytes() for b, n in enumerate(sizes)]


# ===== JPEG input (rrv_jpeg_parse and the decode entries; include/rerevst_hip.h "JPEG input" states the streams taken and the arithmetic) =====
JPEG_IN_LAYOUTS = {400: "i444", 420: "i420", 422: "i422", 444: "i444"}      # the YUV layout a decoded frame has (grey: chroma planes of 128)


def _jpeg_parse(data, what="data"):
    """the rrv_jpeg_info of one stream; a stream the parser refuses raises ValueError with the library's words"""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError("%s must be bytes (one baseline JPEG stream), got %s" % (what, type(data).__name__))
    data = bytes(data)
    info, why = _lib.JpegInfo(), C.create_string_buffer(256)
    rc = _lib.load().rrv_jpeg_parse(C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(info), why, len(why))
    if rc != 0:
        raise ValueError("%s is not a JPEG stream this stage takes: %s" % (what, why.value.decode() or "rrv_jpeg_parse failed with %d" % rc))
    return info


def jpeg_info(data):
    """What rrv_jpeg_parse reads from the header of one baseline JPEG stream (no GPU): dict(H, W, chroma 400 / 420 / 422 / 444, components,
    interval (0: none), mcu_cols, mcu_rows, blocks, intervals, scan_offset, scan_bytes, q: uint8 [components][64] natural order, huff_dc,
    huff_ac: the specification each component uses, huff_given: the stream has DHT segments, huff: {"dc0", "dc1", "ac0", "ac1": (bits, vals)}).
    A stream the stage does not take raises ValueError with the reason."""
    f = _jpeg_parse(data)
    nc = f.components
    d = {k: int(getattr(f, k)) for k in ("H", "W", "chroma", "components", "interval", "mcu_cols", "mcu_rows", "blocks", "intervals", "scan_offset", "scan_bytes")}
    d["q"] = np.array([list(f.q[c]) for c in range(nc)], np.uint8)
    d["huff_dc"], d["huff_ac"] = [int(f.huff_dc[c]) for c in range(nc)], [int(f.huff_ac[c]) for c in range(nc)]
    d["huff_given"] = bool(f.huff_given)
    d["huff"] = {}
    for k, name in enumerate(("dc0", "dc1", "ac0", "ac1")):
        bits = [int(v) for v in f.huff_bits[k]]
        d["huff"][name] = (bits, [int(v) for v in f.huff_vals[k][:sum(bits)]])
    return d


def jpeg_status_words(status):
    """the words of a d_status value of the decode entries (rrv_jpeg_status_words)"""
    return _lib.load().rrv_jpeg_status_words(int(status)).decode()


def _jpeg_streams(streams):
    """a list of bytes -> (JpegInfo array, uint8 ndarray [B][cap] with frame b's bytes at the start of row b, cap)"""
    if isinstance(streams, (bytes, bytearray, memoryview)) or len(streams) < 1:
        raise ValueError("expected a non-empty list of bytes, one baseline JPEG stream per frame")
    infos = (_lib.JpegInfo * len(streams))()
    for b, s in enumerate(streams):
        infos[b] = _jpeg_parse(s, "stream %d" % b)
        if (infos[b].H, infos[b].W, infos[b].chroma) != (infos[0].H, infos[0].W, infos[0].chroma):
            raise ValueError("stream %d is %d x %d, chroma %d; stream 0 is %d x %d, chroma %d: the frames of one call share H, W and the chroma format"
                             % (b, infos[b].H, infos[b].W, infos[b].chroma, infos[0].H, infos[0].W, infos[0].chroma))
    cap = (max(len(s) for s in streams) + 15) & ~15
    host = np.zeros((len(streams), cap), np.uint8)
    for b, s in enumerate(streams):
        host[b, :len(s)] = np.frombuffer(bytes(s), np.uint8)
    return infos, host, cap


def _jpeg_statuses(status):
    """a decode call's statuses, read on the host: a corrupt frame raises ValueError naming its index and the reason"""
    st = status.cpu().numpy()
    bad = [(b, int(v)) for b, v in enumerate(st) if v != 0]
    if bad:
        raise ValueError("JPEG frame %d is corrupt: %s (frames that failed: %s)" % (bad[0][0], jpeg_status_words(bad[0][1]), [b for b, _ in bad]))


# ===== scaling (the rrv_*_scaled* entries; include/rerevst_hip.h "Scaling" states the arithmetic) =====
def _work_size(work_size):
    """(H, W) of a work_size= keyword: the size the frames are resampled to on the GPU, and the size of the delivered frame"""
    if work_size is None or len(work_size) != 2:
        raise ValueError("work_size must be (H, W), got %r" % (work_size,))
    H, W = int(work_size[0]), int(work_size[1])
    if H < 1 or W < 1:
        raise ValueError("work_size must be at least 1 x 1, got %d x %d" % (H, W))
    return H, W


def _no_styles_with_work_size(style_weights, style_masks):
    if style_weights is not None or style_masks is not None:
        raise ValueError("work_size does not combine with style_weights / style_masks yet: scale the frames with resample_tensor first")


def _out_size(out_size, source):
    """(DH, DW) of an out_size= keyword: the size the stylized working frame is resampled to on the GPU on its way out.  "source": the
    size of the frames as passed, `source` = (H, W)"""
    if isinstance(out_size, str):
        if out_size != "source":
            raise ValueError("out_size must be (H, W) or 'source', got %r" % (out_size,))
        return int(source[0]), int(source[1])
    try:
        ok = len(out_size) == 2 and all(int(v) == v for v in out_size)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("out_size must be (H, W) or 'source', got %r" % (out_size,))
    DH, DW = int(out_size[0]), int(out_size[1])
    if DH < 1 or DW < 1:
        raise ValueError("out_size must be at least 1 x 1, got %d x %d" % (DH, DW))
    return DH, DW


def _guide_args(guide, radius, eps, out_size):
    """(r, eps) of a guided call: guide names the call's own source, and the call names a delivered size"""
    if guide != "source":
        raise ValueError("guide must be 'source' (the frames as passed guide the upsampling), got %r" % (guide,))
    if out_size is None:
        raise ValueError("guide= needs out_size= (the size of the frames as passed: out_size='source')")
    return int(radius), float(eps)


def _no_styles_with_out_size(style_weights, style_masks):
    if style_weights is not None or style_masks is not None:
        raise ValueError("out_size does not combine with style_weights / style_masks yet: deliver the blended frames with deliver_tensor")


# ===== compositing (the rrv_*composite* entries; include/rerevst_hip.h "Compositing" states the arithmetic) =====
KEEP_NAMES = {None: _lib.KEEP_NONE, "colour": _lib.KEEP_COLOUR, "color": _lib.KEEP_COLOUR, "luma": _lib.KEEP_LUMA}


class CompositeArgs():
    """strength= / matte= / keep= of a call of B frames delivered at H x W, checked: `strength` a float32 [B] array, `matte` None, a
    C-contiguous ndarray or (tensors) a contiguous torch tensor on the device, [frames][H][W] float32 or uint8 with frames 1 or B, `keep`
    an RRV_KEEP_* value.  request(b0, nb) is the rrv_composite of frames b0 .. b0 + nb - 1."""

    def __init__(self, strength, matte, keep, B, H, W, tensors=False, device=None):
        if keep not in KEEP_NAMES:
            raise ValueError("keep must be None, 'colour' ('color') or 'luma', got %r" % (keep,))
        self.keep = KEEP_NAMES[keep]
        try:
            st = np.ones(B, np.float32) if strength is None else np.ascontiguousarray(np.broadcast_to(np.asarray(strength, np.float32).reshape(-1), (B,)))
        except ValueError:
            raise ValueError("strength must be one number or a sequence of %d, one per frame" % B) from None
        if not bool(np.all((st >= 0) & (st <= 1))):
            raise ValueError("strength must lie in 0..1 for every frame, got %r" % (strength,))
        self.strength, self.matte, self.frames, self.dtype, self.step = st, None, 0, _lib.DT_F32, 0
        if matte is None:
            return
        is_tensor = tensors and not isinstance(matte, np.ndarray)
        if is_tensor:
            import torch
            if not isinstance(matte, torch.Tensor):
                raise ValueError("matte must be a torch tensor on the handle's device or an ndarray, float32 or uint8")
            _on_device(matte, "matte", device)
            kinds = {torch.float32: _lib.DT_F32, torch.uint8: _lib.DT_U8}
        else:
            matte = np.asarray(matte)
            kinds = {np.dtype(np.float32): _lib.DT_F32, np.dtype(np.uint8): _lib.DT_U8}
        if matte.dtype not in kinds:
            raise ValueError("matte must be float32 or uint8, got %s" % (matte.dtype,))
        shape = tuple(matte.shape)
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3 or shape[0] not in (1, B) or shape[1:] != (H, W):
            raise ValueError("matte has shape %s, expected [%d or 1][%d][%d]: the delivered size" % (tuple(matte.shape), B, H, W))
        self.dtype, self.frames = kinds[matte.dtype], shape[0]
        self.matte = matte.reshape(shape).contiguous() if is_tensor else np.ascontiguousarray(matte.reshape(shape))
        self.step = H * W * (1 if self.dtype == _lib.DT_U8 else 4)

    def on_device(self, like):
        """the matte in HBM for the device entries: a host array is copied there on the current stream"""
        if self.matte is not None and isinstance(self.matte, np.ndarray):
            import torch
            self.matte = torch.from_numpy(self.matte).to(like.device, non_blocking=False)
        return self

    def request(self, b0, nb):
        ptr = None
        if self.matte is not None:
            base = self.matte.ctypes.data if isinstance(self.matte, np.ndarray) else self.matte.data_ptr()
            ptr = base + (0 if self.frames == 1 else b0 * self.step)
        return _lib.Composite(self.strength[b0:].ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(ptr), self.dtype, 1 if self.frames == 1 else nb, self.keep)


def _composite_args(strength, matte, keep, style_weights, style_masks, B, H, W, tensors=False, device=None):
    """None when no compositing keyword is given (the call is then what it was), else the checked CompositeArgs"""
    if strength is None and matte is None and keep is None:
        return None
    if style_weights is not None or style_masks is not None:
        raise ValueError("strength / matte / keep do not combine with style_weights / style_masks: blended and masked compositing are not offered")
    return CompositeArgs(strength, matte, keep, B, H, W, tensors, device)


def _picture_args(picture, H, W, out_size, style_weights, style_masks, jpeg):
    """The checked rrv_picture of a picture= keyword on H x W frames, and what does not combine with it: the delivered frame has the
    source's size, so out_size is implied to be "source"; the blended and masked models and the JPEG forms are not offered with a window"""
    if style_weights is not None or style_masks is not None:
        raise ValueError("picture= does not combine with style_weights / style_masks: blended and masked models are not offered with a window")
    if jpeg:
        raise ValueError('picture= does not combine with the "jpeg" input and output forms: decode or encode with the JPEG entries around the call')
    if out_size is not None and _out_size(out_size, (H, W)) != (H, W):
        raise ValueError("picture=: the delivered frame has the source's size (out_size is implied to be 'source'), got out_size=%r" % (out_size,))
    return _lib.Picture(*check_picture(picture, H, W))


def _host_in_desc(in_format):
    """rrv_image_desc of host frames as the scaled host entries take them: uint8 BGR HWC, or a YUV format by name"""
    if in_format == "bgr":
        return _lib.ImageDesc(_lib.DT_U8, _lib.LAY_HWC_BGR, _lib.SP_PIXEL)
    fmt = YUV_FORMATS[in_format]
    return _lib.ImageDesc(_lib.DT_U8 if fmt.bits == 8 else _lib.DT_U16, fmt.layout, _lib.SP_PIXEL)


def shot_plan(H, W):
    """rrv_shot_plan in Python (include/rerevst_hip.h "Shots"): the thumbnail size (th, tw) the shot signature of an H x W frame is taken
    from: f = the smallest integer in 1..8 with ceil(max(H, W) / f) <= 512, or 8 if there is none; th = ceil(H / f), tw = ceil(W / f)."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("shot_plan: H, W must be at least 1, got %d x %d" % (H, W))
    f = next((k for k in range(1, 9) if -(-max(H, W) // k) <= 512), 8)
    return -(-H // f), -(-W // f)


def _runs(keys):
    """[(first, count)] of the runs of equal consecutive keys"""
    runs = []
    for i, k in enumerate(keys):
        if runs and keys[runs[-1][0]] == k:
            runs[-1][1] += 1
        else:
            runs.append([i, 1])
    return [(a, b) for a, b in runs]


def resample_taps(S, D):
    """rrv_resample_taps: (first [D] int32, count [D] int32, weights [D][16] float32) of one axis of the resampler, S source and D
    destination samples; needs no GPU.  Raises ValueError outside the ratio limits (S / D and D / S at most 8)."""
    S, D = int(S), int(D)
    first, count, w = np.zeros(max(D, 1), np.int32), np.zeros(max(D, 1), np.int32), np.zeros((max(D, 1), 16), np.float32)
    rc = _lib.load().rrv_resample_taps(S, D, first.ctypes.data_as(C.POINTER(C.c_int)), count.ctypes.data_as(C.POINTER(C.c_int)),
                                       w.ctypes.data_as(C.POINTER(C.c_float)), 16)
    if rc != 0:
        raise ValueError("no resampling from %d to %d samples: the ratio is limited to 8 either way" % (S, D))
    return first, count, w


# the per-frame style weights of a blended call, as style_weight_args() works them out: `host` a C-contiguous float32 [B][S]
# array, or `dev` a float32 torch tensor on the handle's device ([B,S], or [S] with `broadcast` set: one vector for every frame)
StyleWeights = collections.namedtuple("StyleWeights", "host dev S broadcast")


def style_weight_args(style_weights, B, style_num, device, use_Global=True, tensors=False):
    """Check the `style_weights` of transfer_batch / transfer_frames / transfer_tensor for B frames on a handle made for
    `style_num` styles, without touching the GPU.  A host sequence or ndarray of shape [B][S] (or one [S] vector, used for
    every frame) becomes a float32 array; with tensors=True (transfer_tensor) a torch tensor is passed on as it is and must
    be float32, contiguous, [B,S] or [S], on cuda:`device`.  Raises ValueError otherwise, for S outside 1..style_num, and on
    a frame-mode handle (use_Global=False: the reference has no blended frame-mode model)."""
    if not use_Global:
        raise ValueError("style_weights need the global-feature-sharing model (use_Global=True)")
    if hasattr(style_weights, "is_contiguous") and hasattr(style_weights, "device"):        # a torch tensor
        t = style_weights
        if not tensors:
            raise ValueError("style_weights must be a host sequence or ndarray here (transfer_tensor takes device tensors)")
        if t.device.type != "cuda" or t.device.index != int(device):
            raise ValueError("a style_weights tensor must be on cuda:%d (the handle's device), got %s; pass host weights as "
                             "a list or ndarray" % (int(device), t.device))
        if str(t.dtype) != "torch.float32":
            raise ValueError("a style_weights tensor must be torch.float32, got %s" % (t.dtype,))
        shp = tuple(t.shape)
        if t.dim() not in (1, 2) or (t.dim() == 2 and shp[0] != B):
            raise ValueError("style_weights must have shape [%d, S] or [S], got %s" % (B, shp))
        if not t.is_contiguous():
            raise ValueError("a style_weights tensor must be contiguous")
        host, dev, S = None, t, shp[-1]
    else:
        host = np.asarray(style_weights, dtype=np.float32)
        if host.ndim == 1:
            host = np.broadcast_to(host, (B, host.shape[0]))
        if host.ndim != 2 or host.shape[0] != B:
            raise ValueError("style_weights must have shape [%d][S] or [S], got %s" % (B, np.shape(style_weights)))
        host, dev, S = np.ascontiguousarray(host), None, host.shape[1]
    if not 1 <= S <= min(int(style_num), _lib.MAX_STYLES):
        raise ValueError("style_weights name %d styles; this handle was made for style_num=%d" % (S, style_num))
    return StyleWeights(host=host, dev=dev, S=S, broadcast=dev is not None and dev.dim() == 1)


StyleMasks = collections.namedtuple("StyleMasks", "host dev S images")


def style_mask_args(style_masks, style_weights, B, H, W, style_num, device, use_Global=True, tensors=False):
    """Check the `style_masks` of transfer_batch / transfer_frames / transfer_tensor for B frames of H x W (the frames as the
    caller passes them) on a handle made for `style_num` styles, without touching the GPU.  A float32 ndarray [B][S][H][W]
    (one mask per frame) or [S][H][W] (one mask for every frame); with tensors=True (transfer_tensor) also a contiguous
    float32 torch tensor of those shapes on cuda:`device`, passed on as it is.  Nothing is converted or normalised: another
    dtype or shape raises ValueError, as do S outside 1..style_num, style_weights given as well, and a frame-mode handle
    (use_Global=False: the reference's frame-mode model has no blended state).  `images` is B or 1."""
    if style_weights is not None:
        raise ValueError("style_masks and style_weights are mutually exclusive (a mask constant over the frame is a weight vector)")
    if not use_Global:
        raise ValueError("style_masks need the global-feature-sharing model (use_Global=True)")
    m = style_masks
    if hasattr(m, "is_contiguous") and hasattr(m, "device"):        # a torch tensor
        if not tensors:
            raise ValueError("style_masks must be a float32 ndarray here (transfer_tensor takes device tensors)")
        if m.device.type != "cuda" or m.device.index != int(device):
            raise ValueError("a style_masks tensor must be on cuda:%d (the handle's device), got %s" % (int(device), m.device))
        if str(m.dtype) != "torch.float32":
            raise ValueError("a style_masks tensor must be torch.float32, got %s" % (m.dtype,))
        if not m.is_contiguous():
            raise ValueError("a style_masks tensor must be contiguous")
        host, dev, shp = None, m, tuple(m.shape)
    else:
        if not isinstance(m, np.ndarray):
            raise ValueError("style_masks must be a float32 ndarray (or, for transfer_tensor, a torch tensor), got %s" % type(m).__name__)
        if m.dtype != np.float32:
            raise ValueError("style_masks must be float32, got %s" % (m.dtype,))
        host, dev, shp = np.ascontiguousarray(m), None, m.shape
    if len(shp) not in (3, 4) or tuple(shp[-2:]) != (H, W) or (len(shp) == 4 and shp[0] != B):
        raise ValueError("style_masks must have shape [%d][S][%d][%d] or [S][%d][%d], got %s" % (B, H, W, H, W, tuple(shp)))
    S = shp[-3]
    if not 1 <= S <= min(int(style_num), _lib.MAX_STYLES):
        raise ValueError("style_masks name %d styles; this handle was made for style_num=%d" % (S, style_num))
    return StyleMasks(host=host, dev=dev, S=S, images=B if len(shp) == 4 else 1)


# The C entry of a transfer by (input is YUV, output is YUV) and what blends the styles: 0 nothing (one state; frame mode), 1 per-frame
# weights, 2 per-pixel masks.  A BGR output takes the entry's _u8 twin for uint8; the plain BGR entry also names the model and geometry.
_PLAIN, _BLEND, _MASK = 0, 1, 2
_HOST_ENTRIES = {
    (False, False): ("rrv_transfer{model}{geometry}", "rrv_transfer_blend_batch", "rrv_transfer_mask_batch"),
    (False, True): ("rrv_transfer_yuv", "rrv_transfer_blend_batch_yuv", "rrv_transfer_mask_batch_yuv"),
    (True, False): ("rrv_transfer_from_yuv", "rrv_transfer_blend_from_yuv", "rrv_transfer_mask_from_yuv"),
}
_HOST_ENTRIES[True, True] = _HOST_ENTRIES[True, False]      # (the output descriptor of the _from_yuv entries names the format)
_VIEW_ENTRIES = ("rrv_transfer_view_device", "rrv_transfer_view_blend_device", "rrv_transfer_view_mask_device")
_TENSOR_ENTRIES = {      # by (input is YUV): the output descriptor names every output format
    False: ("rrv_transfer_image_device", "rrv_transfer_image_blend_device", "rrv_transfer_image_mask_device"),
    True: ("rrv_transfer_from_yuv_device", "rrv_transfer_blend_from_yuv_device", "rrv_transfer_mask_from_yuv_device"),
}


class Stylization():
    """``Stylization(checkpoint, cuda=True, use_Global=True)`` (test/framework.py:57).

    `checkpoint` is a path to the reference ``.pth`` state_dict, or a ``{key: ndarray}``
    dict with the same keys (used with the seeded synthetic weights, since the released
    checkpoint is download-only).  `device` picks the HIP device ordinal (one process per
    GPU; defaults to LOCAL_RANK or 0).
    """

    # the transfer entries take dtype=np.uint8 / a uint8 `out`: the float32 output rounded half to even on the GPU
    # (include/rerevst_hip.h, the rrv_*_u8 entries); driver.stylize_files* ask for it
    uint8_output = True
    # transfer_batch / transfer_frames take out_format="i420" | "nv12" (the rrv_*_yuv entries): driver.stylize_files asks for it when
    # it writes only a .y4m video
    yuv_output = True
    # transfer_batch / transfer_frames take out_format="jpeg" (rrv_transfer_jpeg): driver.stylize_files asks for it with gpu_jpeg=
    jpeg_output = True
    # transfer_batch / transfer_frames / add take in_format="jpeg" (rrv_transfer_from_jpeg, rrv_add_from_jpeg): driver.stylize_files asks for it with gpu_decode=
    jpeg_input = True
    # transfer_batch / transfer_frames / add take in_format="i420" | "nv12" with size=(H, W) (the rrv_*_from_yuv entries): driver.stylize_y4m
    # feeds a .y4m input that way
    yuv_input = True
    # shot_signatures(frames, in_format=, size=) computes the signatures a cut detector compares (the rrv_shot_signature entries):
    # driver.stylize_files / stylize_y4m ask for it with shots="auto"
    shot_detection = True
    # picture_profiles / scan_frames compute the line profiles video.detect_picture reads, and picture=(y0, x0, h, w) on add, add_tensor,
    # transfer_batch, transfer_frames and transfer_tensor stylizes inside that window of the frame (the rrv_*picture* entries):
    # driver.stylize_files / stylize_y4m ask for both with picture="auto"
    picture_detection = True

    def __init__(self, checkpoint, cuda=True, use_Global=True, device=None, style_num=1):
        if not cuda:
            raise RRVError("this implementation only runs on an MI355X GPU (cuda=False has no CPU fallback)")
        self.use_Global = bool(use_Global)   # False: per-frame statistics model of test/style_network_frame.py
        self._lib = _lib.load()
        if device is None:
            import os
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = int(device)
        self.style_num = int(style_num)
        self._open = {}           # ticket id -> output array of an open transfer_async(): the GPU (or the retiring host copy)
                                  # writes into it until the ticket is collected or retired, whatever the caller keeps
        self._h = C.c_void_p()
        rc = self._lib.rrv_create(self.device, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise RRVError("rrv_create(device=%d) failed with %d (no HIP device?)" % (self.device, rc))
        weights = checkpoint if isinstance(checkpoint, dict) else load_checkpoint(checkpoint)
        for key, shape in weight_table().items():     # strict: every key, exact shape
            if key not in weights:
                raise KeyError("missing weight %s" % key)
            w = np.ascontiguousarray(weights[key], dtype=np.float32)
            if tuple(w.shape) != tuple(shape):
                raise ValueError("weight %s has shape %s, expected %s" % (key, w.shape, shape))
            shp = (C.c_int64 * w.ndim)(*w.shape)
            self._chk(self._lib.rrv_load_weight(self._h, key.encode(), w.ctypes.data_as(C.c_void_p), shp, w.ndim))
        self._chk(self._lib.rrv_finalize_weights(self._h))

    # ------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            msg = self._lib.rrv_last_error(self._h)
            err = RRVError("librerevst_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
            err.code = rc          # RRV_E_* of include/rerevst_hip.h (-5 = RRV_E_NOMEM)
            raise err

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rrv_destroy(self._h)      # waits for every stream: nothing writes the open tickets' outputs after it
            self._h = None
        self._open = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ===== Sequence-Level Global Feature Sharing (test/framework.py:82-95) =====
    def _global_only(self, what):
        if not self.use_Global:   # the reference's frame-mode TransformerNet has no add/compute/clean either
            raise RRVError("%s() belongs to Sequence-Level Global Feature Sharing (use_Global=True)" % what)

    def _yuv_depth(self, in_format=None, out_format=None):
        """the uint16 formats carry their depth: install it (rrv_set_yuv_depth) before the call that reads or writes them"""
        bi = YUV_FORMATS[in_format].bits if in_format in YUV_FORMATS else 8
        bo = YUV_FORMATS[out_format].bits if out_format in YUV_FORMATS else 8
        if bi > 8 or bo > 8:
            self._chk(self._lib.rrv_set_yuv_depth(self._h, bi if bi > 8 else 0, bo if bo > 8 else 0))

    def add(self, patch, in_format="bgr", size=None, work_size=None, picture=None):
        """A sampled frame: uint8 BGR HWC, or with in_format "i420" / "nv12" and size=(H, W) 8-bit YUV 4:2:0 bytes
        [yuv_frame_bytes(H, W)] (or [B][..]: every frame, in order) read by the first kernel (rrv_add_from_yuv); in_format "i420p10" /
        "i420p12" / "i420p16" / "p010" / "p012" / "p016": uint16 samples of that depth.  (The depth is read when the deferred encoding
        runs: add frames of one depth between clean() and compute().)
        work_size=(H, W): the frame is resampled to that size on the GPU first, as transfer_frames(work_size=) does (rrv_add_scaled);
        size= stays the size of the frame as passed.
        picture=(y0, x0, h, w): only that window of the frame is added (rrv_add_picture; include/rerevst_hip.h "Picture area"): the saved
        state equals, byte for byte, that of adding the cropped frame; with work_size the window is resampled to it.  Not with "jpeg"."""
        self._global_only("add")
        work = None if work_size is None else _work_size(work_size)
        if picture is not None and in_format == "jpeg":
            _picture_args(picture, 8, 8, None, None, None, True)
        if in_format == "jpeg":      # (rrv_add_from_jpeg: one stream, or a list of them; the size comes from the stream)
            if size is not None:
                raise ValueError('in_format="jpeg": the size comes from the streams, size= does not apply')
            work = _work_size(work_size) if work_size is not None else (0, 0)
            for data in ([patch] if isinstance(patch, (bytes, bytearray, memoryview)) else patch):
                data = bytes(data)
                try:
                    self._chk(self._lib.rrv_add_from_jpeg(self._h, data, len(data), *work))
                except RRVError as e:
                    if getattr(e, "code", 0) == _lib.E_DATA:
                        raise ValueError(str(e)) from None
                    raise
            return
        if in_format != "bgr":
            a, H, W = yuv_frames_args(patch, in_format, size)
            self._yuv_depth(in_format)
        else:
            a = _u8_image(patch, "patch")[None]
            H, W = a.shape[1:3]
        pic = None if picture is None else _picture_args(picture, H, W, None, None, None, False)
        for f in a:
            src = f.ctypes.data_as(C.c_void_p)
            if pic is not None:
                self._chk(self._lib.rrv_add_picture(self._h, src, _host_in_desc(in_format), H, W, C.byref(pic), *(work if work is not None else (0, 0))))
            elif work is not None:
                self._chk(self._lib.rrv_add_scaled(self._h, src, _host_in_desc(in_format), H, W, *work))
            elif in_format != "bgr":
                self._chk(self._lib.rrv_add_from_yuv(self._h, src, YUV_FORMATS[in_format].layout, H, W))
            else:
                self._chk(self._lib.rrv_add(self._h, src, H, W))

    def compute(self):
        self._global_only("compute")
        self._chk(self._lib.rrv_compute(self._h))

    def set_debug(self, level):
        """Bounds-checked debug mode: 0 off, 1 verify guard bands / zero rings after every call, 2 after every kernel."""
        self._chk(self._lib.rrv_set_debug(self._h, int(level)))

    def debug_selftest(self):
        self._chk(self._lib.rrv_debug_selftest(self._h))

    def debug_fail_alloc(self, nth):
        """Failure injection: the nth next device allocation reports out-of-memory (0 disarms)."""
        self._chk(self._lib.rrv_debug_fail_alloc(self._h, int(nth)))

    def set_workspace_cap(self, nbytes):
        """compute() keeps all sampled frames' activations resident while they fit `nbytes` (default 64 GiB); beyond
        that it streams groups of frames one synchronisation point at a time (workspace independent of the frame count)."""
        self._chk(self._lib.rrv_set_workspace_cap(self._h, int(nbytes)))

    def last_compute_info(self):
        """(groups, frames per group, workspace bytes) of the last compute()."""
        g, n, b = C.c_int(), C.c_int(), C.c_size_t()
        self._chk(self._lib.rrv_last_compute_info(self._h, C.byref(g), C.byref(n), C.byref(b)))
        return g.value, n.value, b.value

    def clean(self):
        self._global_only("clean")
        self._chk(self._lib.rrv_clean(self._h))

    # ===== Style Transfer (test/framework.py:99-118) =====
    def prepare_style(self, style):
        """Single style image (test/framework.py:99) or a list of them
        ("Multi-style Interpolation/stylization.py":71)."""
        styles = style if isinstance(style, (list, tuple)) else [style]
        for sid, s in enumerate(styles):
            a = _u8_image(s, "style")
            self._chk(self._lib.rrv_prepare_style(self._h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1], sid))

    def _stream(self, t):
        """the current stream of t's device, as the entries take it"""
        import torch
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def _flags(self, pad_crop, on_stream=False):
        """RRV_TF_* of a call: the geometry, the handle's model, and for the tensor entries the caller's stream"""
        return (_lib.TF_ON_STREAM if on_stream else 0) | (_lib.TF_PAD_CROP if pad_crop else 0) | (0 if self.use_Global else _lib.TF_FRAME_MODE)

    def _source(self, x, space, layout, size, views=True, yuv=True):
        """The input side of a tensor call, resolved once (_Source): x as transfer_tensor reads it — an ImageView, a YUV tensor with `layout` a
        format name and size=(H, W) (where `yuv` is set: the entries that read YUV frames), or an image tensor in `layout` / `space`.  A strided
        image tensor that fits a view stays where it is where `views` is set (the entries that take views); any other is copied to a packed one."""
        if isinstance(x, ImageView):
            _on_device(x.storage, "x.storage", self.device)
            v = x.with_space(space, "x")
            return _Source(v.desc, v, x.storage.data_ptr(), x.frames, x.H, x.W, True, x.storage, x.layout, v.frame_stride * _ELEM_BYTES[v.desc.dtype])
        if yuv and layout in YUV_FORMATS:
            _yuv_in_pixel_space(layout, space)
            a = yuv_tensor_io_args(x, self.device, layout, size)
            desc, view = _host_in_desc(layout), None
        else:
            a = _tensor_io(x, self.device, views, space=space, layout=layout)
            desc, view = a.in_desc, a.in_view
        step = view.frame_stride * _ELEM_BYTES[desc.dtype] if view is not None else a.x.stride(0) * a.x.element_size() if a.batched else 0
        return _Source(desc, view, a.x.data_ptr(), a.B, a.H, a.W, a.batched, a.x, layout, step)

    def _target(self, out, out_layout, out_space, out_dtype, B, Ho, Wo, batched, like, default_layout):
        """The output side of a tensor call, resolved once (_Target): B frames of Ho x Wo — the size as delivered — into `out` (an ImageView, a
        tensor or a window of one: written in place) or a fresh tensor on like's device, in out_layout (default: the view's, else
        default_layout) / out_space / out_dtype."""
        import torch
        ov = out if isinstance(out, ImageView) else None
        if out_layout is None:
            out_layout = ov.layout if ov is not None else default_layout
        _check_out_layout(out_layout, out_space)
        if ov is not None:      # written in place, through the view
            _on_device(ov.storage, "out.storage", self.device)
            if out_layout != ov.layout:
                raise ValueError("out is an %r view, out_layout says %r" % (ov.layout, out_layout))
            if (ov.frames, ov.H, ov.W) != (B, Ho, Wo):
                raise ValueError("out must hold %d frames of %d x %d, got %d of %d x %d" % (B, Ho, Wo, ov.frames, ov.H, ov.W))
            view = ov.with_space(out_space, "out")
            if self._lib.rrv_image_view_check(C.byref(view), B, Ho, Wo, 1) != 0:
                raise ValueError("out: the planes and frames of an output view must not overlap")
            return _Target(view.desc, view, ov.storage.data_ptr(), out, out_layout, view.frame_stride * _ELEM_BYTES[view.desc.dtype])
        desc, shape, dtype, view = _tensor_out_args(self.device, B, Ho, Wo, batched, out_space, out_dtype, out_layout, True, out)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=like.device)
        step = view.frame_stride * _ELEM_BYTES[desc.dtype] if view is not None else out.stride(0) * out.element_size() if batched else 0
        return _Target(desc, view, out.data_ptr(), out, out_layout, step)

    def prepare_style_tensor(self, style, *, space="pixel", layout="nchw"):
        """prepare_style for style images already on the handle's GPU: one torch tensor [3,H,W] RGB (layout="nchw") or
        [H,W,3] BGR ("nhwc"), or a list of them (multi-style), uint8 or float32 in `space`: transfer_tensor's input
        conventions.  Read in the order of torch.cuda.current_stream(); complete when the call returns."""
        styles = style if isinstance(style, (list, tuple)) else [style]
        for sid, s in enumerate(styles):
            src = self._source(s, space, layout, None, views=False, yuv=False)      # (the style entry reads packed images)
            if src.batched:
                raise ValueError("a style is one image: [3,H,W] or [H,W,3], got shape %s" % (tuple(s.shape),))
            self._chk(self._lib.rrv_prepare_style_image_device(self._h, C.c_void_p(src.ptr), src.desc, src.H, src.W, sid, self._stream(s)))

    def resample_tensor(self, x, work_size, *, space="pixel", layout="nchw", size=None):
        """The resampler alone (rrv_resample_view_device): x as transfer_tensor takes it — an image tensor in `layout` / `space`, a YUV
        tensor with layout a format name and size=(SH, SW), or an ImageView — resampled to work_size=(H, W) on the GPU, in the order of
        the current stream.  Returns a float32 tensor [B,H,W,3] ([H,W,3] for an unbatched x): BGR, "pixel" space, not rounded to
        integers; transfer_tensor(y, layout="nhwc") on it is what transfer_tensor(x, work_size=) computes."""
        import torch
        H, W = _work_size(work_size)
        src = self._source(x, space, layout, size)
        self._yuv_depth(src.layout, None)
        out = torch.empty((src.B, H, W, 3), dtype=torch.float32, device=src.tensor.device)
        stream, v = self._stream(src.tensor), _whole_view(src, src.H, src.W)
        for _, nb, p, q in _chunks(src.B, (src.ptr, src.step), (out.data_ptr(), out.stride(0) * 4)):
            self._chk(self._lib.rrv_resample_view_device(self._h, p, C.byref(v), nb, src.H, src.W, H, W, q, stream))
        return out if src.batched else out[0]

    def shot_signatures(self, frames, in_format="bgr", size=None):
        """The shot signatures of host frames (include/rerevst_hip.h "Shots"): np.uint32 [B][16][32], a 32-bin luma histogram for each cell
        of a 4 x 4 grid over each frame's thumbnail (shot_plan), computed on the GPU; video.shot_distances and video.detect_cuts turn them
        into cuts.  Needs no torch and no prepared style.  in_format: every host form of transfer_frames — "bgr" (uint8 HWC frames: one
        [B][H][W][3] array or a list, whose sizes may differ: runs of equal size go to the GPU together), a YUV format name with
        size=(H, W), or "jpeg" (a list of bytes, grouped into runs of one size and chroma format; JFIF's colour space).  A stream the parser
        refuses or a corrupt frame raises ValueError with the frame's index in `frames` and the library's words."""
        if in_format == "jpeg":
            if size is not None:
                raise ValueError('in_format="jpeg": the size comes from the streams, size= does not apply')
            if isinstance(frames, (bytes, bytearray, memoryview)) or len(frames) < 1 or not all(isinstance(s, (bytes, bytearray, memoryview)) for s in frames):
                raise ValueError('in_format="jpeg": frames must be a non-empty list of bytes, one baseline JPEG stream per frame')
            streams = [bytes(s) for s in frames]
            infos = [_jpeg_parse(s, "frame %d" % b) for b, s in enumerate(streams)]
            out = np.empty((len(streams), 16, 32), np.uint32)
            for b0, nb in _runs([(f.H, f.W, f.chroma) for f in infos]):
                ptrs, sizes = (C.c_char_p * nb)(*streams[b0:b0 + nb]), (C.c_size_t * nb)(*[len(s) for s in streams[b0:b0 + nb]])
                try:
                    self._chk(self._lib.rrv_shot_signature_from_jpeg(self._h, ptrs, sizes, nb, out[b0:].ctypes.data_as(C.c_void_p)))
                except RRVError as e:
                    if getattr(e, "code", 0) == _lib.E_DATA:      # a refused or corrupt stream: the library's words, its index in the run made the caller's
                        raise ValueError(re.sub(r"\bframe (\d+)", lambda m: "frame %d" % (b0 + int(m.group(1))), str(e), count=1)) from None
                    raise
            return out
        if in_format != "bgr":
            a, H, W = yuv_frames_args(frames, in_format, size)
            self._yuv_depth(in_format)
            groups = [(a, H, W)]
        elif isinstance(frames, np.ndarray) and frames.ndim == 4:
            a = _u8_frames(frames, "frame")
            groups = [(a, a.shape[1], a.shape[2])]
        else:
            imgs = [_u8_image(f, "frame") for f in frames]
            if not imgs:
                raise ValueError("shot_signatures: no frames")
            groups = [(np.stack(imgs[b0:b0 + nb]), *imgs[b0].shape[:2]) for b0, nb in _runs([f.shape for f in imgs])]
        out = np.empty((sum(len(a) for a, _, _ in groups), 16, 32), np.uint32)
        b0 = 0
        for a, H, W in groups:
            self._chk(self._lib.rrv_shot_signature(self._h, a.ctypes.data_as(C.c_void_p), _host_in_desc(in_format), len(a), H, W, out[b0:].ctypes.data_as(C.c_void_p)))
            b0 += len(a)
        return out

    def shot_signatures_tensor(self, x, *, space="pixel", layout="nchw", size=None):
        """shot_signatures for frames already on the handle's GPU (rrv_shot_signature_view_device), with resample_tensor's input
        conventions: an image tensor in `layout` / `space`, a YUV tensor with layout a format name and size=(H, W), or an ImageView.  Runs in
        the order of the current stream and returns an int32 tensor [B,16,32] (B = 1 for an unbatched x) on x's device: the uint32 words of
        the signature, whose counts never reach 2^31.  Equals resample_tensor(x, shot_plan(H, W)) followed by the kernel, bit for bit."""
        import torch
        src = self._source(x, space, layout, size)
        self._yuv_depth(src.layout, None)
        out = torch.empty((src.B, 16, 32), dtype=torch.int32, device=src.tensor.device)
        stream, v = self._stream(src.tensor), _whole_view(src, src.H, src.W)
        for _, nb, p, q in _chunks(src.B, (src.ptr, src.step), (out.data_ptr(), 2048)):
            self._chk(self._lib.rrv_shot_signature_view_device(self._h, p, C.byref(v), nb, src.H, src.W, q, stream))
        return out

    def scan_frames(self, frames, in_format="bgr", size=None, threshold=10, signatures=True, profiles=True):
        """The whole detection pass over host frames in one upload (rrv_scan_frames; include/rerevst_hip.h "Picture area"): returns
        (signatures, profiles), np.uint32 [B][16][32] as shot_signatures gives them, word for word, and np.uint32 [B][H + W] as
        picture_profiles does; the one not asked for is None (asking for neither is a ValueError).  frames: one [B][H][W][3] uint8 BGR
        array or a list of equally sized frames, or with in_format a YUV format name and size=(H, W) the samples [B][..].  threshold: the
        profile's, 0..254 (10: ffmpeg cropdetect's 24 on limited-range codes moved to full range; not tuned on real footage)."""
        if not signatures and not profiles:
            raise ValueError("scan_frames: neither signatures nor profiles asked for")
        if in_format == "jpeg":
            raise ValueError('scan_frames: in_format="jpeg" is not offered (shot_signatures takes JPEG streams)')
        if in_format != "bgr":
            a, H, W = yuv_frames_args(frames, in_format, size)
            self._yuv_depth(in_format)
        else:
            a = _u8_frames(frames, "frame")
            H, W = a.shape[1:3]
        B = len(a)
        sig = np.empty((B, 16, 32), np.uint32) if signatures else None
        prof = np.empty((B, H + W), np.uint32) if profiles else None
        self._chk(self._lib.rrv_scan_frames(self._h, a.ctypes.data_as(C.c_void_p), _host_in_desc(in_format), B, H, W, int(threshold),
                                            sig.ctypes.data_as(C.c_void_p) if signatures else None, prof.ctypes.data_as(C.c_void_p) if profiles else None))
        return sig, prof

    def picture_profiles(self, frames, in_format="bgr", size=None, threshold=10):
        """The line profiles of host frames (include/rerevst_hip.h "Picture area"): np.uint32 [B][H + W], per frame the lit pixels of every
        row, then of every column (video.picture_profile restates it), computed on the GPU; video.detect_picture turns them into the
        active picture area.  scan_frames with the profiles alone."""
        return self.scan_frames(frames, in_format=in_format, size=size, threshold=threshold, signatures=False, profiles=True)[1]

    def picture_profiles_tensor(self, x, *, space="pixel", layout="nchw", size=None, threshold=10):
        """picture_profiles for frames already on the handle's GPU (rrv_picture_profile_view_device), with resample_tensor's input
        conventions.  Runs in the order of the current stream and returns an int32 tensor [B, H + W] (B = 1 for an unbatched x) on x's
        device: the uint32 words of the profile, whose counts never reach 2^31.  Equals resample_tensor(x, (H, W)) followed by the
        kernels, bit for bit."""
        import torch
        src = self._source(x, space, layout, size)
        self._yuv_depth(src.layout, None)
        n = src.H + src.W
        out = torch.empty((src.B, n), dtype=torch.int32, device=src.tensor.device)
        stream, v = self._stream(src.tensor), _whole_view(src, src.H, src.W)
        for _, nb, p, q in _chunks(src.B, (src.ptr, src.step), (out.data_ptr(), 4 * n)):
            self._chk(self._lib.rrv_picture_profile_view_device(self._h, p, C.byref(v), nb, src.H, src.W, int(threshold), q, stream))
        return out

    def add_tensor(self, x, *, space="pixel", layout="nchw", size=None, work_size=None, picture=None):
        """add for sampled frames already on the handle's GPU (transfer_tensor's input conventions): one image, or a batch
        [B,3,H,W] / [B,H,W,3] whose images are added in order.  work_size=(H, W): each frame is resampled to that size on the GPU
        first (rrv_add_scaled_view_device), as transfer_tensor(work_size=) does; x may then also be a YUV tensor with size=(SH, SW).
        picture=(y0, x0, h, w): only that window of each frame is added (rrv_add_picture_view_device), as add(picture=) does; x may then
        also be a YUV tensor with size=(SH, SW)."""
        self._global_only("add")
        work = None if work_size is None else _work_size(work_size)
        src = self._source(x, space, layout, size, yuv=work is not None or picture is not None)
        pic = None if picture is None else _picture_args(picture, src.H, src.W, None, None, None, False)
        self._yuv_depth(src.layout, None)
        stream = self._stream(src.tensor)
        v = _whole_view(src, src.H, src.W) if work is not None or pic is not None else src.view
        for _, _, p in _chunks(src.B, (src.ptr, src.step), chunk=1):      # a surface, a crop or a pitched tensor: each frame is compacted on the GPU
            if pic is not None:
                self._chk(self._lib.rrv_add_picture_view_device(self._h, p, C.byref(v), src.H, src.W, C.byref(pic), *(work if work is not None else (0, 0)), stream))
            elif work is not None:
                self._chk(self._lib.rrv_add_scaled_view_device(self._h, p, C.byref(v), src.H, src.W, *work, stream))
            elif v is not None:
                self._chk(self._lib.rrv_add_view_device(self._h, p, C.byref(v), src.H, src.W, stream))
            else:
                self._chk(self._lib.rrv_add_image_device(self._h, p, src.desc, src.H, src.W, stream))

    def transfer(self, frame, style_weight=None, dtype=np.float32):
        """uint8 BGR HWC frame -> float32 BGR HWC in 0..255 (test/framework.py:106-118).
        With `style_weight` (list of floats) the saved state of the prepared styles is
        blended first (stylization.py:94-100).  dtype=np.uint8: the frame as cv2.imwrite would write it (the float
        output rounded half to even and saturated, on the GPU): a quarter of the bytes."""
        a = _u8_image(frame, "frame")
        H, W = a.shape[:2]
        out, u8 = _output((*_stylized_size(H, W), 3), dtype, None)
        if not self.use_Global:
            fn = self._lib.rrv_transfer_frame_mode_u8 if u8 else self._lib.rrv_transfer_frame_mode
            self._chk(fn(self._h, a.ctypes.data_as(C.c_void_p), H, W, out.ctypes.data_as(C.c_void_p)))
            return out
        if style_weight is None:      # the reference's hot call: plain addresses (ctypes' data_as() objects cost ~10 us a call)
            fn = self._lib.rrv_transfer_u8 if u8 else self._lib.rrv_transfer
            rc = fn(self._h, a.__array_interface__["data"][0], H, W, out.__array_interface__["data"][0])
            if rc != 0:
                self._chk(rc)
            return out
        w = (C.c_float * len(style_weight))(*[float(v) for v in style_weight])
        fn = self._lib.rrv_transfer_blend_u8 if u8 else self._lib.rrv_transfer_blend
        self._chk(fn(self._h, a.ctypes.data_as(C.c_void_p), H, W, w, len(style_weight), out.ctypes.data_as(C.c_void_p)))
        return out

    # ===== look-ahead form of transfer() for a one-frame-per-call loop =====
    def transfer_async(self, frame, out=None, dtype=np.float32):
        """Queue one frame (H2D copy, kernels, D2H copy) and return a ticket at once; ``result(ticket)`` returns the
        stylized frame.  A driver loop written as

            prev = None
            for frame in frames:
                t = framework.transfer_async(frame)
                if prev is not None: write(framework.result(prev))
                prev = t
            write(framework.result(prev))

        overlaps frame i+1's copy-in and kernels with frame i's kernel tails, copy-out and file write.  Up to four
        tickets may be open (each on its own stream with a quarter of the CUs per launch): keeping three frames
        submitted ahead of the one being collected gives the best rate.  Same arithmetic as transfer(): bit-identical results.
        dtype / a uint8 `out`: uint8 output as transfer(dtype=np.uint8)."""
        if not self.use_Global:
            raise RRVError("transfer_async() needs the global-feature-sharing model (use_Global=True)")
        a = _u8_image(frame, "frame")
        H, W = a.shape[:2]
        out, u8 = _output((*_stylized_size(H, W), 3), dtype, out)
        t = C.c_long(-1)
        fn = self._lib.rrv_transfer_async_u8 if u8 else self._lib.rrv_transfer_async
        self._chk(fn(self._h, a.ctypes.data_as(C.c_void_p), H, W, out.ctypes.data_as(C.c_void_p), C.byref(t)))
        # The library owns `out` until the ticket is collected or retired: a caller that drops the ticket (an exception in
        # its loop, `prev` overwritten) must not hand the block back to the pool under a running kernel.  Submitting
        # ticket t retired ticket t - 4 (four staging sets), so only the last four stay referenced here.
        self._open[t.value] = out
        for old in [k for k in self._open if k <= t.value - 4]:
            del self._open[old]
        return (t.value, out)

    def result(self, ticket):
        tid, out = ticket
        self._chk(self._lib.rrv_transfer_wait(self._h, tid))
        self._open.pop(tid, None)
        return out

    # ===== device-resident entry (what bench.py times) =====
    # With use_Global=False the batch / frames / device entries run the frame-mode model (rrv_transfer_frame_mode_*): each frame
    # gets its own statistics, bit-identical to transfer() on that frame alone.  dtype=np.uint8: d_out receives uint8 BGR
    # (the *_device_u8 entries), 3 bytes per pixel instead of 12.
    def _entry(self, name, u8):
        return getattr(self._lib, name + ("_u8" if u8 else ""))

    def transfer_device(self, d_in_ptr, H, W, d_out_ptr, dtype=np.float32):
        if not self.use_Global:
            self.transfer_batch_device(d_in_ptr, 1, H, W, d_out_ptr, dtype)
            return
        self._chk(self._entry("rrv_transfer_device", _out_u8(dtype))(self._h, C.c_void_p(d_in_ptr), H, W, C.c_void_p(d_out_ptr)))

    def transfer_batch_device(self, d_in_ptr, B, H, W, d_out_ptr, dtype=np.float32):
        """[B][H][W][3] uint8 in HBM -> [B][H][W][3] float32 (or uint8) in HBM, asynchronous on the library stream."""
        name = "rrv_transfer_batch_device" if self.use_Global else "rrv_transfer_frame_mode_batch_device"
        self._chk(self._entry(name, _out_u8(dtype))(self._h, C.c_void_p(d_in_ptr), B, H, W, C.c_void_p(d_out_ptr)))

    def _host_frames(self, frames, out, dtype, style_weights, style_masks, pad_crop, out_format="bgr", in_format="bgr", size=None, work_size=None,
                     out_size=None, guide=None, guide_radius=4, guide_eps=1e-3, strength=None, matte=None, keep=None, jpeg=None, picture=None):
        """transfer_batch (pad_crop False) / transfer_frames (True): the host array of the frames (uint8 BGR, or YUV 4:2:0 samples for
        size=(H, W)), the checked masks or weights, the output in out_format, and the C entry of that combination (_HOST_ENTRIES).
        jpeg: (quality, chroma, restart, cap) of out_format="jpeg" (rrv_transfer_jpeg): a list of bytes comes back"""
        is_jpeg = out_format == "jpeg"
        if picture is not None:
            return self._host_picture(frames, out, dtype, style_weights, style_masks, out_format, in_format, size, work_size, out_size, guide, guide_radius,
                                      guide_eps, strength, matte, keep, picture)
        if is_jpeg:
            _jpeg_alone(style_weights, style_masks, 'out_format="jpeg"')
            if out is not None or np.dtype(dtype) != np.float32:
                raise ValueError('out_format="jpeg" returns a list of bytes: out= and dtype= do not apply')
            j, out_format = jpeg_args(*jpeg[:3]), "bgr"
        yuv_in, yuv_out = in_format != "bgr", out_format != "bgr"
        if yuv_out and out_format not in YUV_FORMATS:
            raise ValueError("out_format must be 'bgr', %s, got %r" % (YUV_FORMAT_NAMES, out_format))
        if in_format == "jpeg":
            return self._host_from_jpeg(frames, out, dtype, style_weights, style_masks, pad_crop, out_format, j if is_jpeg else None, jpeg, size, work_size,
                                        out_size, guide, guide_radius, guide_eps, strength, matte, keep)
        if yuv_in:
            a, H, W = yuv_frames_args(frames, in_format, size)
        else:
            a = _u8_frames(frames, "frame")
            H, W = a.shape[1:3]
        B = a.shape[0]
        # Scaling: the frames as passed are SH x SW and H x W becomes the working size (SH = SW = 0: no input scaling); the stylized working
        # frame leaves at its own size, or resampled to DH x DW.
        SH = SW = 0
        if out_size is not None:
            _no_styles_with_out_size(style_weights, style_masks)
            DH, DW = _out_size(out_size, (H, W))
        elif work_size is not None:
            _no_styles_with_work_size(style_weights, style_masks)
        if work_size is not None:
            (SH, SW), (H, W) = (H, W), _work_size(work_size)
        m = None if style_masks is None else style_mask_args(style_masks, style_weights, B, H, W, self.style_num, self.device, self.use_Global)
        Ho, Wo = (DH, DW) if out_size is not None else _stylized_size(H, W, pad_crop)
        comp = _composite_args(strength, matte, keep, style_weights, style_masks, B, Ho, Wo)
        if is_jpeg:      # (r = 0: bilinear delivery; DH = DW = 0: the working frame is delivered; a null request: nothing is composited)
            cap = jpeg_slot_bytes(Ho, Wo, jpeg[1], jpeg[2], jpeg[3])
            r, eps = _guide_args(guide, guide_radius, guide_eps, out_size) if guide is not None else (0, 0.0)
            req = comp.request(0, B) if comp is not None else None
            data, sizes = np.empty((B, cap), np.uint8), np.zeros(B, np.int32)
            self._yuv_depth(in_format, None)
            self._chk(self._lib.rrv_transfer_jpeg(self._h, a.ctypes.data_as(C.c_void_p), _host_in_desc(in_format), B, SH, SW, H, W,
                                                  *((DH, DW) if out_size is not None else (0, 0)), r, eps, C.byref(req) if req is not None else None, C.byref(j),
                                                  data.ctypes.data_as(C.c_void_p), cap, sizes.ctypes.data_as(C.c_void_p), self._flags(pad_crop)))
            return jpeg_frames(data, sizes)
        out, u8 = _output((B, Ho, Wo, 3), dtype, out, out_format)
        self._yuv_depth(in_format, out_format)
        desc = _lib.ImageDesc(_lib.DT_U16 if out.dtype == np.uint16 else _lib.DT_U8 if u8 else _lib.DT_F32,
                              YUV_FORMATS[out_format].layout if yuv_out else _lib.LAY_HWC_BGR, _lib.SP_PIXEL)
        if m is not None:
            blend, styles = _MASK, (m.host.ctypes.data_as(C.POINTER(C.c_float)), m.S, m.images)
        elif style_weights is not None:
            w = style_weight_args(style_weights, B, self.style_num, self.device, self.use_Global)
            blend, styles = _BLEND, (w.host.ctypes.data_as(C.POINTER(C.c_float)), w.S)
        else:
            blend, styles = _PLAIN, ()
        # The C entry and its arguments: the scaled families take descriptors on both sides; the others go by (input is YUV, output is YUV) and
        # what blends the styles (_HOST_ENTRIES), and the plain BGR entry also names the model and the geometry.
        src, dst, flags = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), self._flags(pad_crop)
        name = _HOST_ENTRIES[yuv_in, yuv_out][blend].format(model="" if self.use_Global else "_frame_mode", geometry="_frames" if pad_crop else "_batch")
        if comp is not None:      # (r = 0: bilinear delivery; DH = DW = 0: the working frame is delivered)
            r, eps = _guide_args(guide, guide_radius, guide_eps, out_size) if guide is not None else (0, 0.0)
            req = comp.request(0, B)
            name, args = "rrv_transfer_composite", (src, _host_in_desc(in_format), B, SH, SW, H, W, *((DH, DW) if out_size is not None else (0, 0)), r, eps,
                                                    C.byref(req), dst, desc, flags)
        elif guide is not None:
            r, eps = _guide_args(guide, guide_radius, guide_eps, out_size)
            name, args = "rrv_transfer_guided", (src, _host_in_desc(in_format), B, SH, SW, H, W, DH, DW, r, eps, dst, desc, flags)
        elif out_size is not None:
            name, args = "rrv_transfer_deliver", (src, _host_in_desc(in_format), B, SH, SW, H, W, DH, DW, dst, desc, flags)
        elif work_size is not None:
            name, args = "rrv_transfer_scaled", (src, _host_in_desc(in_format), B, SH, SW, H, W, dst, desc, flags)
        elif yuv_in:      # (h, in, in_layout, B, H, W, [weights, S | masks, S, images,] out, its descriptor, flags)
            args = (src, YUV_FORMATS[in_format].layout, B, H, W, *styles, dst, desc, flags)
        elif yuv_out:     # (h, in, B, H, W, flags | [weights, S | masks, S, images,] pad_crop, layout, out)
            args = (src, B, H, W, *((flags,) if blend == _PLAIN else styles + (int(pad_crop),)), desc.layout, dst)
        else:             # (h, in, B, H, W, [weights, S, pad_crop | masks, S, images, pad_crop,] out); the _u8 twin by the output's dtype
            name += "_u8" if u8 else ""
            args = (src, B, H, W, *(() if blend == _PLAIN else styles + (int(pad_crop),)), dst)
        self._chk(getattr(self._lib, name)(self._h, *args))
        return out

    def _host_picture(self, frames, out, dtype, style_weights, style_masks, out_format, in_format, size, work_size, out_size, guide, guide_radius, guide_eps,
                      strength, matte, keep, picture):
        """picture= of transfer_batch / transfer_frames (rrv_transfer_picture): the window is stylized, the frame comes back at its own size"""
        if in_format == "jpeg" or out_format == "jpeg":
            _picture_args(picture, 8, 8, None, None, None, True)
        yuv_out = out_format != "bgr"
        if yuv_out and out_format not in YUV_FORMATS:
            raise ValueError("out_format must be 'bgr', %s, got %r" % (YUV_FORMAT_NAMES, out_format))
        if in_format != "bgr":
            a, H, W = yuv_frames_args(frames, in_format, size)
        else:
            a = _u8_frames(frames, "frame")
            H, W = a.shape[1:3]
        B = a.shape[0]
        pic = _picture_args(picture, H, W, out_size, style_weights, style_masks, False)
        work = (0, 0) if work_size is None else _work_size(work_size)
        r, eps = _guide_args(guide, guide_radius, guide_eps, "source") if guide is not None else (0, 0.0)
        comp = _composite_args(strength, matte, keep, None, None, B, pic.h, pic.w)
        req = comp.request(0, B) if comp is not None else None
        out, u8 = _output((B, H, W, 3), dtype, out, out_format)
        self._yuv_depth(in_format, out_format)
        desc = _lib.ImageDesc(_lib.DT_U16 if out.dtype == np.uint16 else _lib.DT_U8 if u8 else _lib.DT_F32,
                              YUV_FORMATS[out_format].layout if yuv_out else _lib.LAY_HWC_BGR, _lib.SP_PIXEL)
        self._chk(self._lib.rrv_transfer_picture(self._h, a.ctypes.data_as(C.c_void_p), _host_in_desc(in_format), B, H, W, C.byref(pic), *work, r, eps,
                                                 C.byref(req) if req is not None else None, out.ctypes.data_as(C.c_void_p), desc, self._flags(True)))
        return out

    def _host_from_jpeg(self, streams, out, dtype, style_weights, style_masks, pad_crop, out_format, j, jpeg, size, work_size, out_size, guide, guide_radius,
                        guide_eps, strength, matte, keep):
        """in_format="jpeg" of transfer_batch / transfer_frames (rrv_transfer_from_jpeg, rrv_transfer_jpeg_from_jpeg): `streams` a list of bytes,
        one baseline JPEG stream per frame; the size comes from the streams.  j: the rrv_jpeg of out_format="jpeg", else None."""
        _jpeg_alone(style_weights, style_masks, 'in_format="jpeg"')
        if size is not None:
            raise ValueError('in_format="jpeg": the size comes from the streams, size= does not apply')
        if isinstance(streams, (bytes, bytearray, memoryview)) or len(streams) < 1 or not all(isinstance(s, (bytes, bytearray, memoryview)) for s in streams):
            raise ValueError('in_format="jpeg": frames must be a non-empty list of bytes, one baseline JPEG stream per frame')
        streams = [bytes(s) for s in streams]
        f = _jpeg_parse(streams[0], "frame 0")
        B, H, W = len(streams), f.H, f.W
        for b in range(1, B):      # (the library parses them again; a stream it would refuse, or another size, is a ValueError here, before any GPU work)
            g = _jpeg_parse(streams[b], "frame %d" % b)
            if (g.H, g.W, g.chroma) != (f.H, f.W, f.chroma):
                raise ValueError("frame %d is %d x %d, chroma %d; frame 0 is %d x %d, chroma %d: the frames of one call share H, W and the chroma format"
                                 % (b, g.H, g.W, g.chroma, f.H, f.W, f.chroma))
        WH = WW = 0
        if out_size is not None:
            DH, DW = _out_size(out_size, (H, W))
        if work_size is not None:
            H, W = WH, WW = _work_size(work_size)
        Ho, Wo = (DH, DW) if out_size is not None else _stylized_size(H, W, pad_crop)
        comp = _composite_args(strength, matte, keep, None, None, B, Ho, Wo)
        r, eps = _guide_args(guide, guide_radius, guide_eps, out_size) if guide is not None else (0, 0.0)
        req = comp.request(0, B) if comp is not None else None
        ptrs, sizes = (C.c_char_p * B)(*streams), (C.c_size_t * B)(*[len(s) for s in streams])
        head = (self._h, ptrs, sizes, B, WH, WW, *((DH, DW) if out_size is not None else (0, 0)), r, eps, C.byref(req) if req is not None else None)
        try:
            if j is not None:
                cap = jpeg_slot_bytes(Ho, Wo, jpeg[1], jpeg[2], jpeg[3])
                data, osz = np.empty((B, cap), np.uint8), np.zeros(B, np.int32)
                self._chk(self._lib.rrv_transfer_jpeg_from_jpeg(*head, C.byref(j), data.ctypes.data_as(C.c_void_p), cap, osz.ctypes.data_as(C.c_void_p), self._flags(pad_crop)))
                return jpeg_frames(data, osz)
            yuv_out = out_format != "bgr"
            out, u8 = _output((B, Ho, Wo, 3), dtype, out, out_format)
            self._yuv_depth(None, out_format)
            desc = _lib.ImageDesc(_lib.DT_U16 if out.dtype == np.uint16 else _lib.DT_U8 if u8 else _lib.DT_F32,
                                  YUV_FORMATS[out_format].layout if yuv_out else _lib.LAY_HWC_BGR, _lib.SP_PIXEL)
            self._chk(self._lib.rrv_transfer_from_jpeg(*head, out.ctypes.data_as(C.c_void_p), desc, self._flags(pad_crop)))
            return out
        except RRVError as e:
            if getattr(e, "code", 0) == _lib.E_DATA:      # a refused or corrupt stream: the library's words
                raise ValueError(str(e)) from None
            raise

    def transfer_batch(self, frames, out=None, dtype=np.float32, style_weights=None, style_masks=None, out_format="bgr", in_format="bgr", size=None,
                       work_size=None, out_size=None, guide=None, guide_radius=4, guide_eps=1e-3, strength=None, matte=None, keep=None,
                       jpeg_quality=90, jpeg_chroma="420", jpeg_restart=None, jpeg_cap=None, picture=None):
        """Stylize equally sized uint8 BGR frames (a list, or one [B][H][W][3] array) in one call; sub-batches are
        pipelined inside the library (copy in / kernels / copy out).  `out`: optional float32 or uint8 [B][H][W][3] array
        to fill instead of allocating a fresh one (its dtype selects the output format; else `dtype` does).
        style_weights: multi-style interpolation ("Multi-style Interpolation/stylization.py":94-100) from the frames: [B][S]
        weights, frame b blending the saved state of styles 0..S-1 with style_weights[b] (one [S] vector: every frame);
        frame b equals transfer(frames[b], style_weight=style_weights[b]), bit for bit for a fixed kernel choice.
        style_masks: the styles blended PER PIXEL instead: a float32 ndarray [B][S][H][W] (or [S][H][W]: every frame) at the
        frames' resolution; every saved quantity becomes sum_s m_s(p) q_s at each decoder pixel p, m the mean of the mask
        over the input pixels p covers (rrv_transfer_mask_batch).  Not normalised; mutually exclusive with style_weights.
        out_format: "bgr" (default), or "i420" / "nv12": 8-bit YUV 4:2:0 converted on the GPU with the matrix of set_yuv_matrix
        (rrv_transfer_yuv and its blend / mask forms): a uint8 [B][yuv_frame_bytes(Ho, Wo)] array (`out` of that shape is
        filled; yuv_planes() gives the planes), 1.5 bytes per pixel over PCIe; composes with style_weights / style_masks.
        in_format: "bgr" (default), or "i420" / "nv12" with size=(H, W): `frames` is a uint8 array [B][yuv_frame_bytes(H, W)] of 8-bit
        YUV 4:2:0 frames, read by the first kernel with the matrix of set_yuv_input_matrix (the rrv_*_from_yuv entries): 1.5 bytes
        per pixel in as well, and no conversion on the host.  A wrong byte count or a missing size raises ValueError.
        10 / 12 / 16 bits: in_format / out_format "i420p10" | "i420p12" | "i420p16" (planar, the code in the low bits: ffmpeg's
        yuv420p10le, Y4M C420p10) and "p010" | "p012" | "p016" (semi-planar, the code in the high bits: hardware decoders / encoders);
        the arrays are uint16 [B][yuv_frame_bytes(H, W)] (that many SAMPLES), the name carries the depth (rrv_set_yuv_depth is called
        here), the matrices are those of set_yuv_matrix / set_yuv_input_matrix(.., bits=) — by default BT.601 limited range at that
        depth.  Any mix of input and output depth and layout works.  A wrong dtype or shape raises ValueError before any GPU work.
        4:2:2 and 4:4:4: "i422" | "nv16" | "i422p10" / "p12" / "p16" | "p210" / "p212" / "p216" and "i444" | "nv24" | "i444p10" / "p12" /
        "p16" | "p410" / "p412" / "p416" (ffmpeg yuv422p, nv16, yuv422p10le, p210le, yuv444p, nv24, yuv444p10le, p410le, ..), under the
        rules of the 4:2:0 name they extend; a frame is yuv_frame_bytes(H, W, chroma="422" | "444") samples, and any mix of chroma format,
        depth and layout between input and output works ("nv12" in, "p210" out).
        work_size=(H, W): the frames are resampled to that working size on the GPU first (rrv_transfer_scaled: an antialiased triangle
        filter, include/rerevst_hip.h "Scaling") and the result has the working size; size= stays the size of YUV frames as passed.
        Each axis scales by at most 8 either way.  Not with style_weights / style_masks (ValueError).
        out_size=(DH, DW) or "source": the stylized working frame is resampled to that size on the GPU on its way out (rrv_transfer_deliver;
        include/rerevst_hip.h "Scaling, output size") and converted to `out` / `dtype` / out_format there: [B][DH][DW][3], or the YUV frames
        of that size.  "source" is the size of the frames as passed: with work_size, "stylize at the working size, give me back my
        resolution"; without it, H x W in place of 8*(H//8) x 8*(W//8).  At most 8 either way per axis; not with style_weights /
        style_masks (ValueError).
        guide="source" with out_size="source" (or that size): guided delivery (rrv_transfer_guided; include/rerevst_hip.h "Guided delivery").
        The stylized working frame is upsampled along the edges of the source's luma with the fast guided filter instead of bilinearly:
        guide_radius is the box radius in working pixels (1..16), guide_eps the regulariser in the units of a 0..1 image (smaller keeps
        more of the source's edges, larger tends to the bilinear picture).  The working size must be delivered whole: H and W of the
        working frame multiples of 8 (transfer_frames: any).  video.guided_upsample restates the arithmetic in numpy.
        strength / matte / keep: compositing with the frames as passed (rrv_transfer_composite; include/rerevst_hip.h "Compositing"), on
        the GPU, behind the delivery or guided stage and in front of out_format / dtype.  strength: one number in 0..1 or one per frame, how
        much of the stylized frame shows; matte: a float32 (0..1) or uint8 (0..255) array [B or 1][Ho][Wo] at the delivered size, where it
        shows; keep: "colour" ("color") keeps the source's colours and takes the stylized luminance, "luma" the reverse.  They combine with
        work_size, out_size, guide, in_format, out_format and dtype; the working size must be delivered whole as for guide=.  Not with
        style_weights / style_masks (ValueError).  video.composite restates the arithmetic in numpy.
        out_format="jpeg": the delivered frame is encoded as baseline JPEG on the GPU (rrv_transfer_jpeg; include/rerevst_hip.h "JPEG
        output") and a list of B `bytes` comes back, each a complete .jpg file: jpeg_quality 1..100, jpeg_chroma "420" | "422" | "444",
        jpeg_restart the MCUs per restart interval (None: one MCU row), jpeg_cap the bytes reserved per frame (None: two per delivered pixel
        plus the header; a frame that does not fit raises a ValueError that names jpeg_cap).  It combines with work_size, out_size, guide,
        strength / matte / keep and in_format; not with style_weights / style_masks, out= or dtype=.
        in_format="jpeg": `frames` is a list of `bytes`, one baseline JPEG stream per frame, all of one size and chroma format, decoded on the
        GPU (rrv_transfer_from_jpeg / rrv_transfer_jpeg_from_jpeg; include/rerevst_hip.h "JPEG input"); the size comes from the streams
        (size= is refused), the colour space is JFIF's whatever set_yuv_input_matrix holds, and it combines with work_size, out_size, guide,
        strength / matte / keep, every out_format (no matte with out_format="jpeg") and dtype; not with style_weights / style_masks.  A
        stream the parser refuses or a corrupt frame raises ValueError with the frame's index and the library's words.
        picture=(y0, x0, h, w): the active picture area (rrv_transfer_picture; include/rerevst_hip.h "Picture area").  Only that window of
        the frames is stylized, with transfer_frames' geometry whichever of the two is called (reflect padding inside the window, so no bar
        bends the strokes), and the frames come back at their own size: outside the window every pixel is the source's, passed through the
        input and output conversions (uint8 BGR in and out: the source's bytes).  out_size is implied to be "source" (another size is a
        ValueError).  It combines with work_size (the window is resampled to it), guide, strength / matte / keep (a matte has the window's
        size [B or 1][h][w]), in_format, out_format and dtype; not with style_weights / style_masks or the "jpeg" forms (ValueError)."""
        return self._host_frames(frames, out, dtype, style_weights, style_masks, False, out_format, in_format, size, work_size, out_size, guide,
                                 guide_radius, guide_eps, strength, matte, keep, (jpeg_quality, jpeg_chroma, jpeg_restart, jpeg_cap), picture)

    def transfer_frames(self, frames, out=None, dtype=np.float32, style_weights=None, style_masks=None, out_format="bgr", in_format="bgr", size=None,
                        work_size=None, out_size=None, guide=None, guide_radius=4, guide_eps=1e-3, strength=None, matte=None, keep=None,
                        jpeg_quality=90, jpeg_chroma="420", jpeg_restart=None, jpeg_cap=None, picture=None):
        """UNPADDED uint8 BGR frames (a list, or one [B][H][W][3] array) -> [B][H][W][3] float32 stylized frames.
        The reference driver's ReshapeTool.process + crop (test/generate_real_video.py:61-83, :167) run on the
        device, without the padded copies on the host or over PCIe: the same picture as pad -> transfer -> crop (bit-identical
        for a fixed kernel choice, set_f43(0) / set_f43(2); the default picks kernels per launch geometry, the crop window included).
        `out` / `dtype` as in transfer_batch: uint8 output is to_uint8 of the float output, computed on the GPU.
        style_weights: [B][S] (or [S]) blend weights per frame, as in transfer_batch.
        style_masks: [B][S][H][W] (or [S][H][W]) per-pixel blend weights for the UNPADDED frames, as in transfer_batch; the
        mask is reflect-padded on the device as the frame is.
        out_format: "i420" / "nv12" as in transfer_batch: uint8 [B][yuv_frame_bytes(H, W)]; an odd H or W gives a last chroma row
        or column that covers one pixel row / column (replicated, never the padding).
        in_format / size: "i420" / "nv12" input frames [B][yuv_frame_bytes(H, W)], as in transfer_batch; with out_format set too, a
        decoder's frames go to an encoder with no pixel touched on the host.
        work_size=(H, W): as in transfer_batch; the resampled H x W frame is what gets reflect-padded and cropped, and [B][H][W][3]
        (or the YUV frames of that size) is what comes back.
        out_size=(DH, DW) or "source": as in transfer_batch; the cropped H x W frame is what gets resampled to DH x DW.
        guide / guide_radius / guide_eps: guided delivery, as in transfer_batch; any working size.
        strength / matte / keep: compositing with the frames as passed, as in transfer_batch; any working size.
        out_format="jpeg" with jpeg_quality / jpeg_chroma / jpeg_restart / jpeg_cap: a list of `bytes`, as in transfer_batch.
        in_format="jpeg": a list of `bytes` in, as in transfer_batch.
        picture=(y0, x0, h, w): the active picture area, as in transfer_batch."""
        return self._host_frames(frames, out, dtype, style_weights, style_masks, True, out_format, in_format, size, work_size, out_size, guide,
                                 guide_radius, guide_eps, strength, matte, keep, (jpeg_quality, jpeg_chroma, jpeg_restart, jpeg_cap), picture)

    def transfer_frames_device(self, d_in_ptr, B, H, W, d_out_ptr, dtype=np.float32):
        """Same on HBM buffers ([B][H][W][3] uint8 -> [B][H][W][3] float32 or uint8), asynchronous on the library stream."""
        name = "rrv_transfer_frames_device" if self.use_Global else "rrv_transfer_frame_mode_frames_device"
        self._chk(self._entry(name, _out_u8(dtype))(self._h, C.c_void_p(d_in_ptr), B, H, W, C.c_void_p(d_out_ptr)))

    def transfer_tensor(self, x, *, space="pixel", out_space="pixel", out_dtype=None, layout="nchw", out_layout=None,
                        pad_crop=False, out=None, style_weights=None, style_masks=None, size=None, work_size=None, out_size=None, guide=None,
                        guide_radius=4, guide_eps=1e-3, strength=None, matte=None, keep=None, jpeg_quality=90, jpeg_chroma="420", jpeg_restart=None,
                        jpeg_cap=None, picture=None):
        """Stylize torch tensors already on the handle's GPU, ordered on torch.cuda.current_stream(x.device) (no host sync).

        x: [B,3,H,W] RGB (layout="nchw", torch's convention) or [B,H,W,3] BGR ("nhwc", cv2's); unbatched [3,H,W] / [H,W,3]
        returns an unbatched result.  uint8 in 0..255, or float32 in the value space `space`: "pixel" 0..255, "unit" 0..1,
        "norm" the reference's transform_image output (x/255 - mean)/std.  The output is out_dtype (torch.float32 or
        torch.uint8; `out`'s dtype when given) in `out_layout` (default: `layout`) and `out_space`: "pixel" the values
        transfer_batch_device writes (uint8: its _u8 twin's), "unit" those / 255 exactly, "norm" the pre-clamp network
        output — with space="norm" as well, what the reference's `self.model(frame)` returns.  pad_crop: the geometry of
        transfer_frames (reflect pad in, crop out: [.., H, W]); otherwise [.., 8*(H//8), 8*(W//8)].  With use_Global=False
        the frame-mode model runs.  Batches above 64 images are split into calls of 64.
        style_weights: multi-style interpolation, one weight vector per image: a host sequence / ndarray [B][S] (or [S]), or
        a float32 torch tensor [B,S] (or [S]) on the handle's device, which the library reads on the GPU in the order of
        the current stream — weights a kernel has just produced need no synchronisation and never visit the host.
        style_masks: the styles blended per pixel (rrv_transfer_image_mask_device): a float32 torch tensor [B,S,H,W] (or
        [S,H,W]: every image) on the handle's device, read in the order of the current stream with no host synchronisation,
        or a float32 ndarray of those shapes (copied to the device on that stream).  H, W are those of x.  Mutually exclusive
        with style_weights.
        out_layout "i420" / "nv12": 8-bit YUV 4:2:0 (the matrix of set_yuv_matrix), a uint8 tensor [B, yuv_frame_bytes(Ho, Wo)]
        ([yuv_frame_bytes] unbatched) in the "pixel" space; yuv_planes() gives views of the planes.
        layout "i420" / "nv12" with size=(H, W): x is a uint8 tensor [B, yuv_frame_bytes(H, W)] of 8-bit YUV 4:2:0 frames (a hardware
        decoder's NV12), read with the matrix of set_yuv_input_matrix (the rrv_*_from_yuv_device entries); out_layout then defaults
        to the same YUV layout, and may be "nchw" / "nhwc".
        layout / out_layout "i420p10" | "i420p12" | "i420p16" | "p010" | "p012" | "p016": 10 / 12 / 16-bit samples as in transfer_batch,
        in torch.uint16 tensors (this build's torch has the dtype; a torch.int16 tensor holding the same bits, x.view(torch.int16),
        is taken too, and `out` may be one); a fresh output is torch.uint16.
        Strided tensors: an x that is a crop x[:, :, y0:y1, x0:x1], has pitched rows or is a grey tensor expanded to three channels
        (image_view_of says which strides fit) is read where it is, with no copy; any other non-contiguous x is copied.  `out` may be
        a window of a larger canvas: it is written in place and returned (the result is `out`); nothing outside the window is touched.
        x and / or out may be an ImageView: a pitched surface (a hardware decoder's NV12 / P010, an encoder's input) in a 1-D storage
        tensor; layout, out_layout and size then come from the view, the result is the `out` view.  A strided call delivers the bits
        of the contiguous call on the same pixels.  The memory x and out address must not overlap.
        work_size=(H, W): the frames (any of the forms above; size= stays the size of YUV frames as passed) are resampled to that working
        size on the GPU first (rrv_transfer_scaled_view_device; include/rerevst_hip.h "Scaling"), and the output has the working size:
        [.., H, W] with pad_crop, else [.., 8*(H//8), 8*(W//8)].  Not with style_weights / style_masks (ValueError).
        out_size=(DH, DW) or "source" (the size of the frames as passed): the stylized working frame is resampled to that size on the GPU
        on its way out (rrv_transfer_deliver_view_device; include/rerevst_hip.h "Scaling, output size"), with or without work_size, into
        any out_layout / out_space / out_dtype or `out` (a tensor, a window or an ImageView of DH x DW frames): [.., DH, DW].  A "norm"
        output is then the normalised delivered pixel (a resampled frame has no pre-clamp value).  Not with style_weights / style_masks.
        guide="source" with out_size="source" (or that size): guided delivery (rrv_transfer_guided_view_device; include/rerevst_hip.h "Guided
        delivery"), guide_radius in working pixels (1..16) and guide_eps in the units of a 0..1 image as in transfer_batch.  The call equals
        the float32 "nhwc" call at the working size, resample_tensor for the two guides and deliver_tensor(.., guide_lo=, guide_hi=).
        strength / matte / keep: compositing with x itself (rrv_transfer_composite_view_device; include/rerevst_hip.h "Compositing"), as in
        transfer_batch; matte a float32 or uint8 tensor [B or 1, Ho, Wo] on the handle's device, read in the order of the current stream
        like style_masks (an ndarray is copied there).  The call equals the float32 "nhwc" call with the same work_size / out_size / guide,
        resample_tensor for the source at the delivered size and composite_tensor.
        out_layout="jpeg": the delivered frame is encoded as baseline JPEG on the GPU (rrv_transfer_jpeg_view_device; include/rerevst_hip.h
        "JPEG output") with jpeg_quality / jpeg_chroma / jpeg_restart / jpeg_cap as in transfer_batch.  Returns (uint8 [B][cap] tensor, int32
        [B] sizes tensor) in stream order, as encode_jpeg_tensor does (framework.jpeg_frames reads them on the host); the call equals the
        float32 "nhwc" call followed by encode_jpeg_tensor.  Not with style_weights / style_masks, out=, out_dtype= or another out_space.
        picture=(y0, x0, h, w): the active picture area (rrv_transfer_picture_view_device; include/rerevst_hip.h "Picture area"), as in
        transfer_batch: pad_crop is forced, the output has the source's size (out_size is implied to be "source") in any out_layout /
        out_space / out_dtype or `out`, and a matte has the window's size.  The call equals resample_tensor(x, (H, W)) as the canvas, the
        float32 "nhwc" pad_crop call on the window (ImageView.window or the crop) with the same work_size / guide / strength / matte / keep and
        out_size="source" written into the canvas's window, and deliver_tensor(canvas, (H, W), ..), bit for bit in a fixed kernel mode."""
        import torch
        composite = strength is not None or matte is not None or keep is not None
        is_jpeg = isinstance(out_layout, str) and out_layout == "jpeg"
        if picture is not None:
            src = self._source(x, space, layout, size)
            pic = _picture_args(picture, src.H, src.W, out_size, style_weights, style_masks, is_jpeg)
            work = (0, 0) if work_size is None else _work_size(work_size)
            g_r, g_eps = _guide_args(guide, guide_radius, guide_eps, "source") if guide is not None else (0, 0.0)
            comp = _composite_args(strength, matte, keep, None, None, src.B, pic.h, pic.w, tensors=True, device=self.device)
            dst = self._target(out, out_layout, out_space, out_dtype, src.B, src.H, src.W, src.batched, src.tensor, default_layout=src.layout)
            if comp is not None:
                comp.on_device(src.tensor)
            vi, vo = _whole_view(src, src.H, src.W), _whole_view(dst, src.H, src.W)
            self._yuv_depth(src.layout, dst.layout)
            flags, stream = self._flags(True, on_stream=True), self._stream(src.tensor)
            for b0, nb, p, q in _chunks(src.B, (src.ptr, src.step), (dst.ptr, dst.step)):
                req = comp.request(b0, nb) if comp is not None else None
                self._chk(self._lib.rrv_transfer_picture_view_device(self._h, p, C.byref(vi), nb, src.H, src.W, C.byref(pic), *work, g_r, g_eps,
                                                                     C.byref(req) if req is not None else None, q, C.byref(vo), flags, stream))
            return dst.result
        if is_jpeg:
            _jpeg_alone(style_weights, style_masks, 'out_layout="jpeg"')
            if out is not None or out_dtype is not None or out_space != "pixel":
                raise ValueError('out_layout="jpeg" returns (bytes tensor, sizes tensor): out=, out_dtype= and out_space= do not apply')
            j = jpeg_args(jpeg_quality, jpeg_chroma, jpeg_restart)
        if guide is not None:
            g_r, g_eps = _guide_args(guide, guide_radius, guide_eps, out_size)
        if out_size is not None:
            _no_styles_with_out_size(style_weights, style_masks)
        elif work_size is not None:
            _no_styles_with_work_size(style_weights, style_masks)
        work = None if work_size is None else _work_size(work_size)
        scaled = work is not None or out_size is not None or composite or is_jpeg      # (the view entries serve every compositing and JPEG call)
        xv, ov = (t if isinstance(t, ImageView) else None for t in (x, out))
        # An unscaled call refuses in tensor_io_args' order and words (tests/call_record.json pins which refusal a call meets): the space
        # of a YUV surface first, and for a tensor x the names of both sides before x is looked at.
        if not scaled:
            if xv is not None and xv.layout in YUV_FORMATS:
                _yuv_in_pixel_space(xv.layout, space)
            if xv is None:
                _check_in_names(space, layout, size)
                _check_out_layout(out_layout if out_layout is not None else ov.layout if ov is not None else layout, out_space)
        src = self._source(x, space, layout, size)
        B, H, W, SH, SW = src.B, src.H, src.W, 0, 0
        if out_size is not None:
            DH, DW = _out_size(out_size, (H, W))
        if work is not None:      # the frames as passed are SH x SW; everything from here on has the working size
            (SH, SW), (H, W) = (H, W), work
        Ho, Wo = (DH, DW) if out_size is not None else _stylized_size(H, W, pad_crop)
        if not scaled and xv is None and ov is not None:      # (.. and the dtype of an output view for a tensor x, before the view is looked at)
            _tensor_out_args(self.device, B, Ho, Wo, src.batched, out_space, ov.storage.dtype, ov.layout if out_layout is None else out_layout, True, None)
        comp = _composite_args(strength, matte, keep, style_weights, style_masks, B, Ho, Wo, tensors=True, device=self.device)
        if is_jpeg:
            cap = jpeg_slot_bytes(Ho, Wo, jpeg_chroma, jpeg_restart, jpeg_cap)
            data = torch.empty((B, cap), dtype=torch.uint8, device=src.tensor.device)
            sizes = torch.empty((B,), dtype=torch.int32, device=src.tensor.device)
            if comp is not None:
                comp.on_device(src.tensor)
            vi = _whole_view(src, src.H, src.W)
            self._yuv_depth(src.layout, None)
            for b0, nb, p, q, sz in _chunks(B, (src.ptr, src.step), (data.data_ptr(), cap), (sizes.data_ptr(), 4)):
                req = comp.request(b0, nb) if comp is not None else None
                self._chk(self._lib.rrv_transfer_jpeg_view_device(self._h, p, C.byref(vi), nb, SH, SW, H, W, *((DH, DW) if out_size is not None else (0, 0)),
                                                                  g_r if guide is not None else 0, g_eps if guide is not None else 0.0,
                                                                  C.byref(req) if req is not None else None, C.byref(j), q, cap, sz,
                                                                  self._flags(pad_crop, on_stream=True), self._stream(src.tensor)))
            return data, sizes
        dst = self._target(out, out_layout, out_space, out_dtype, B, Ho, Wo, src.batched, src.tensor, default_layout=src.layout)
        if comp is not None:
            comp.on_device(src.tensor)
        # The view entries serve a call with a strided side and every scaled call (a packed side then goes as its contiguous view), the
        # descriptor entries every other: by (input is YUV), the _from_yuv_device entries taking the layout alone.
        if scaled or src.view is not None or dst.view is not None:
            vi, vo = _whole_view(src, src.H, src.W), _whole_view(dst, Ho, Wo)
            in_arg, out_arg, names = C.byref(vi), C.byref(vo), _VIEW_ENTRIES
        else:
            yuv_in = src.layout in YUV_FORMATS
            in_arg, out_arg, names = src.desc.layout if yuv_in else src.desc, dst.desc, _TENSOR_ENTRIES[yuv_in]
        w = m = None
        if style_masks is not None:
            m = style_mask_args(style_masks, style_weights, B, H, W, self.style_num, self.device, self.use_Global, tensors=True)
            md = m.dev if m.dev is not None else torch.from_numpy(m.host).to(src.tensor.device, non_blocking=False)
            md = md if m.images == 1 else md.reshape(B, -1)
        if style_weights is not None:
            w = style_weight_args(style_weights, B, self.style_num, self.device, self.use_Global, tensors=True)
            wd = w.dev.unsqueeze(0).expand(B, w.S).contiguous() if w.broadcast else w.dev
        flags = self._flags(pad_crop, on_stream=True)
        self._yuv_depth(src.layout, dst.layout)
        stream = self._stream(src.tensor)
        for b0, nb, p, q in _chunks(B, (src.ptr, src.step), (dst.ptr, dst.step)):
            if comp is not None:
                req = comp.request(b0, nb)
                self._chk(self._lib.rrv_transfer_composite_view_device(self._h, p, in_arg, nb, SH, SW, H, W, *((DH, DW) if out_size is not None else (0, 0)),
                                                                       g_r if guide is not None else 0, g_eps if guide is not None else 0.0, C.byref(req),
                                                                       q, out_arg, flags, stream))
            elif guide is not None:
                self._chk(self._lib.rrv_transfer_guided_view_device(self._h, p, in_arg, nb, SH, SW, H, W, DH, DW, g_r, g_eps, q, out_arg, flags, stream))
            elif out_size is not None:
                self._chk(self._lib.rrv_transfer_deliver_view_device(self._h, p, in_arg, nb, SH, SW, H, W, DH, DW, q, out_arg, flags, stream))
            elif work is not None:
                self._chk(self._lib.rrv_transfer_scaled_view_device(self._h, p, in_arg, nb, SH, SW, H, W, q, out_arg, flags, stream))
            elif m is not None:
                mp = md.data_ptr() if m.images == 1 else md[b0].data_ptr()
                self._chk(getattr(self._lib, names[_MASK])(self._h, p, in_arg, nb, H, W, C.c_void_p(mp), m.S, 1 if m.images == 1 else nb, q, out_arg, flags, stream))
            elif w is not None:       # the chunk's rows of the weights, by address: host memory, or HBM with TF_WEIGHTS_DEVICE
                wp = wd[b0].data_ptr() if wd is not None else w.host[b0].ctypes.data
                self._chk(getattr(self._lib, names[_BLEND])(self._h, p, in_arg, nb, H, W, C.c_void_p(wp), w.S, q, out_arg,
                                                            flags | (_lib.TF_WEIGHTS_DEVICE if wd is not None else 0), stream))
            else:
                self._chk(getattr(self._lib, names[_PLAIN])(self._h, p, in_arg, nb, H, W, q, out_arg, flags, stream))
        return dst.result

    def deliver_tensor(self, y, out_size, *, out_space="pixel", out_dtype=None, out_layout=None, out=None, guide_lo=None, guide_hi=None, guide_radius=4,
                       guide_eps=1e-3):
        """The delivery stage alone (rrv_deliver_view_device): y a float32 tensor [B,H,W,3] ([H,W,3]) on the handle's GPU, BGR, "pixel"
        space — what transfer_tensor(.., layout="nhwc") and resample_tensor return — resampled to out_size=(DH, DW) on the GPU and written
        as transfer_tensor(out_size=) writes it: out_layout ("nhwc" by default, "nchw", or a YUV format name), out_space, out_dtype, or
        `out` (a tensor, a window of a canvas, or an ImageView of DH x DW frames).  Ordered on the current stream, like resample_tensor.
        guide_lo, guide_hi: the guided stage alone instead (rrv_deliver_guided_view_device; include/rerevst_hip.h "Guided delivery"): float32
        tensors of y's form, the source at y's size and at out_size (resample_tensor gives both); guide_radius in pixels of y (1..16),
        guide_eps in the units of a 0..1 image.  out_size is at least y's size and at most 8 times it, per axis."""
        import torch
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.dim() not in (3, 4) or y.shape[-1] != 3:
            raise ValueError("y must be a float32 tensor [B,H,W,3] or [H,W,3] (BGR, 'pixel' space)")
        _on_device(y, "y", self.device)
        batched = y.dim() == 4
        yb = (y if batched else y.unsqueeze(0)).contiguous()
        B, H, W = yb.shape[:3]
        DH, DW = _out_size(out_size, (H, W))
        dst = self._target(out, out_layout, out_space, out_dtype, B, DH, DW, batched, y, default_layout="nhwc")
        vo = _whole_view(dst, DH, DW)
        self._yuv_depth(None, dst.layout)
        stream = self._stream(y)
        if guide_lo is not None or guide_hi is not None:
            if guide_lo is None or guide_hi is None:
                raise ValueError("guided delivery needs both guide_lo (the source at y's size) and guide_hi (the source at out_size)")
            glo, ghi = (self._guide_tensor(g, name, (B, gh, gw, 3), batched) for g, name, gh, gw in ((guide_lo, "guide_lo", H, W), (guide_hi, "guide_hi", DH, DW)))
            r, eps = _guide_args("source", guide_radius, guide_eps, out_size)
            for b0, nb, p, q in _chunks(B, (yb.data_ptr(), yb.stride(0) * 4), (dst.ptr, dst.step)):
                self._chk(self._lib.rrv_deliver_guided_view_device(self._h, p, C.c_void_p(glo[b0].data_ptr()), C.c_void_p(ghi[b0].data_ptr()), nb, H, W, DH, DW,
                                                                   r, eps, q, C.byref(vo), stream))
            return dst.result
        for _, nb, p, q in _chunks(B, (yb.data_ptr(), yb.stride(0) * 4), (dst.ptr, dst.step)):
            self._chk(self._lib.rrv_deliver_view_device(self._h, p, nb, H, W, DH, DW, q, C.byref(vo), stream))
        return dst.result

    def composite_tensor(self, stylized, source, *, strength=None, matte=None, keep=None, out_space="pixel", out_dtype=None, out_layout=None, out=None):
        """The compositing stage alone (rrv_composite_view_device; include/rerevst_hip.h "Compositing"): stylized and source float32 tensors
        [B,H,W,3] ([H,W,3]) on the handle's GPU, BGR, "pixel" space, of one size -- what transfer_tensor(.., layout="nhwc") and
        resample_tensor return -- mixed by strength (a number or one per frame, 0..1), matte (float32 or uint8 [B or 1, H, W], a tensor on
        the device or an ndarray) and keep (None, "colour" / "color", "luma") and written as deliver_tensor writes a frame of that size:
        out_layout ("nhwc" by default, "nchw", or a YUV format name), out_space, out_dtype, or `out`.  Ordered on the current stream.  The
        tensors need no alignment beyond their elements'.  video.composite restates the arithmetic in numpy."""
        import torch
        if not isinstance(stylized, torch.Tensor) or stylized.dtype != torch.float32 or stylized.dim() not in (3, 4) or stylized.shape[-1] != 3:
            raise ValueError("stylized must be a float32 tensor [B,H,W,3] or [H,W,3] (BGR, 'pixel' space)")
        _on_device(stylized, "stylized", self.device)
        batched = stylized.dim() == 4
        yb = (stylized if batched else stylized.unsqueeze(0)).contiguous()
        B, H, W = yb.shape[:3]
        sb = self._guide_tensor(source, "source", (B, H, W, 3), batched)
        comp = CompositeArgs(strength, matte, keep, B, H, W, tensors=True, device=self.device).on_device(yb)
        dst = self._target(out, out_layout, out_space, out_dtype, B, H, W, batched, stylized, default_layout="nhwc")
        vo = _whole_view(dst, H, W)
        self._yuv_depth(None, dst.layout)
        stream = self._stream(stylized)
        for b0, nb, p, q in _chunks(B, (yb.data_ptr(), yb.stride(0) * 4), (dst.ptr, dst.step)):
            req = comp.request(b0, nb)
            self._chk(self._lib.rrv_composite_view_device(self._h, p, C.c_void_p(sb[b0].data_ptr()), nb, H, W, C.byref(req), q, C.byref(vo), stream))
        return dst.result

    def _jpeg_frames(self, y, what):
        import torch
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.dim() not in (3, 4) or y.shape[-1] != 3:
            raise ValueError("%s must be a float32 tensor [B,H,W,3] or [H,W,3] (BGR, 'pixel' space)" % what)
        _on_device(y, what, self.device)
        return (y if y.dim() == 4 else y.unsqueeze(0)).contiguous()

    def jpeg_blocks_tensor(self, y, *, jpeg_quality=90, jpeg_chroma="420", jpeg_restart=None):
        """The first half of the JPEG stage alone (rrv_jpeg_blocks_device): the quantised coefficient blocks of y, an int16 tensor
        [B][blocks][64] in zigzag order, the blocks in scan order.  Ordered on the current stream."""
        import torch
        yb = self._jpeg_frames(y, "y")
        B, H, W = yb.shape[:3]
        j = jpeg_args(jpeg_quality, jpeg_chroma, jpeg_restart)
        blocks = jpeg_plan(H, W, jpeg_chroma, jpeg_restart)["blocks"]
        coef = torch.empty((B, blocks, 64), dtype=torch.int16, device=yb.device)
        for _, nb, p, q in _chunks(B, (yb.data_ptr(), yb.stride(0) * 4), (coef.data_ptr(), blocks * 128)):
            self._chk(self._lib.rrv_jpeg_blocks_device(self._h, p, nb, H, W, C.byref(j), q, self._stream(yb)))
        return coef

    def jpeg_entropy_tensor(self, coef, size, *, jpeg_quality=90, jpeg_chroma="420", jpeg_restart=None, jpeg_cap=None):
        """The second half alone (rrv_jpeg_entropy_device): coef an int16 tensor [B][blocks][64] as jpeg_blocks_tensor returns it, of frames of
        size=(H, W) -> (uint8 [B][cap] tensor, int32 [B] sizes tensor).  Ordered on the current stream."""
        import torch
        H, W = int(size[0]), int(size[1])
        j = jpeg_args(jpeg_quality, jpeg_chroma, jpeg_restart)
        cap = jpeg_slot_bytes(H, W, jpeg_chroma, jpeg_restart, jpeg_cap)
        blocks = jpeg_plan(H, W, jpeg_chroma, jpeg_restart)["blocks"]
        if not isinstance(coef, torch.Tensor) or coef.dtype != torch.int16 or coef.dim() != 3 or tuple(coef.shape[1:]) != (blocks, 64):
            raise ValueError("coef must be an int16 tensor [B][%d][64] for %d x %d frames" % (blocks, H, W))
        _on_device(coef, "coef", self.device)
        cb = coef.contiguous()
        B = cb.shape[0]
        data = torch.empty((B, cap), dtype=torch.uint8, device=cb.device)
        sizes = torch.empty((B,), dtype=torch.int32, device=cb.device)
        for _, nb, p, q, sz in _chunks(B, (cb.data_ptr(), blocks * 128), (data.data_ptr(), cap), (sizes.data_ptr(), 4)):
            self._chk(self._lib.rrv_jpeg_entropy_device(self._h, p, nb, H, W, C.byref(j), q, cap, sz, self._stream(cb)))
        return data, sizes

    def encode_jpeg_tensor(self, y, *, jpeg_quality=90, jpeg_chroma="420", jpeg_restart=None, jpeg_cap=None):
        """The JPEG stage alone (rrv_jpeg_encode_device; include/rerevst_hip.h "JPEG output"): y a float32 tensor [B,H,W,3] ([H,W,3]) on the
        handle's GPU, BGR, "pixel" space -- what transfer_tensor(.., layout="nhwc"), deliver_tensor and composite_tensor return -- encoded as
        baseline JPEG on the GPU.  Returns (uint8 [B][cap] tensor, int32 [B] sizes tensor) in stream order: frame b is data[b, :sizes[b]]; a
        frame that did not fit has sizes[b] = -(the bytes it needs).  jpeg_cap: bytes per slot (None: two per pixel plus the header).
        framework.jpeg_frames turns the pair into a list of bytes on the host."""
        import torch
        yb = self._jpeg_frames(y, "y")
        B, H, W = yb.shape[:3]
        j = jpeg_args(jpeg_quality, jpeg_chroma, jpeg_restart)
        cap = jpeg_slot_bytes(H, W, jpeg_chroma, jpeg_restart, jpeg_cap)
        data = torch.empty((B, cap), dtype=torch.uint8, device=yb.device)
        sizes = torch.empty((B,), dtype=torch.int32, device=yb.device)
        for _, nb, p, q, sz in _chunks(B, (yb.data_ptr(), yb.stride(0) * 4), (data.data_ptr(), cap), (sizes.data_ptr(), 4)):
            self._chk(self._lib.rrv_jpeg_encode_device(self._h, p, nb, H, W, C.byref(j), q, cap, sz, self._stream(yb)))
        return data, sizes

    def jpeg_coefficients_tensor(self, streams, *, check=True, return_status=False):
        """The entropy half of the JPEG input stage alone (rrv_jpeg_scan_device; include/rerevst_hip.h "JPEG input"): a list of bytes, one
        baseline JPEG stream per frame, all of one size and chroma format -> the int16 tensor [B][blocks][64] of their coefficient blocks
        (zigzag order, scan order) on the handle's GPU, in stream order.  check: read the statuses back and raise ValueError for a corrupt
        frame; return_status: (coef, int32 [B] status tensor) instead, nothing read back."""
        return self._jpeg_in(streams, False, check, return_status)

    def decode_jpeg_tensor(self, streams, *, check=True, return_status=False):
        """The JPEG input stage alone (rrv_jpeg_decode_device): a list of bytes, one baseline JPEG stream per frame, all of one size and chroma
        format -> (uint8 tensor [B][frame_bytes] of planar frames on the handle's GPU, layout name "i420" | "i422" | "i444") in stream order:
        what transfer_tensor(.., layout=name, size=(H, W)) reads, with rrv_yuv_input_matrix(BT.601, full range) as JFIF's colour space.  A
        grey stream gives an "i444" frame whose chroma planes hold 128.  check / return_status as in jpeg_coefficients_tensor."""
        return self._jpeg_in(streams, True, check, return_status)

    def _jpeg_in(self, streams, planes, check, return_status):
        import torch
        infos, host, cap = _jpeg_streams(streams)
        B, f = len(streams), infos[0]
        dev = torch.device("cuda", self.device)
        d = torch.from_numpy(host).to(dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        if planes:
            hs, vs = (2 if f.chroma in (420, 422) else 1), (2 if f.chroma == 420 else 1)
            step = f.H * f.W + 2 * (-(-f.H // vs)) * (-(-f.W // hs))
            out = torch.empty((B, step), dtype=torch.uint8, device=dev)
        else:
            step = f.blocks * 128
            out = torch.empty((B, f.blocks, 64), dtype=torch.int16, device=dev)
        fn = self._lib.rrv_jpeg_decode_device if planes else self._lib.rrv_jpeg_scan_device
        for b0, nb, p, q, st in _chunks(B, (d.data_ptr(), cap), (out.data_ptr(), step), (status.data_ptr(), 4)):
            sub = (_lib.JpegInfo * nb)(*infos[b0:b0 + nb])
            self._chk(fn(self._h, p, cap, sub, nb, q, st, self._stream(d)))
        if return_status:
            return (out, JPEG_IN_LAYOUTS[f.chroma], status) if planes else (out, status)
        if check:
            _jpeg_statuses(status)
        return (out, JPEG_IN_LAYOUTS[f.chroma]) if planes else out

    def jpeg_planes_tensor(self, coef, streams):
        """The pixel half alone (rrv_jpeg_planes_device): coef an int16 tensor [B][blocks][64] as jpeg_coefficients_tensor returns it for
        `streams` (which give the size and the quantisers) -> (uint8 planes tensor, layout name) as decode_jpeg_tensor returns them."""
        import torch
        infos, _, _ = _jpeg_streams(streams)
        B, f = len(streams), infos[0]
        if not isinstance(coef, torch.Tensor) or coef.dtype != torch.int16 or tuple(coef.shape) != (B, f.blocks, 64):
            raise ValueError("coef must be an int16 tensor [%d][%d][64] for these streams" % (B, f.blocks))
        _on_device(coef, "coef", self.device)
        cb = coef.contiguous()
        hs, vs = (2 if f.chroma in (420, 422) else 1), (2 if f.chroma == 420 else 1)
        step = f.H * f.W + 2 * (-(-f.H // vs)) * (-(-f.W // hs))
        out = torch.empty((B, step), dtype=torch.uint8, device=cb.device)
        for b0, nb, p, q in _chunks(B, (cb.data_ptr(), f.blocks * 128), (out.data_ptr(), step)):
            sub = (_lib.JpegInfo * nb)(*infos[b0:b0 + nb])
            self._chk(self._lib.rrv_jpeg_planes_device(self._h, p, sub, nb, q, self._stream(cb)))
        return out, JPEG_IN_LAYOUTS[f.chroma]

    def _guide_tensor(self, g, name, shape, batched):
        """a guide of deliver_tensor as a contiguous float32 [B,H,W,3] tensor on the handle's GPU"""
        import torch
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.dim() != (4 if batched else 3):
            raise ValueError("%s must be a float32 tensor of y's form (BGR, 'pixel' space)" % name)
        _on_device(g, name, self.device)
        gb = (g if batched else g.unsqueeze(0)).contiguous()
        if tuple(gb.shape) != tuple(shape):
            raise ValueError("%s has shape %s, expected %s" % (name, tuple(gb.shape), tuple(shape)))
        return gb

    def sync(self):
        self._chk(self._lib.rrv_sync(self._h))

    def set_caller_stream(self, stream_ptr, enable=True):
        """Order the *_device entries against the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream):
        they wait for what is queued on it and it waits for their output — no host synchronisation needed."""
        self._chk(self._lib.rrv_set_caller_stream(self._h, C.c_void_p(stream_ptr), 1 if enable else 0))

    def set_f43(self, mode):
        """Kernel choice for the ten layers with a Winograd F(4x4,3x3) pack (rrv_set_f43): 0 never; 1 (default) per layer where
        the launch geometry — frames per launch, frame size, CUs the launch may use — lets it win, so a frame's low-order bits
        depend on how it was submitted (inside the parity bounds either way); 2 always.  With 0 or 2 every entry delivers
        the same bits for a frame."""
        self._chk(self._lib.rrv_set_f43(self._h, int(mode)))

    def set_grid_share(self, share):
        """Persistent grids use 1/share of the CUs (share 1..4): launches of several streams run side by side."""
        self._chk(self._lib.rrv_set_grid_share(self._h, int(share)))

    def debug_tensor(self, slot, index, H, W):
        """Activation tensor `index` of workspace slot `slot` for H x W frames (rrv_debug_copy_tensor), flat float32."""
        n = C.c_size_t(0)
        self._chk(self._lib.rrv_debug_copy_tensor(self._h, int(slot), int(index), int(H), int(W), None, 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        self._chk(self._lib.rrv_debug_copy_tensor(self._h, int(slot), int(index), int(H), int(W), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def debug_tensor_ex(self, slot, index, H, W, image=0):
        """Tensor `index` (0..36: 23..32 the channel-chunk-major twins, 33..36 the four level masks of a masked launch, stride 1,
        2, 4, 8) of image `image` of the last launch on workspace slot `slot` for H x W frames (rrv_debug_copy_tensor_ex):
        (flat float32 as stored, layout 0 NHWC ring / 1 P8, channels)."""
        n, lay, ch = C.c_size_t(0), C.c_int(0), C.c_int(0)
        args = (self._h, int(slot), int(index), int(image), int(H), int(W))
        self._chk(self._lib.rrv_debug_copy_tensor_ex(*args, None, 0, C.byref(n), C.byref(lay), C.byref(ch)))
        out = np.empty(n.value, np.float32)
        self._chk(self._lib.rrv_debug_copy_tensor_ex(*args, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(lay), C.byref(ch)))
        return out, lay.value, ch.value

    def debug_state_set(self, slot, image=0):
        """The state set (get_state's blob layout) of image `image` as the last launch on workspace slot `slot` (0 or 1) wrote it
        (rrv_debug_copy_state): a frame-mode launch's per-image statistics and predicted filters, or a grouped multi-style
        launch's per-image blended state.  Refused when that launch kept no per-image state or did not write the image."""
        out = np.empty(_lib.STATE_FLOATS, dtype=np.float32)
        self._chk(self._lib.rrv_debug_copy_state(self._h, _lib.DBG_STATE_SET, int(slot), int(image), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def debug_style_pred(self, style_id=0):
        """The style half of the filter predictions of a prepared style (rrv_debug_copy_state): float32 [6][32], Filter1.F1 ..
        Filter3.F2."""
        out = np.empty((6, 32), dtype=np.float32)
        self._chk(self._lib.rrv_debug_copy_state(self._h, _lib.DBG_STYLE_PRED, 0, int(style_id), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def debug_style_blob(self, style_id=0):
        """The state blob of a prepared style as it stands, computed or not (rrv_debug_copy_state): after a compute() that
        debug_prep_stop ended early, the entries up to that sync point and the style statistics."""
        out = np.empty(_lib.STATE_FLOATS, dtype=np.float32)
        self._chk(self._lib.rrv_debug_copy_state(self._h, _lib.DBG_STYLE_BLOB, 0, int(style_id), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def debug_prep_stop(self, stage):
        """compute() ends at sync point `stage` (0..13: Decoder.norm[0], Filter1..3, Decoder.norm[1], then norm1 / norm2 / the AdaIN
        norm of each residual block) and keeps its workspace for debug_prep_tensor; -1 switches it off (rrv_debug_prep_stop)."""
        self._chk(self._lib.rrv_debug_prep_stop(self._h, int(stage)))

    def debug_prep_tensor(self, name, image=0):
        """Image `image` of tensor `name` (_lib.PREP_TENSORS) of the preparation pass (rrv_debug_copy_prep_tensor): float32
        [H+2][W+2][C] as stored, ring included."""
        idx = _lib.PREP_TENSORS.index(name)
        n, H, W, Ch = C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_int(0)
        tail = (C.byref(n), C.byref(H), C.byref(W), C.byref(Ch))
        self._chk(self._lib.rrv_debug_copy_prep_tensor(self._h, idx, int(image), None, 0, *tail))
        out = np.empty(n.value, np.float32)
        self._chk(self._lib.rrv_debug_copy_prep_tensor(self._h, idx, int(image), out.ctypes.data_as(C.c_void_p), n.value, *tail))
        return out.reshape(H.value + 2, W.value + 2, Ch.value)

    def debug_weights(self):
        """Every weight buffer the handle holds in HBM, in the library's order (rrv_debug_weight_count / _info): yields
        (info, read) with info = {"key", "form" (_lib.WEIGHT_FORMS), "Cout", "Cin", "taps", "BN", "sets", "floats"} and read(set=0)
        the buffer of that state set as flat float32 (rrv_debug_copy_weights; `sets` > 1: the folded KernelFilter weights, refused
        for a set nothing has folded)."""
        count = self._lib.rrv_debug_weight_count(self._h)
        if count < 0:
            self._chk(count)
        for i in range(count):
            key = C.create_string_buffer(128)
            form, cout, cin, taps, bn, sets, n = [C.c_int(0) for _ in range(6)] + [C.c_size_t(0)]
            self._chk(self._lib.rrv_debug_weight_info(self._h, i, key, len(key), C.byref(form), C.byref(cout), C.byref(cin), C.byref(taps), C.byref(bn),
                                                      C.byref(sets), C.byref(n)))
            info = {"key": key.value.decode(), "form": _lib.WEIGHT_FORMS[form.value], "Cout": cout.value, "Cin": cin.value, "taps": taps.value,
                    "BN": bn.value, "sets": sets.value, "floats": n.value}

            def read(set=0, i=i, floats=n.value):
                out, got = np.empty(floats, np.float32), C.c_size_t(0)
                self._chk(self._lib.rrv_debug_copy_weights(self._h, i, int(set), out.ctypes.data_as(C.c_void_p), out.size, C.byref(got)))
                assert got.value == floats
                return out
            yield info, read

    def _set_matrix(self, set8, set16, matrix_of, input_side, standard, full_range, bits):
        """set_yuv_matrix / set_yuv_input_matrix: the side's 8-bit or uint16 setter, its depth, and matrix_of(standard, full_range, bits)"""
        bits = _yuv_depth(bits)
        setter = set8 if bits == 8 else set16
        if bits > 8:
            self._chk(self._lib.rrv_set_yuv_depth(self._h, bits if input_side else 0, 0 if input_side else bits))
        if standard is None:
            self._chk(setter(self._h, None))
            return matrix_of("bt601", False, bits)
        m = matrix_of(standard, full_range, bits) if isinstance(standard, str) else np.ascontiguousarray(standard, dtype=np.float32).reshape(-1)
        if m.size != 12:
            raise ValueError("a YUV matrix has 12 coefficients, got %d" % m.size)
        self._chk(setter(self._h, m.ctypes.data_as(C.POINTER(C.c_float))))
        return m.reshape(3, 4).copy()

    def set_yuv_matrix(self, standard="bt601", full_range=False, bits=8):
        """The conversion matrix of the "i420" / "nv12" outputs (rrv_set_yuv_matrix): a standard ("bt601" | "bt709") and range, or
        twelve finite floats ([3][4]: rows Y, Cb, Cr; columns R, G, B, offset) in place of `standard`; None restores the default,
        BT.601 limited range.  Read when a call launches; returns the float32 [3][4] matrix now installed.
        bits = 10, 12, 16: the matrix of the uint16 outputs instead ("i420p10", "p010", ..: rrv_set_yuv16_matrix, independent of the
        8-bit one), installed together with that output depth (rrv_set_yuv_depth); None: BT.601 limited range at the depth in force
        when a call launches."""
        return self._set_matrix(self._lib.rrv_set_yuv_matrix, self._lib.rrv_set_yuv16_matrix, yuv_matrix, False, standard, full_range, bits)

    def set_yuv_input_matrix(self, standard="bt601", full_range=False, bits=8):
        """The conversion matrix of the "i420" / "nv12" INPUTS (rrv_set_yuv_input_matrix): a standard ("bt601" | "bt709") and range,
        or twelve finite floats ([3][4]: rows R, G, B; columns Y, Cb, Cr, offset) in place of `standard`; None restores the default,
        BT.601 limited range.  Independent of set_yuv_matrix; read when a call launches its first kernel.  Returns the float32
        [3][4] matrix now installed.
        bits = 10, 12, 16: the matrix of the uint16 inputs instead (rrv_set_yuv16_input_matrix), installed together with that input
        depth; None: BT.601 limited range at the depth in force when a call launches."""
        return self._set_matrix(self._lib.rrv_set_yuv_input_matrix, self._lib.rrv_set_yuv16_input_matrix, yuv_input_matrix, True, standard, full_range, bits)

    def set_host_io(self, mode):
        """0 (default): staged H2D / D2H copies; 1: zero copy — kernels read / write page-locked host memory directly."""
        self._chk(self._lib.rrv_set_host_io(self._h, int(mode)))

    def set_pipeline(self, n_slots):
        """1: every device-entry call runs on one stream; 2 (default): consecutive calls alternate over two
        (stream, workspace) pairs so two independent batches are in flight."""
        self._chk(self._lib.rrv_set_pipeline(self._h, int(n_slots)))

    # ===== shared state (RCCL broadcast payload / golden comparison) =====
    def get_state(self, style_id=0):
        out = np.empty(_lib.STATE_FLOATS, dtype=np.float32)
        self._chk(self._lib.rrv_get_state(self._h, out.ctypes.data_as(C.c_void_p), out.size, style_id))
        return out

    def set_state(self, blob, style_id=0):
        b = np.ascontiguousarray(blob, dtype=np.float32).reshape(-1)
        if b.size != _lib.STATE_FLOATS:
            raise ValueError("state blob must have %d floats" % _lib.STATE_FLOATS)
        self._chk(self._lib.rrv_set_state(self._h, b.ctypes.data_as(C.c_void_p), b.size, style_id))

    # ===== the path's one collective through the C ABI (RCCL; rerevst_hip.h: rrv_comm_*, rrv_broadcast_state) =====
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        if self._lib.rrv_comm_unique_id(buf) != 0:
            raise RRVError("rrv_comm_unique_id failed (librccl.so not found? set RRV_RCCL_PATH)")
        return bytes(buf.raw)

    def comm_init_rank(self, unique_id, nranks, rank):
        comm = C.c_void_p()
        self._chk(self._lib.rrv_comm_init_rank(self._h, C.create_string_buffer(bytes(unique_id), 128), int(nranks), int(rank), C.byref(comm)))
        return comm

    def comm_destroy(self, comm):
        if self._lib.rrv_comm_destroy(comm) != 0:
            raise RRVError("rrv_comm_destroy failed")

    def broadcast_state(self, comm, root, rank, style_id=0):
        """ncclBroadcast of the style's 17 536-float state from `root`; afterwards this rank holds it as after set_state."""
        self._chk(self._lib.rrv_broadcast_state(self._h, comm, int(root), int(rank), int(style_id)))

    def preclamp(self, H, W, image=0):
        """Pre-clamp network output of the last transfer (image `image` of its last launch), NHWC RGB normalised units."""
        out = _outputs.empty((H, W, 3))
        self._chk(self._lib.rrv_get_preclamp_image(self._h, out.ctypes.data_as(C.c_void_p), H, W, int(image)))
        return out

    # ===== per-launch timing (HIP events on the library's stream) =====
    def profile_begin(self):
        self._chk(self._lib.rrv_profile_begin(self._h))

    def profile_end(self):
        self._chk(self._lib.rrv_profile_end(self._h))
        n = self._lib.rrv_profile_count(self._h)
        rows = []
        name, ms, fl, by, fx = C.c_char_p(), C.c_float(), C.c_double(), C.c_double(), C.c_double()
        for i in range(n):
            self._chk(self._lib.rrv_profile_entry(self._h, i, C.byref(name), C.byref(ms), C.byref(fl), C.byref(by), C.byref(fx)))
            rows.append((name.value.decode(), ms.value, fl.value, by.value, fx.value))
        return rows

    def profile_grids(self):
        """After profile_end(): one (grid.x, xcd_slabs) per row of its log (rrv_profile_entry_grid).  The persistent kernels
        report the grid they were launched with; xcd_slabs is 1 / 0 for the two item walks of a transform-domain launch and -1
        for a launch that has none; every other launch reports (0, -1)."""
        g, x = C.c_uint(0), C.c_int(0)
        out = []
        for i in range(self._lib.rrv_profile_count(self._h)):
            self._chk(self._lib.rrv_profile_entry_grid(self._h, i, C.byref(g), C.byref(x)))
            out.append((g.value, x.value))
        return out


class ContentFeature():
    """Handle to an encoder output cached in HBM (what the reference stores as cache/%d.pt)."""

    def __init__(self, fid, shape):
        self.id, self.shape = fid, shape


class MultiStyleStylization(Stylization):
    """Mirror of "Multi-style Interpolation/stylization.py":42-100: ``Stylization(checkpoint, cuda, style_num)``
    with ``prepare_style(list)``, ``generate_content_features(img)``, ``add_patch(feature)``,
    ``compute_norm()``, ``clean()`` and ``transfer(feature, style_weight)``."""

    def __init__(self, checkpoint="", cuda=True, style_num=1, device=None):
        super().__init__(checkpoint, cuda=cuda, use_Global=True, device=device, style_num=style_num)

    def generate_content_features(self, content):
        a = _u8_image(content, "content")
        fid = C.c_int(-1)
        self._chk(self._lib.rrv_generate_content_features(self._h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1], C.byref(fid)))
        return ContentFeature(fid.value, a.shape)

    def generate_content_features_batch(self, frames):
        """`generate_content_features` for a run of equally sized frames (a list, or one [B][H][W][3] array) in one call:
        the reference's caching loop ("Multi-style Interpolation/test.py":87-101) pipelined inside the library
        (rrv_generate_content_features_batch).  Returns one ContentFeature per frame."""
        a = _u8_frames(frames, "content")
        B, H, W, _ = a.shape
        ids = (C.c_int * B)()
        self._chk(self._lib.rrv_generate_content_features_batch(self._h, a.ctypes.data_as(C.c_void_p), B, H, W, ids))
        return [ContentFeature(int(i), (H, W, 3)) for i in ids]

    def add_patch(self, patch_feature):
        self._chk(self._lib.rrv_add_patch(self._h, patch_feature.id))

    def compute_norm(self):
        self.compute()

    def transfer(self, cur_feature, style_weight=[1.], out=None, dtype=np.float32):
        """`out` / `dtype`: float32 (default) or uint8 output, as Stylization.transfer_batch."""
        out, u8 = _output((*_stylized_size(*cur_feature.shape[:2]), 3), dtype, out)
        w = (C.c_float * len(style_weight))(*[float(v) for v in style_weight])
        fn = self._entry("rrv_transfer_features", u8)
        self._chk(fn(self._h, cur_feature.id, w, len(style_weight), out.ctypes.data_as(C.c_void_p)))
        return out

    def transfer_many(self, features, style_weights, out=None, dtype=np.float32):
        """`transfer` for a run of cached features, one weight vector each, pipelined inside the library
        (rrv_transfer_features_batch).  Returns / fills a float32 (or, by `out` / `dtype`, uint8) [n][H][W][3] array."""
        n = len(features)
        ns = len(style_weights[0])
        out, u8 = _output((n, *_stylized_size(*features[0].shape[:2]), 3), dtype, out)
        ids = (C.c_int * n)(*[f.id for f in features])
        w = (C.c_float * (n * ns))(*[float(v) for row in style_weights for v in row])
        self._chk(self._entry("rrv_transfer_features_batch", u8)(self._h, ids, w, n, ns, out.ctypes.data_as(C.c_void_p)))
        return out

    def release_features(self):
        self._chk(self._lib.rrv_release_features(self._h))

    def set_multistyle_group(self, frames):
        """Frames per launch sequence of transfer_many (1..16; 0 = by the frame size, the default): per-image blended state inside one launch."""
        self._chk(self._lib.rrv_set_multistyle_group(self._h, int(frames)))

    def set_feature_cache_cap(self, nbytes):
        """Features are cached in HBM up to `nbytes` (default 64 GiB); beyond that a frame is kept as uint8 pixels and
        re-encoded at every use (the reference's cache is on disk: "Multi-style Interpolation/test.py":87-101)."""
        self._chk(self._lib.rrv_set_feature_cache_cap(self._h, int(nbytes)))

    def feature_cache_info(self):
        """(cached features, spilled features, bytes held by the cached ones)."""
        r, sp, b = C.c_int(), C.c_int(), C.c_size_t()
        self._chk(self._lib.rrv_feature_cache_info(self._h, C.byref(r), C.byref(sp), C.byref(b)))
        return r.value, sp.value, b.value

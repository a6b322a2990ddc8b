"""What the Python binding does with a call, pinned without a GPU: every public tensor / host method of framework.Stylization is driven
with a recording stand-in for the library, and what it records — the C entries reached, in order, with every argument, and what comes
back or is raised — is compared with tests/call_record.json, entry for entry (the file keeps a digest of each call sequence, the
entries it reaches and the result or refusal text in full: "the fixture" below).

The stand-in records every entry but rrv_image_view_check and rrv_image_view_contiguous, which it forwards to the real library (they
need no GPU and are not part of what a call hands to the GPU).  A scalar is recorded as it is, an rrv_image_desc as
"d:dtype/layout/space", an rrv_image_view as "v:dtype/layout/space/frame_stride/plane offsets/pitches", and a pointer as the buffer it
falls in plus a byte offset: "x" ("x0", "x1", .. of a list), "out" (the caller's, or the fresh result), "w" (style_weights), "m" (style_masks), "stream", "h" (the
handle), or "tmpK": a buffer the binding made itself (a contiguous copy, broadcast weights), named by the argument position K it is
passed at, the offset counted from its first use.  The result is "out" (the caller's own object) or the shape and dtype of the fresh
array / tensor, and for a refused call the exception's type and text.

The "GPU" tensors are CPU tensors of a subclass that reports cuda:0; inside record() only, torch.cuda.current_stream is stubbed, fresh
torch outputs are allocated on the CPU, Tensor.to(a cuda device) keeps the memory where it is, and the page-locked allocator refuses (so
host outputs are plain numpy arrays).

    python tests/test_call_record.py --write [--framework FILE]

writes the fixture.  FILE is another framework.py to record (it is loaded inside the package, so its relative imports resolve): the
committed fixture was written from the framework.py of the commit before the binding was refactored,

    git show <that commit>:rerevst-code_amd/framework.py > /tmp/framework_before.py
    python tests/test_call_record.py --write --framework /tmp/framework_before.py

and that command reproduces its bytes.
"""
import ctypes as C
import importlib
import importlib.util
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "call_record.json")
PKG = "rerevst-code_amd"
STREAM, HANDLE = 0x57AEA000, 0x4A4D1E00      # sentinels no buffer lies at
FORWARDED = ("rrv_image_view_check", "rrv_image_view_contiguous")

torch = pytest.importorskip("torch")
L = importlib.import_module(PKG + "._lib")
VIDEO = importlib.import_module(PKG + ".video")


class OnGpu(torch.Tensor):
    """a CPU tensor that reports cuda:0; slices, copies and reshapes of it do too"""
    device = property(lambda self: torch.device("cuda", 0))


def gpu(t):
    return t.as_subclass(OnGpu)


class Recorder:
    """stands in for the library: records every entry and answers 0; the two view helpers go to the real library"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in FORWARDED:
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _region(obj):
    """(address, bytes) of the whole buffer behind a tensor, an ImageView or an array; None for anything else"""
    if not isinstance(obj, torch.Tensor) and hasattr(obj, "storage") and hasattr(obj, "frames"):         # framework.ImageView
        obj = obj.storage
    if isinstance(obj, torch.Tensor):
        st = obj.untyped_storage()
        return st.data_ptr(), st.nbytes()
    if isinstance(obj, np.ndarray):
        while isinstance(obj.base, np.ndarray):
            obj = obj.base
        return obj.ctypes.data, obj.nbytes
    return None


def _view(v):
    return "v:%d/%d/%d/%d/%s/%s" % (v.desc.dtype, v.desc.layout, v.desc.space, v.frame_stride, ",".join(str(o) for o in v.plane_offset),
                                    ",".join(str(p) for p in v.pitch))


class _Pointers:
    """names a pointer by the buffer it falls in"""

    def __init__(self, regions):
        self.regions, self.tmp = [(n, r) for n, r in regions if r is not None], {}

    def name(self, addr, pos):
        if addr is None:
            return "null"
        if addr == STREAM:
            return "stream"
        if addr == HANDLE:
            return "h"
        for n, (base, size) in self.regions:
            if base <= addr < base + max(size, 1):
                return "%s+%d" % (n, addr - base)
        return "tmp%d+%d" % (pos, addr - self.tmp.setdefault(pos, addr))


def _arg(a, pos, ptrs):
    if isinstance(a, L.ImageDesc):
        return "d:%d/%d/%d" % (a.dtype, a.layout, a.space)
    if isinstance(a, L.ImageView):
        return _view(a)
    if type(a).__name__ == "CArgObject":             # C.byref(view)
        return _view(a._obj) if isinstance(a._obj, L.ImageView) else "ref:" + type(a._obj).__name__
    if isinstance(a, C.c_void_p):
        return ptrs.name(a.value, pos)
    if isinstance(a, C._Pointer):                     # array.ctypes.data_as(POINTER(c_float))
        return ptrs.name(C.cast(a, C.c_void_p).value, pos)
    if a is None:
        return "null"
    if isinstance(a, (bool, int, np.integer)):
        return int(a)
    if isinstance(a, float):
        return a
    return "?" + type(a).__name__


def _result(r, out):
    if r is None:
        return None
    if out is not None and r is out:
        return "out"
    if isinstance(r, torch.Tensor):
        return "tensor %s %s" % (list(r.shape), str(r.dtype).replace("torch.", ""))
    if isinstance(r, np.ndarray):
        return "array %s %s" % (list(r.shape), r.dtype.name)
    return "?" + type(r).__name__


class Session:
    """one framework module under the fakes"""

    def __init__(self, F, mp):
        self.F, self.real = F, L.load()
        mp.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": STREAM})())
        empty = torch.empty
        mp.setattr(torch, "empty", lambda *a, device=None, **kw: gpu(empty(*a, **kw)))
        to = torch.Tensor.to
        mp.setattr(torch.Tensor, "to", lambda t, *a, **kw: gpu(t) if a and isinstance(a[0], torch.device) and a[0].type == "cuda" else to(t, *a, **kw))
        mp.setattr(self.real, "rrv_host_alloc", lambda n, p: -1)

    def handle(self, use_Global=True):
        s = self.F.Stylization.__new__(self.F.Stylization)
        s.device, s.style_num, s.use_Global, s._open = 0, 4, use_Global, {}
        s._lib, s._h = Recorder(self.real), C.c_void_p(HANDLE)
        return s

    def record(self, method, x, *args, use_Global=True, **kw):
        """{"calls": [...], "result": ..} or {"calls": [...], "raises": "Type: text"} of Stylization.method(x, *args, **kw)"""
        s = self.handle(use_Global)
        out, res, err = kw.get("out"), None, None
        try:
            res = getattr(s, method)(x, *args, **kw)
        except Exception as e:      # noqa: BLE001  (whatever is raised is the record)
            err = "%s: %s" % (type(e).__name__, e)
        calls, s._h = s._lib.calls, None
        regions = [("x%d" % i, _region(v)) for i, v in enumerate(x)] if isinstance(x, (list, tuple)) else [("x", _region(x))]
        regions += [("out", _region(out if out is not None else res)), ("w", _region(kw.get("style_weights"))), ("m", _region(kw.get("style_masks")))]
        ptrs = _Pointers(regions)
        rec = {"calls": ["%s(%s)" % (name, ",".join(str(_arg(a, i, ptrs)) for i, a in enumerate(a_))) for name, a_ in calls]}
        if err is not None:
            rec["raises"] = err
        else:
            rec["result"] = _result(res, out)
        return rec


# ---------------------------------------------------------------- inputs and outputs of the cases
BH, BW = 24, 40          # the batch geometry (8*(H//8) x 8*(W//8) is the frame itself)
OH, OW = 37, 51          # the pad_crop geometry
WORK, DELIVER = (16, 24), (29, 45)
SCALINGS = {"plain": {}, "work": {"work_size": WORK}, "deliver": {"out_size": DELIVER}, "both": {"work_size": WORK, "out_size": DELIVER},
            "source": {"out_size": "source"}}


def fb(fmt, H, W):
    return VIDEO.yuv_frame_bytes(H, W, chroma=VIDEO.YUV_FORMATS[fmt].chroma)


def planes(layout, H, W):
    """[(row length, rows)] of an H x W frame's planes, in elements"""
    if layout == "nhwc":
        return [(3 * W, H)]
    if layout == "nchw":
        return [(W, H)] * 3
    CH, CW = VIDEO.chroma_plane_size(H, W, VIDEO.YUV_FORMATS[layout].chroma)
    return [(W, H), (CW, CH), (CW, CH)] if VIDEO.YUV_FORMATS[layout].planar else [(W, H), (2 * CW, CH)]


def np_dtype(layout, f32=True):
    if layout in VIDEO.YUV_FORMATS:
        return VIDEO.YUV_FORMATS[layout].dtype
    return np.dtype(np.float32 if f32 else np.uint8)


def tensor(shape, dtype):
    return gpu(torch.from_numpy(np.zeros(shape, dtype)))


def surface(F, layout, B, H, W, pad=5, f32=True, **kw):
    """an ImageView of B pitched H x W frames in `layout`: every row `pad` elements longer than it needs, 3 spare rows between frames"""
    pl = planes(layout, H, W)
    pitch = [ln + pad for ln, _ in pl]
    frame = sum(p * rows for p, (_, rows) in zip(pitch, pl)) + 3 * pitch[0]
    return F.ImageView(tensor((B * frame,), np_dtype(layout, f32)), layout, (H, W), pitch, frame_stride=frame, frames=B, **kw)


def packed(layout, B, H, W, f32=True, batched=True):
    shape = (B, fb(layout, H, W)) if layout in VIDEO.YUV_FORMATS else (B, 3, H, W) if layout == "nchw" else (B, H, W, 3)
    t = tensor(shape, np_dtype(layout, f32))
    return t if batched else t[0]


def window(layout, B, H, W, f32=True, batched=True):
    """B x H x W frames inside a larger canvas; a YUV layout has no window: every second frame of a buffer (refused as an output)"""
    if layout in VIDEO.YUV_FORMATS:
        t = tensor((2 * B, fb(layout, H, W)), np_dtype(layout))[::2]
    elif layout == "nchw":
        t = tensor((B, 3, H + 9, W + 7), np_dtype(layout, f32))[:, :, 3:3 + H, 2:2 + W]
    else:
        t = tensor((B, H + 9, W + 7, 3), np_dtype(layout, f32))[:, 3:3 + H, 2:2 + W]
    return t if batched else t[0]


def source(F, kind, B, H, W, batched=True):
    """(x, keywords) of the input kinds of the tensor entries"""
    if kind == "f32nchw":
        return packed("nchw", B, H, W, batched=batched), {}
    if kind == "u8nhwc":
        return packed("nhwc", B, H, W, f32=False, batched=batched), {"layout": "nhwc"}
    if kind == "crop":
        return window("nchw", B, H, W, batched=batched), {}
    if kind == "copied":        # NHWC memory under an NCHW shape fits no view
        t = packed("nchw", B, H, W).to(memory_format=torch.channels_last)
        return (t if batched else t[0]), {}
    if kind == "nv12":
        return packed("nv12", B, H, W, batched=batched), {"layout": "nv12", "size": (H, W)}
    if kind == "nv12view":
        return surface(F, "nv12", B, H, W), {}
    raise KeyError(kind)


SOURCES = ("f32nchw", "u8nhwc", "crop", "copied", "nv12", "nv12view")
SOURCE_LAYOUT = {"f32nchw": "nchw", "u8nhwc": "nhwc", "crop": "nchw", "copied": "nchw", "nv12": "nv12", "nv12view": "nv12"}


def target(F, kind, layout, B, H, W, f32=True, batched=True):
    if kind == "fresh":
        return None
    if kind == "tensor":
        return packed(layout, B, H, W, f32, batched)
    if kind == "window":
        return window(layout, B, H, W, f32, batched)
    if kind == "view":
        return surface(F, layout, B, H, W, f32=f32)
    raise KeyError(kind)


TARGETS = ("fresh", "tensor", "window", "view")


def out_hw(H, W, pad_crop, scaling):
    kw = SCALINGS[scaling]
    if "out_size" in kw:
        return (H, W) if kw["out_size"] == "source" else kw["out_size"]
    if "work_size" in kw:
        H, W = kw["work_size"]
    return (H, W) if pad_crop else (H // 8 * 8, W // 8 * 8)


def host_frames(in_format, B, H, W):
    if in_format == "bgr":
        return np.zeros((B, H, W, 3), np.uint8), {}
    return np.zeros((B, fb(in_format, H, W)), VIDEO.YUV_FORMATS[in_format].dtype), {"in_format": in_format, "size": (H, W)}


HOST_OUTPUTS = {"f32": {}, "u8": {"dtype": np.uint8}, "i420": {"out_format": "i420"}, "p210": {"out_format": "p210"}}


def host_styles(kind, B, H, W):
    if kind == "w_bs":
        return {"style_weights": np.full((B, 2), 0.5, np.float32)}
    if kind == "w_s":
        return {"style_weights": [0.25, 0.75]}
    if kind == "m_bshw":
        return {"style_masks": np.full((B, 2, H, W), 0.5, np.float32)}
    if kind == "m_shw":
        return {"style_masks": np.full((3, H, W), 0.25, np.float32)}
    return {}


STYLES = ("none", "w_bs", "w_s", "m_bshw", "m_shw")


# ---------------------------------------------------------------- the case groups: each yields (id, record)
def host_cases(S):
    for method, (H, W) in (("transfer_batch", (BH, BW)), ("transfer_frames", (OH, OW))):
        for inf, (oname, okw), st, (sname, skw), glob in itertools.product(("bgr", "nv12", "i422p10"), HOST_OUTPUTS.items(), STYLES, SCALINGS.items(),
                                                                              (True, False)):
            frames, ikw = host_frames(inf, 2, H, W)
            yield ("%s %s>%s %s %s %s" % (method, inf, oname, st, sname, "global" if glob else "frame"),
                   S.record(method, frames, use_Global=glob, **ikw, **okw, **host_styles(st, 2, H, W), **skw))
    # a list of frames, the caller's own output array, a batch above one chunk, and the checks of the host side
    frames, _ = host_frames("bgr", 2, BH, BW)
    yield "transfer_batch list", S.record("transfer_batch", [frames[0], frames[1]])
    yield "transfer_batch out f32", S.record("transfer_batch", frames, out=np.zeros((2, BH, BW, 3), np.float32))
    yield "transfer_batch out u8", S.record("transfer_batch", frames, out=np.zeros((2, BH, BW, 3), np.uint8), style_weights=[1.0])
    yield "transfer_frames out nv12 deliver", S.record("transfer_frames", frames, out=np.zeros((2, fb("nv12", *DELIVER)), np.uint8), out_format="nv12",
                                                       out_size=DELIVER)
    yield "transfer_batch out wrong shape", S.record("transfer_batch", frames, out=np.zeros((2, BH, BW + 8, 3), np.float32))
    yield "transfer_batch out wrong dtype", S.record("transfer_batch", frames, out=np.zeros((2, fb("p010", BH, BW)), np.uint8), out_format="p010")
    yield "transfer_batch bad dtype", S.record("transfer_batch", frames, dtype=np.float16)
    yield "transfer_batch bad out_format", S.record("transfer_batch", frames, out_format="rgb")
    yield "transfer_batch bad in_format", S.record("transfer_batch", frames, in_format="yuv", size=(BH, BW))
    yield "transfer_batch no size", S.record("transfer_batch", np.zeros((2, fb("nv12", BH, BW)), np.uint8), in_format="nv12")
    yield "transfer_batch wrong samples", S.record("transfer_batch", np.zeros((2, fb("nv12", BH, BW) + 1), np.uint8), in_format="nv12", size=(BH, BW))
    yield "transfer_batch float frames", S.record("transfer_batch", np.zeros((2, BH, BW, 3), np.float32))
    yield "transfer_batch bad work_size", S.record("transfer_batch", frames, work_size=(0, 8))
    yield "transfer_batch bad out_size", S.record("transfer_batch", frames, out_size="frame")
    yield "transfer_batch five styles", S.record("transfer_batch", frames, style_weights=np.ones((2, 5), np.float32))
    yield "transfer_batch mask size", S.record("transfer_batch", frames, style_masks=np.ones((2, 2, BH, BW + 1), np.float32))
    yield "transfer_batch mask dtype", S.record("transfer_batch", frames, style_masks=np.ones((2, 2, BH, BW), np.float64))
    p010, ikw = host_frames("p010", 2, BH, BW)        # calls wrong in two ways: which of the two is reported, and what reached the library before
    yield "transfer_batch p010 five styles", S.record("transfer_batch", p010, style_weights=np.ones((2, 5), np.float32), **ikw)
    yield "transfer_batch p010 five masks", S.record("transfer_batch", p010, style_masks=np.ones((2, 5, BH, BW), np.float32), **ikw)
    yield "transfer_batch bad out_format and float frames", S.record("transfer_batch", np.zeros((2, BH, BW, 3), np.float32), out_format="rgb")
    yield "transfer_batch bad work_size and out_size", S.record("transfer_batch", frames, work_size=(0, 8), out_size="frame")
    yield "transfer_batch wrong out and bad work_size", S.record("transfer_batch", frames, out=np.zeros((2, BH, BW + 8, 3), np.float32), work_size=(0, 8))
    yield "transfer_batch wrong out and five masks", S.record("transfer_batch", frames, out=np.zeros((2, BH, BW + 8, 3), np.float32),
                                                              style_masks=np.ones((2, 5, BH, BW), np.float32))
    yield "transfer_batch 65", S.record("transfer_batch", np.zeros((65, 8, 8, 3), np.uint8))


def add_cases(S):
    patch = np.zeros((OH, OW, 3), np.uint8)
    one, two = np.zeros(fb("nv12", OH, OW), np.uint8), np.zeros((2, fb("p010", OH, OW)), np.uint16)
    yield "add bgr", S.record("add", patch)
    yield "add nv12", S.record("add", one, in_format="nv12", size=(OH, OW))
    yield "add p010 x2", S.record("add", two, in_format="p010", size=(OH, OW))
    yield "add bgr work", S.record("add", patch, work_size=WORK)
    yield "add nv12 work", S.record("add", one, in_format="nv12", size=(OH, OW), work_size=WORK)
    yield "add p010 x2 work", S.record("add", two, in_format="p010", size=(OH, OW), work_size=WORK)
    yield "add frame mode", S.record("add", patch, use_Global=False)
    yield "add no size", S.record("add", one, in_format="nv12")
    yield "add gray", S.record("add", np.zeros((OH, OW), np.uint8))
    yield "add bad work_size", S.record("add", patch, work_size=(8,))


def tensor_styles(kind, B, H, W):
    if kind == "w_host_bs":
        return {"style_weights": np.full((B, 2), 0.5, np.float32)}
    if kind == "w_host_s":
        return {"style_weights": [0.25, 0.75]}
    if kind == "w_dev_bs":
        return {"style_weights": tensor((B, 2), np.float32)}
    if kind == "w_dev_s":
        return {"style_weights": tensor((3,), np.float32)}
    if kind == "m_dev_bshw":
        return {"style_masks": tensor((B, 2, H, W), np.float32)}
    if kind == "m_dev_shw":
        return {"style_masks": tensor((2, H, W), np.float32)}
    if kind == "m_host_bshw":
        return {"style_masks": np.full((B, 2, H, W), 0.5, np.float32)}
    if kind == "m_host_shw":
        return {"style_masks": np.full((2, H, W), 0.5, np.float32)}
    return {}


TENSOR_STYLES = ("w_host_bs", "w_host_s", "w_dev_bs", "w_dev_s", "m_dev_bshw", "m_dev_shw", "m_host_bshw", "m_host_shw")


def transfer_tensor_cases(S):
    F = S.F
    # every source into every kind of output, both geometries, every scaling; out_layout left to default
    for src, tgt, pad_crop, scaling in itertools.product(SOURCES, TARGETS, (False, True), SCALINGS):
        H, W = (OH, OW) if pad_crop else (BH, BW)
        x, kw = source(F, src, 2, H, W)
        lay = SOURCE_LAYOUT[src]
        out = target(F, tgt, lay, 2, *out_hw(H, W, pad_crop, scaling))
        yield ("transfer_tensor %s>%s %s %s" % (src, tgt, "frames" if pad_crop else "batch", scaling),
               S.record("transfer_tensor", x, out=out, pad_crop=pad_crop, **kw, **SCALINGS[scaling]))
    # out_layout / out_dtype / out_space set, a YUV name included; an output given in another layout than the input's
    for src, olay, scaling in itertools.product(SOURCES, ("nchw", "nhwc", "nv12", "p010", "i444"), ("plain", "work", "both")):
        x, kw = source(F, src, 2, OH, OW)
        yield "transfer_tensor %s out_layout=%s %s" % (src, olay, scaling), S.record("transfer_tensor", x, out_layout=olay, pad_crop=True, **kw, **SCALINGS[scaling])
        if scaling != "work":
            out = target(F, "view" if olay != "nhwc" else "window", olay, 2, *out_hw(OH, OW, True, scaling), f32=False)
            yield ("transfer_tensor %s out_layout=%s given %s" % (src, olay, scaling),
                   S.record("transfer_tensor", x, out_layout=olay, out=out, pad_crop=True, **kw, **SCALINGS[scaling]))
            yield ("transfer_tensor %s layout of out %s %s" % (src, olay, scaling),       # the view names the layout; a tensor does not
                   S.record("transfer_tensor", x, out=out, pad_crop=True, **kw, **SCALINGS[scaling]))
    for src, scaling in itertools.product(SOURCES, ("plain", "deliver")):
        x, kw = source(F, src, 2, BH, BW)
        yield "transfer_tensor %s u8 unit %s" % (src, scaling), S.record("transfer_tensor", x, out_dtype=torch.uint8, out_layout="nhwc", **kw, **SCALINGS[scaling])
        yield "transfer_tensor %s out_space=unit %s" % (src, scaling), S.record("transfer_tensor", x, out_space="unit", out_layout="nchw", **kw, **SCALINGS[scaling])
        yield "transfer_tensor %s frame mode %s" % (src, scaling), S.record("transfer_tensor", x, use_Global=False, **kw, **SCALINGS[scaling])
    x, kw = source(F, "f32nchw", 2, BH, BW)
    yield "transfer_tensor norm in and out", S.record("transfer_tensor", x, space="norm", out_space="norm")
    yield "transfer_tensor norm view out", S.record("transfer_tensor", x, space="unit", out_space="norm", out=surface(F, "nchw", 2, BH, BW))
    # unbatched, and batches above one chunk of 64 (8 x 8 frames)
    for src, tgt, scaling in itertools.product(SOURCES, ("fresh", "window"), ("plain", "both")):
        if src != "nv12view":
            x, kw = source(F, src, 1, BH, BW, batched=False)
            out = target(F, tgt, SOURCE_LAYOUT[src], 1, *out_hw(BH, BW, False, scaling), batched=False)
            yield "transfer_tensor %s>%s unbatched %s" % (src, tgt, scaling), S.record("transfer_tensor", x, out=out, **kw, **SCALINGS[scaling])
        x, kw = source(F, src, 65, 8, 8)
        skw = {} if scaling == "plain" else {"work_size": (16, 16), "out_size": (8, 8)}
        out = target(F, tgt, SOURCE_LAYOUT[src], 65, 8, 8)
        yield "transfer_tensor %s>%s 65 %s" % (src, tgt, scaling), S.record("transfer_tensor", x, out=out, **kw, **skw)
    x, kw = source(F, "u8nhwc", 65, 8, 8)
    yield "transfer_tensor u8nhwc>view 65", S.record("transfer_tensor", x, out=surface(F, "nhwc", 65, 8, 8), **kw)
    # weights and masks, host and device, whole and broadcast, one chunk and two
    for src, st, tgt in itertools.product(("f32nchw", "crop", "copied", "nv12", "nv12view"), TENSOR_STYLES, ("fresh", "window")):
        x, kw = source(F, src, 2, OH, OW)
        out = target(F, tgt, SOURCE_LAYOUT[src], 2, OH, OW)
        yield "transfer_tensor %s>%s %s" % (src, tgt, st), S.record("transfer_tensor", x, out=out, pad_crop=True, **kw, **tensor_styles(st, 2, OH, OW))
        if tgt == "fresh":
            x, kw = source(F, src, 65, 8, 8)
            yield "transfer_tensor %s 65 %s" % (src, st), S.record("transfer_tensor", x, **kw, **tensor_styles(st, 65, 8, 8))


def other_cases(S):
    F = S.F
    for src in SOURCES:
        for name, B, H, W, batched in (("", 2, OH, OW, True), (" unbatched", 1, OH, OW, False), (" 65", 65, 8, 8, True)):
            if not batched and src == "nv12view":
                continue
            x, kw = source(F, src, B, H, W, batched=batched)
            yield "resample_tensor %s%s" % (src, name), S.record("resample_tensor", x, WORK, **kw)
            yield "add_tensor %s%s" % (src, name), S.record("add_tensor", x, **kw)
            yield "add_tensor %s%s work" % (src, name), S.record("add_tensor", x, work_size=WORK, **kw)
    x, kw = source(F, "f32nchw", 2, OH, OW)
    yield "resample_tensor norm", S.record("resample_tensor", x, WORK, space="norm")
    yield "resample_tensor bad work_size", S.record("resample_tensor", x, (8, 8, 8))
    yield "add_tensor frame mode", S.record("add_tensor", x, use_Global=False)
    yield "add_tensor unit view", S.record("add_tensor", surface(F, "nchw", 2, OH, OW), space="unit")
    yield "add_tensor yuv without work_size", S.record("add_tensor", packed("nv12", 2, OH, OW), layout="nv12", size=(OH, OW))
    # deliver_tensor: every kind of output, layouts by default and by name, one chunk and two
    for tgt, olay in itertools.product(TARGETS, (None, "nchw", "nv12", "p210")):
        for name, B, H, W, batched in (("", 2, BH, BW, True), (" unbatched", 1, BH, BW, False), (" 65", 65, 8, 8, True)):
            if (not batched and tgt == "view") or (B == 65 and olay == "p210"):
                continue
            y = packed("nhwc", B, H, W, batched=batched)
            size = (8, 8) if B == 65 else DELIVER
            out = target(F, tgt, olay or "nhwc", B, *size, batched=batched)
            kw = {} if olay is None else {"out_layout": olay}
            yield "deliver_tensor >%s %s%s" % (tgt, olay, name), S.record("deliver_tensor", y, size, out=out, **kw)
            if tgt == "view" and olay is not None:
                yield "deliver_tensor >view layout of out %s%s" % (olay, name), S.record("deliver_tensor", y, size, out=out)
    y = packed("nhwc", 2, BH, BW)
    yield "deliver_tensor source", S.record("deliver_tensor", y, "source")
    yield "deliver_tensor u8 unit", S.record("deliver_tensor", y, DELIVER, out_dtype=torch.uint8)
    yield "deliver_tensor out_space=norm", S.record("deliver_tensor", y, DELIVER, out_space="norm", out_layout="nchw")
    yield "deliver_tensor strided y", S.record("deliver_tensor", window("nhwc", 2, BH, BW), DELIVER)
    yield "deliver_tensor u8 y", S.record("deliver_tensor", packed("nhwc", 2, BH, BW, f32=False), DELIVER)
    yield "deliver_tensor nchw y", S.record("deliver_tensor", packed("nchw", 2, BH, BW), DELIVER)
    yield "deliver_tensor bad out_size", S.record("deliver_tensor", y, (0, 8))
    yield "deliver_tensor wrong view", S.record("deliver_tensor", y, DELIVER, out=surface(F, "nhwc", 2, BH, BW))
    yield "deliver_tensor wrong out", S.record("deliver_tensor", y, DELIVER, out=packed("nhwc", 2, BH, BW))
    # prepare_style_tensor: packed images only (a crop is copied), one or a list
    style = packed("nchw", 1, OH, OW, batched=False)
    yield "prepare_style_tensor one", S.record("prepare_style_tensor", style)
    yield "prepare_style_tensor crop", S.record("prepare_style_tensor", window("nchw", 1, OH, OW, batched=False))
    yield "prepare_style_tensor list", S.record("prepare_style_tensor", [style, window("nchw", 1, BH, BW, batched=False)])
    yield "prepare_style_tensor u8 nhwc", S.record("prepare_style_tensor", packed("nhwc", 1, OH, OW, f32=False, batched=False), layout="nhwc")
    yield "prepare_style_tensor unit", S.record("prepare_style_tensor", style, space="unit")
    yield "prepare_style_tensor batched", S.record("prepare_style_tensor", packed("nchw", 2, OH, OW))
    yield "prepare_style_tensor u8 unit", S.record("prepare_style_tensor", packed("nhwc", 1, OH, OW, f32=False, batched=False), layout="nhwc", space="unit")


def refusal_cases(S):
    F = S.F
    frames, _ = host_frames("bgr", 2, BH, BW)
    x, _ = source(F, "f32nchw", 2, BH, BW)
    w, m = np.full((2, 2), 0.5, np.float32), np.full((2, 2, BH, BW), 0.5, np.float32)
    wd, md = tensor((2, 2), np.float32), tensor((2, 2, BH, BW), np.float32)
    yield "host masks with weights", S.record("transfer_batch", frames, style_weights=w, style_masks=m)
    yield "tensor masks with weights", S.record("transfer_tensor", x, style_weights=wd, style_masks=md)
    yield "host weights with work_size", S.record("transfer_frames", frames, style_weights=w, work_size=WORK)
    yield "tensor weights with work_size", S.record("transfer_tensor", x, style_weights=wd, work_size=WORK)
    yield "tensor masks with out_size", S.record("transfer_tensor", x, style_masks=md, out_size=DELIVER)
    yield "host masks with both", S.record("transfer_batch", frames, style_masks=m, work_size=WORK, out_size=DELIVER)
    yield "frame mode host masks", S.record("transfer_batch", frames, style_masks=m, use_Global=False)
    yield "frame mode tensor masks", S.record("transfer_tensor", x, style_masks=md, use_Global=False)
    yield "frame mode tensor weights", S.record("transfer_tensor", x, style_weights=wd, use_Global=False)
    for scaling in SCALINGS:
        yield "out view of the wrong size %s" % scaling, S.record("transfer_tensor", x, out=surface(F, "nchw", 2, BH + 8, BW), **SCALINGS[scaling])
        yield "out view of the wrong frame count %s" % scaling, S.record("transfer_tensor", x, out=surface(F, "nchw", 3, *out_hw(BH, BW, False, scaling)),
                                                                          **SCALINGS[scaling])
        yield "out view in another layout %s" % scaling, S.record("transfer_tensor", x, out=surface(F, "nchw", 2, *out_hw(BH, BW, False, scaling)),
                                                                  out_layout="nhwc", **SCALINGS[scaling])
        yield "out tensor of the wrong shape %s" % scaling, S.record("transfer_tensor", x, out=packed("nchw", 2, BH + 8, BW), **SCALINGS[scaling])
        yield "yuv tensor in unit space %s" % scaling, S.record("transfer_tensor", packed("nv12", 2, BH, BW), layout="nv12", size=(BH, BW), space="unit",
                                                                **SCALINGS[scaling])
        yield "yuv view in norm space %s" % scaling, S.record("transfer_tensor", surface(F, "nv12", 2, BH, BW), space="norm", **SCALINGS[scaling])
        yield "yuv output in unit space %s" % scaling, S.record("transfer_tensor", x, out_layout="nv12", out_space="unit", **SCALINGS[scaling])
        yield "u8 view out in unit space %s" % scaling, S.record("transfer_tensor", x, out=surface(F, "nchw", 2, *out_hw(BH, BW, False, scaling), f32=False),
                                                                 out_space="unit", **SCALINGS[scaling])
        yield "x on the host %s" % scaling, S.record("transfer_tensor", torch.zeros((2, 3, BH, BW)), **SCALINGS[scaling])
        yield "out on the host %s" % scaling, S.record("transfer_tensor", x, out=torch.zeros((2, 3) + tuple(out_hw(BH, BW, False, scaling))), **SCALINGS[scaling])
        yield "four channels %s" % scaling, S.record("transfer_tensor", tensor((2, 4, BH, BW), np.float32), **SCALINGS[scaling])
        yield "int32 x %s" % scaling, S.record("transfer_tensor", tensor((2, 3, BH, BW), np.int32), **SCALINGS[scaling])
        yield "bad layout %s" % scaling, S.record("transfer_tensor", x, layout="chw", **SCALINGS[scaling])
        yield "bad out_layout %s" % scaling, S.record("transfer_tensor", x, out_layout="chw", **SCALINGS[scaling])
        yield "bad space %s" % scaling, S.record("transfer_tensor", x, space="srgb", **SCALINGS[scaling])
        yield "bad out_space %s" % scaling, S.record("transfer_tensor", x, out_space="srgb", **SCALINGS[scaling])
        yield "yuv tensor without size %s" % scaling, S.record("transfer_tensor", packed("nv12", 2, BH, BW), layout="nv12", **SCALINGS[scaling])
        yield "yuv tensor of the wrong dtype %s" % scaling, S.record("transfer_tensor", packed("nv12", 2, BH, BW), layout="p010", size=(BH, BW), **SCALINGS[scaling])
        yield "f32 out for a yuv layout %s" % scaling, S.record("transfer_tensor", x, out_layout="nv12", out_dtype=torch.float32, **SCALINGS[scaling])
        # calls wrong in two ways: which of the two is reported
        yield "f32 view out named nv12 %s" % scaling, S.record("transfer_tensor", x, out=surface(F, "nchw", 2, *out_hw(BH, BW, False, scaling)), out_layout="nv12",
                                                              **SCALINGS[scaling])
        yield "x on the host and a bad out_layout %s" % scaling, S.record("transfer_tensor", torch.zeros((2, 3, BH, BW)), out_layout="chw", **SCALINGS[scaling])
        yield "four channels and a bad out_space %s" % scaling, S.record("transfer_tensor", tensor((2, 4, BH, BW), np.float32), out_space="srgb", **SCALINGS[scaling])
        yield "bad space and a bad out_space %s" % scaling, S.record("transfer_tensor", x, space="srgb", out_space="srgb", **SCALINGS[scaling])
        yield "yuv tensor without size and a bad out_layout %s" % scaling, S.record("transfer_tensor", packed("nv12", 2, BH, BW), layout="nv12", out_layout="chw",
                                                                                    **SCALINGS[scaling])
        yield "yuv tensor on the host and a bad out_space %s" % scaling, S.record("transfer_tensor", torch.zeros((2, fb("nv12", BH, BW)), dtype=torch.uint8),
                                                                                  layout="nv12", size=(BH, BW), out_space="srgb", **SCALINGS[scaling])
        yield "view on the host and a bad out_layout %s" % scaling, S.record(
            "transfer_tensor", F.ImageView(torch.zeros((BH * (BW + 5),), dtype=torch.uint8), "nhwc", (BH, BW // 3), BW + 5), out_layout="chw", **SCALINGS[scaling])
        yield "x on the host and an out of the wrong shape %s" % scaling, S.record("transfer_tensor", torch.zeros((2, 3, BH, BW)), out=packed("nchw", 2, BH + 8, BW),
                                                                                   **SCALINGS[scaling])
        yield "out of the wrong shape and five styles %s" % scaling, S.record("transfer_tensor", x, out=packed("nchw", 2, BH + 8, BW),
                                                                              style_weights=None if scaling != "plain" else tensor((2, 5), np.float32), **SCALINGS[scaling])
        yield "overlapping out view %s" % scaling, S.record("transfer_tensor", x, **SCALINGS[scaling],
                                                            out=F.ImageView(tensor((3 * (BW + 5) * 40,), np.float32), "nchw", out_hw(BH, BW, False, scaling), BW + 5, frames=2))
        yield "expanded out %s" % scaling, S.record("transfer_tensor", x, **SCALINGS[scaling],
                                                    out=tensor((2, 1) + tuple(out_hw(BH, BW, False, scaling)), np.float32).expand(2, 3, *out_hw(BH, BW, False, scaling)))
    y = packed("nhwc", 2, BH, BW)
    yield "deliver view in another layout", S.record("deliver_tensor", y, DELIVER, out=surface(F, "nchw", 2, *DELIVER), out_layout="nhwc")
    yield "deliver overlapping view", S.record("deliver_tensor", y, DELIVER, out=F.ImageView(tensor((3 * 50 * 40,), np.float32), "nchw", DELIVER, 50, frames=2))
    yield "five dimensions", S.record("transfer_tensor", tensor((1, 2, 3, BH, BW), np.float32))
    yield "no image", S.record("transfer_tensor", tensor((0, 3, BH, BW), np.float32))
    yield "transposed nhwc is copied", S.record("transfer_tensor", tensor((2, BW, BH, 3), np.uint8).permute(0, 2, 1, 3), layout="nhwc")
    yield "out_size a number", S.record("transfer_tensor", x, out_size=32)
    yield "out_size fractional", S.record("transfer_batch", frames, out_size=(32.5, 48))
    yield "yuv frames below 8 x 8", S.record("transfer_batch", np.zeros((2, fb("nv12", 4, 8)), np.uint8), in_format="nv12", size=(4, 8))
    yield "weights of another batch, host", S.record("transfer_batch", frames, style_weights=np.ones((3, 2), np.float32))
    yield "host masks tensor", S.record("transfer_tensor", x, style_masks=torch.zeros((2, 2, BH, BW)))
    yield "f64 masks tensor", S.record("transfer_tensor", x, style_masks=tensor((2, 2, BH, BW), np.float64))
    yield "strided masks tensor", S.record("transfer_tensor", x, style_masks=tensor((2, 2, BH, 2 * BW), np.float32)[..., ::2])
    yield "weights of another batch", S.record("transfer_tensor", x, style_weights=tensor((3, 2), np.float32))
    yield "host weights tensor", S.record("transfer_tensor", x, style_weights=torch.zeros((2, 2)))
    yield "f64 weights tensor", S.record("transfer_tensor", x, style_weights=tensor((2, 2), np.float64))
    yield "strided weights tensor", S.record("transfer_tensor", x, style_weights=tensor((2, 4), np.float32)[:, ::2])
    yield "masks of another size", S.record("transfer_tensor", x, style_masks=tensor((2, 2, BH, BW + 1), np.float32))
    yield "five masks", S.record("transfer_tensor", x, style_masks=tensor((2, 5, BH, BW), np.float32))
    yield "device weights on a host entry", S.record("transfer_batch", frames, style_weights=wd)
    yield "device masks on a host entry", S.record("transfer_batch", frames, style_masks=md)
    yield "mask list", S.record("transfer_batch", frames, style_masks=[[1.0]])


GROUPS = {"host": host_cases, "add": add_cases, "transfer_tensor": transfer_tensor_cases, "other": other_cases, "refusals": refusal_cases}


def record_group(F, mp, group):
    return dict(GROUPS[group](Session(F, mp)))


def load_framework(path=None):
    if path is None:
        return importlib.import_module(PKG + ".framework")
    importlib.import_module(PKG)
    spec = importlib.util.spec_from_file_location(PKG + ".framework_recorded", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- the fixture
# A record in full is some 200 bytes and there are over two thousand, so the file keeps each case as "calls:entries:result" — the first ten
# hex digits of the SHA-256 of its call lines ("-": no call reached the library), an index into the table of the entry sequences that
# occur ("rrv_transfer_view_device*2": which C entries a call reaches, readable), and an index into the table of the results and refusal
# texts that occur, in full — in the order the groups yield them; the names of a group's cases are pinned by one digest.
# `--show [WORD ..]` prints the records of the binding as it is, in full, for the cases whose names hold every WORD.
def _digest(lines):
    import hashlib
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _entries(calls):
    """"name*count name*count .." of a call sequence, runs of one entry folded"""
    runs = []
    for c in calls:
        name = c.split("(")[0]
        if runs and runs[-1][0] == name:
            runs[-1][1] += 1
        else:
            runs.append([name, 1])
    return " ".join(n if k == 1 else "%s*%d" % (n, k) for n, k in runs)


def _outcome(rec):
    return rec["raises"] if "raises" in rec else "-> %s" % (rec["result"],)


def pin(rec):
    """(calls digest, entry sequence, result or refusal) of a record: what the fixture holds of it"""
    return (_digest(rec["calls"])[:10] if rec["calls"] else "-"), _entries(rec["calls"]), _outcome(rec)


def record_all(F):
    rec = {}
    for group in GROUPS:
        with pytest.MonkeyPatch.context() as mp:
            rec[group] = record_group(F, mp, group)
    return rec


@pytest.fixture(scope="module")
def expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded():
    importlib.import_module(PKG + ".build").build_lib(verbose=False)
    return record_all(load_framework())


@pytest.mark.parametrize("group", list(GROUPS))
def test_calls_are_as_recorded(group, expected, recorded):
    got, want = recorded[group], expected["groups"][group]
    cases = [c for line in want["cases"] for c in line.split()]
    assert len(got) == len(cases) and _digest(list(got))[:16] == want["names"]      # the same cases, in the same order
    for (name, rec), case in zip(got.items(), cases):
        d, e, r = case.split(":")
        assert pin(rec) == (d, expected["entries"][int(e)], expected["outcomes"][int(r)]), "%s: %r" % (name, rec)


def test_the_record_reaches_every_entry_family(recorded):
    """the matrix is only worth its name while it reaches the entries: every family of the tensor and host paths is reached"""
    seen = {c.split("(")[0] for g in recorded.values() for r in g.values() for c in r["calls"]}
    for name in ("rrv_transfer_batch", "rrv_transfer_frames", "rrv_transfer_frame_mode_batch", "rrv_transfer_frame_mode_frames", "rrv_transfer_batch_u8",
                 "rrv_transfer_blend_batch", "rrv_transfer_blend_batch_u8", "rrv_transfer_mask_batch", "rrv_transfer_mask_batch_u8", "rrv_transfer_yuv",
                 "rrv_transfer_blend_batch_yuv", "rrv_transfer_mask_batch_yuv", "rrv_transfer_from_yuv", "rrv_transfer_blend_from_yuv",
                 "rrv_transfer_mask_from_yuv", "rrv_transfer_scaled", "rrv_transfer_deliver", "rrv_add", "rrv_add_from_yuv", "rrv_add_scaled",
                 "rrv_transfer_image_device", "rrv_transfer_image_blend_device", "rrv_transfer_image_mask_device", "rrv_transfer_from_yuv_device",
                 "rrv_transfer_blend_from_yuv_device", "rrv_transfer_mask_from_yuv_device", "rrv_transfer_view_device", "rrv_transfer_view_blend_device",
                 "rrv_transfer_view_mask_device", "rrv_transfer_scaled_view_device", "rrv_transfer_deliver_view_device", "rrv_resample_view_device",
                 "rrv_deliver_view_device", "rrv_prepare_style_image_device", "rrv_add_image_device", "rrv_add_view_device", "rrv_add_scaled_view_device",
                 "rrv_set_yuv_depth"):
        assert name in seen, name
    raised = [r["raises"] for g in recorded.values() for r in g.values() if "raises" in r]
    assert len(raised) > 100 and all(": " in t for t in raised)


def write_fixture(framework_path=None):
    importlib.import_module(PKG + ".build").build_lib(verbose=False)
    rec = record_all(load_framework(framework_path))
    entries, outcomes, groups = {}, {}, []
    for group, cases in rec.items():
        pins = [pin(r) for r in cases.values()]
        words = ["%s:%d:%d" % (d, entries.setdefault(e, len(entries)), outcomes.setdefault(o, len(outcomes))) for d, e, o in pins]
        lines = [" ".join(words[i:i + 12]) for i in range(0, len(words), 12)]
        groups.append('%s: {"names": "%s", "cases": [\n%s]}' % (json.dumps(group), _digest(list(cases))[:16], ",\n".join(json.dumps(ln) for ln in lines)))
    with open(FIXTURE, "w") as f:
        f.write('{"entries": [\n%s],\n"outcomes": [\n%s],\n"groups": {\n%s}}\n' % (
            ",\n".join(json.dumps(e) for e in entries), ",\n".join(json.dumps(o) for o in outcomes), ",\n".join(groups)))
    print("%s: %d cases, %d bytes" % (FIXTURE, sum(len(c) for c in rec.values()), os.path.getsize(FIXTURE)))


def show(words, framework_path=None):
    importlib.import_module(PKG + ".build").build_lib(verbose=False)
    for group, cases in record_all(load_framework(framework_path)).items():
        for name, rec in cases.items():
            if all(w in name for w in words):
                print("%s | %s: %s" % (group, name, json.dumps(rec)))


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--framework") + 1] if "--framework" in sys.argv else None
    if "--write" in sys.argv:
        write_fixture(path)
    elif "--show" in sys.argv:
        show([w for w in sys.argv[sys.argv.index("--show") + 1:] if w != "--framework" and w != path], path)
    else:
        sys.exit("usage: python tests/test_call_record.py --write | --show [WORD ..]   [--framework FILE]")

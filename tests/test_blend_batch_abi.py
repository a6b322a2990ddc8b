"""CPU checks of the blended frame entries (rrv_transfer_image_blend_device, rrv_transfer_blend_batch[_u8]) and of the
preparation from device images (rrv_prepare_style_image_device, rrv_add_image_device): declared in the header, listed in the
ctypes table, exported by the built library; bad arguments are refused before a device is touched; the Python check of
`style_weights` (style_weight_args) accepts and rejects what it should without a GPU."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("rerevst-code_amd._lib")
F = importlib.import_module("rerevst-code_amd.framework")
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rerevst_hip.h")).read(), flags=re.S)
RRV_E_ARG = -1
NEW = ("rrv_transfer_image_blend_device", "rrv_transfer_blend_batch", "rrv_transfer_blend_batch_u8",
       "rrv_prepare_style_image_device", "rrv_add_image_device")


def _lib():
    importlib.import_module("rerevst-code_amd.build").build_lib(verbose=False)
    return L.load()


def _params(name):
    """the parameter list of a declared function, one normalised string per parameter"""
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, HDR)
    assert m, "%s is not declared" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_table_and_library_carry_the_entries():
    m = re.search(r"#define RRV_TF_WEIGHTS_DEVICE\s+(\S.*)", HDR)
    assert m and eval(m.group(1).strip(), {"__builtins__": {}}) == L.TF_WEIGHTS_DEVICE == 8      # a C integer constant expression
    assert len({L.TF_PAD_CROP, L.TF_FRAME_MODE, L.TF_ON_STREAM, L.TF_WEIGHTS_DEVICE}) == 4
    assert _params("rrv_transfer_image_blend_device") == [
        "rrv_handle h", "const void* d_in", "rrv_image_desc in", "int B", "int H", "int W", "const float* style_weight", "int n_styles",
        "void* d_out", "rrv_image_desc out", "int flags", "void* hip_stream"]
    host = ["rrv_handle h", "const uint8_t* frames_bgr", "int B", "int H", "int W", "const float* style_weight", "int n_styles", "int pad_crop"]
    assert _params("rrv_transfer_blend_batch") == host + ["float* out_bgr"]
    assert _params("rrv_transfer_blend_batch_u8") == host + ["uint8_t* out_bgr"]
    assert _params("rrv_prepare_style_image_device") == ["rrv_handle h", "const void* d_style", "rrv_image_desc in", "int Hs", "int Ws",
                                                         "int style_id", "void* hip_stream"]
    assert _params("rrv_add_image_device") == ["rrv_handle h", "const void* d_frame", "rrv_image_desc in", "int H", "int W", "void* hip_stream"]
    assert L.SYMBOLS["rrv_transfer_blend_batch_u8"] == L.SYMBOLS["rrv_transfer_blend_batch"] and "rrv_transfer_blend_batch" in L.U8_TWINS
    assert len(L.SYMBOLS["rrv_transfer_image_blend_device"][1]) == 12 and len(L.SYMBOLS["rrv_transfer_blend_batch"][1]) == 9
    assert L.SYMBOLS["rrv_transfer_image_blend_device"][1][2] is L.ImageDesc and L.SYMBOLS["rrv_transfer_image_blend_device"][1][9] is L.ImageDesc
    lib = _lib()
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(lib, name), name


def test_argument_checks_need_no_device():
    lib = _lib()
    u8 = L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_PIXEL)
    f32 = L.ImageDesc(L.DT_F32, L.LAY_HWC_BGR, L.SP_PIXEL)
    frames = np.zeros((2, 64, 64, 3), np.uint8)
    out = np.zeros((2, 64, 64, 3), np.float32)
    wts = np.full((2, 2), 0.5, np.float32)
    fp, op, wp = (a.ctypes.data_as(C.c_void_p) for a in (frames, out, wts))
    wf = wts.ctypes.data_as(C.POINTER(C.c_float))
    # no handle: refused, whatever else is passed
    assert lib.rrv_transfer_image_blend_device(None, fp, u8, 2, 64, 64, wp, 2, op, f32, 0, None) == RRV_E_ARG
    for fn in (lib.rrv_transfer_blend_batch, lib.rrv_transfer_blend_batch_u8):
        assert fn(None, fp, 2, 64, 64, wf, 2, 0, op) == RRV_E_ARG
    assert lib.rrv_prepare_style_image_device(None, fp, u8, 64, 64, 0, None) == RRV_E_ARG
    assert lib.rrv_add_image_device(None, fp, u8, 64, 64, None) == RRV_E_ARG
    h = C.c_void_p()
    if lib.rrv_create(0, C.byref(h)) != 0:
        return                                      # no GPU here: a handle cannot exist
    try:      # (the host buffers stand in for device ones: every call below is refused before anything reads them)
        img = lib.rrv_transfer_image_blend_device
        assert img(h, None, u8, 2, 64, 64, wp, 2, op, f32, 0, None) == RRV_E_ARG
        assert img(h, fp, u8, 2, 64, 64, wp, 2, None, f32, 0, None) == RRV_E_ARG
        assert img(h, fp, u8, 2, 64, 64, None, 2, op, f32, 0, None) == RRV_E_ARG
        for B in (0, -1, 65):
            assert img(h, fp, u8, B, 64, 64, wp, 2, op, f32, 0, None) == RRV_E_ARG, B
        for ns in (0, -1, L.MAX_STYLES + 1):
            assert img(h, fp, u8, 2, 64, 64, wp, ns, op, f32, 0, None) == RRV_E_ARG, ns
        assert img(h, fp, u8, 2, 64, 64, wp, 2, op, f32, 16, None) == RRV_E_ARG                       # unknown flag
        assert img(h, fp, u8, 2, 64, 64, wp, 2, op, f32, L.TF_FRAME_MODE, None) == RRV_E_ARG          # frame mode has no blended state
        assert img(h, fp, u8, 2, 64, 64, wp, 2, op, f32, L.TF_FRAME_MODE | L.TF_WEIGHTS_DEVICE, None) == RRV_E_ARG
        assert img(h, fp, L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_UNIT), 2, 64, 64, wp, 2, op, f32, 0, None) == RRV_E_ARG
        # the plain entry does not know the weights flag
        assert lib.rrv_transfer_image_device(h, fp, u8, 2, 64, 64, op, f32, L.TF_WEIGHTS_DEVICE, None) == RRV_E_ARG
        for fn in (lib.rrv_transfer_blend_batch, lib.rrv_transfer_blend_batch_u8):
            assert fn(h, None, 2, 64, 64, wf, 2, 0, op) == RRV_E_ARG
            assert fn(h, fp, 2, 64, 64, wf, 2, 0, None) == RRV_E_ARG
            assert fn(h, fp, 2, 64, 64, None, 2, 0, op) == RRV_E_ARG
            assert fn(h, fp, 0, 64, 64, wf, 2, 0, op) == RRV_E_ARG
            for ns in (0, L.MAX_STYLES + 1):
                assert fn(h, fp, 2, 64, 64, wf, ns, 0, op) == RRV_E_ARG
        prep, add = lib.rrv_prepare_style_image_device, lib.rrv_add_image_device
        assert prep(h, None, u8, 64, 64, 0, None) == RRV_E_ARG
        assert prep(h, fp, u8, 64, 64, L.MAX_STYLES, None) == RRV_E_ARG and prep(h, fp, u8, 64, 64, -1, None) == RRV_E_ARG
        assert prep(h, fp, u8, 7, 64, 0, None) == RRV_E_ARG
        assert prep(h, fp, L.ImageDesc(L.DT_U8, L.LAY_CHW_RGB, L.SP_NORM), 64, 64, 0, None) == RRV_E_ARG
        assert prep(h, fp, L.ImageDesc(2, 0, 0), 64, 64, 0, None) == RRV_E_ARG
        assert add(h, None, u8, 64, 64, None) == RRV_E_ARG
        assert add(h, fp, L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_UNIT), 64, 64, None) == RRV_E_ARG
        assert add(h, fp, L.ImageDesc(L.DT_F32, 2, 0), 64, 64, None) == RRV_E_ARG
    finally:
        lib.rrv_destroy(h)


def test_framework_signatures():
    for name in ("transfer_batch", "transfer_frames", "transfer_tensor"):
        for cls in (F.Stylization, F.MultiStyleStylization):
            assert inspect.signature(getattr(cls, name)).parameters["style_weights"].default is None, (cls.__name__, name)
    assert list(inspect.signature(F.Stylization.transfer_batch).parameters)[:4] == ["self", "frames", "out", "dtype"]
    assert list(inspect.signature(F.Stylization.transfer_frames).parameters)[:4] == ["self", "frames", "out", "dtype"]
    for name in ("prepare_style_tensor", "add_tensor"):
        p = inspect.signature(getattr(F.MultiStyleStylization, name)).parameters
        assert p["space"].default == "pixel" and p["layout"].default == "nchw", name
    # tensor_io_args keeps its signature
    assert list(inspect.signature(F.tensor_io_args).parameters) == ["x", "device", "space", "out_space", "out_dtype", "layout", "out_layout",
                                                                    "pad_crop", "out"]


def test_host_weights_accepts_and_shapes():
    w = F.style_weight_args([0.25, 0.75], 3, 2, 0)
    assert w.dev is None and w.S == 2 and not w.broadcast
    assert w.host.dtype == np.float32 and w.host.shape == (3, 2) and w.host.flags.c_contiguous
    np.testing.assert_array_equal(w.host, np.array([[0.25, 0.75]] * 3, np.float32))
    rows = [[1.0, 0.0, 0.0], [0.5, 0.25, 0.25]]
    w = F.style_weight_args(rows, 2, 4, 0)
    assert w.S == 3 and w.host.shape == (2, 3)
    np.testing.assert_array_equal(w.host, np.array(rows, np.float32))
    w = F.style_weight_args(np.asarray(rows, np.float64)[:, ::-1], 2, 3, 0)        # float64, not contiguous: converted
    assert w.host.dtype == np.float32 and w.host.flags.c_contiguous and w.host[1, 0] == np.float32(0.25)
    assert F.style_weight_args(np.ones((1, 8), np.float32), 1, 8, 0).S == 8


@pytest.mark.parametrize("case", ["wrong_B", "too_many_styles", "above_max_styles", "no_styles", "rank3", "scalar", "frame_mode"])
def test_host_weights_rejects(case):
    args = dict(wrong_B=(np.ones((3, 2)), 4, 2), too_many_styles=(np.ones((2, 3)), 2, 2), above_max_styles=(np.ones((2, 9)), 2, 16),
                no_styles=(np.ones((2, 0)), 2, 2), rank3=(np.ones((2, 2, 2)), 2, 2), scalar=(0.5, 1, 1), frame_mode=(np.ones((2, 2)), 2, 2))[case]
    with pytest.raises(ValueError):
        F.style_weight_args(args[0], args[1], args[2], 0, use_Global=case != "frame_mode")


torch = pytest.importorskip("torch")


class _OnGpu:
    """A CPU tensor that reports a GPU device: style_weight_args only reads device, dtype, shape and contiguity."""

    def __init__(self, t, index=0):
        self.t, self.device = t, torch.device("cuda", index)

    dtype = property(lambda self: self.t.dtype)
    shape = property(lambda self: self.t.shape)

    def dim(self):
        return self.t.dim()

    def is_contiguous(self):
        return self.t.is_contiguous()


def test_device_weights_accepts():
    t = _OnGpu(torch.ones((5, 3)))
    w = F.style_weight_args(t, 5, 4, 0, tensors=True)
    assert w.dev is t and w.host is None and w.S == 3 and not w.broadcast
    t = _OnGpu(torch.ones(2), index=1)
    w = F.style_weight_args(t, 7, 2, 1, tensors=True)
    assert w.dev is t and w.S == 2 and w.broadcast


@pytest.mark.parametrize("case", ["cpu", "other_device", "float64", "float16", "non_contiguous", "wrong_B", "too_many_styles", "rank3",
                                  "frame_mode", "host_entry"])
def test_device_weights_rejects(case):
    t, B, kw = _OnGpu(torch.ones((4, 2))), 4, dict(tensors=True)
    if case == "cpu":
        t = torch.ones((4, 2))                                      # a device tensor is required: host weights go as list / ndarray
    elif case == "other_device":
        t = _OnGpu(torch.ones((4, 2)), index=1)
    elif case == "float64":
        t = _OnGpu(torch.ones((4, 2), dtype=torch.float64))
    elif case == "float16":
        t = _OnGpu(torch.ones((4, 2), dtype=torch.float16))
    elif case == "non_contiguous":
        t = _OnGpu(torch.ones((2, 4)).t())
        assert not t.is_contiguous() and tuple(t.shape) == (4, 2)
    elif case == "wrong_B":
        B = 5
    elif case == "too_many_styles":
        t = _OnGpu(torch.ones((4, 3)))
    elif case == "rank3":
        t = _OnGpu(torch.ones((4, 2, 1)))
    elif case == "frame_mode":
        kw["use_Global"] = False
    elif case == "host_entry":
        kw["tensors"] = False                                       # transfer_batch / transfer_frames take host weights
    with pytest.raises(ValueError):
        F.style_weight_args(t, B, 2, 0, **kw)


def test_methods_refuse_weights_before_the_library_is_called():
    """transfer_batch / transfer_frames check the weights first: a frame-mode handle and a wrong B never reach the library."""
    class Lib:
        def __getattr__(self, name):
            raise AssertionError("library entry %s called" % name)

    frames = np.zeros((2, 16, 16, 3), np.uint8)
    for use_global, wts in ((False, [[1.0], [1.0]]), (True, [[1.0]] * 3), (True, [[0.5, 0.5]] * 2)):
        s = F.Stylization.__new__(F.Stylization)
        s._lib, s._h, s.use_Global, s.style_num, s.device = Lib(), None, use_global, 1, 0
        for fn in (s.transfer_batch, s.transfer_frames):
            with pytest.raises(ValueError):
                fn(frames, out=np.zeros((2, 16, 16, 3), np.float32), style_weights=wts)

"""CPU checks of the torch-tensor entry (rrv_transfer_image_device, Stylization.transfer_tensor): the header declares it with
its descriptor and constants, the library and the ctypes table export it, and the argument checks of transfer_tensor
(tensor_io_args) reject every bad input without a GPU."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("rerevst-code_amd._lib")
HDR = open(os.path.join(ROOT, "include", "rerevst_hip.h")).read()


def test_header_declares_entry_descriptor_and_constants():
    assert re.search(r"typedef struct\s*\{\s*int dtype;\s*int layout;\s*int space;\s*\}\s*rrv_image_desc;", HDR)
    assert re.search(r"int rrv_transfer_image_device\(rrv_handle h, const void\* d_in, rrv_image_desc in, int B, int H, int W,\s*"
                     r"void\* d_out, rrv_image_desc out, int flags, void\* hip_stream\);", HDR)
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (RRV_(?:DT|LAY|SP|TF)_[A-Z_0-9]+) (\d+)", HDR))
    assert consts == {"RRV_DT_U8": L.DT_U8, "RRV_DT_F32": L.DT_F32, "RRV_LAY_HWC_BGR": L.LAY_HWC_BGR, "RRV_LAY_CHW_RGB": L.LAY_CHW_RGB,
                      "RRV_SP_PIXEL": L.SP_PIXEL, "RRV_SP_UNIT": L.SP_UNIT, "RRV_SP_NORM": L.SP_NORM,
                      "RRV_TF_PAD_CROP": L.TF_PAD_CROP, "RRV_TF_FRAME_MODE": L.TF_FRAME_MODE, "RRV_TF_ON_STREAM": L.TF_ON_STREAM}
    assert len(set(consts[k] for k in consts if "_TF_" in k)) == 3


def test_library_exports_the_entry():
    b = importlib.import_module("rerevst-code_amd.build")
    b.build_lib(verbose=False)
    lib = L.load()
    assert hasattr(lib, "rrv_transfer_image_device")
    res, args = L.SYMBOLS["rrv_transfer_image_device"]
    assert args[2] is L.ImageDesc and args[7] is L.ImageDesc and len(args) == 10
    assert [f[0] for f in L.ImageDesc._fields_] == ["dtype", "layout", "space"]


torch = pytest.importorskip("torch")
F = importlib.import_module("rerevst-code_amd.framework")


class _OnGpu:
    """A CPU tensor that reports a GPU device: tensor_io_args only reads device, dtype, shape and contiguity, so the checks
    run without a GPU."""

    def __init__(self, t, index=0):
        self.t, self.device = t, torch.device("cuda", index)

    dtype = property(lambda self: self.t.dtype)
    shape = property(lambda self: self.t.shape)

    def dim(self):
        return self.t.dim()

    def is_contiguous(self):
        return self.t.is_contiguous()

    def contiguous(self):
        return _OnGpu(self.t.contiguous(), self.device.index)


def _x(shape=(2, 3, 20, 28), dtype=torch.uint8):
    return _OnGpu(torch.zeros(shape, dtype=dtype))


def test_validation_accepts_and_shapes():
    a = F.tensor_io_args(_x(), 0)
    assert a.out_shape == (2, 3, 16, 24) and a.out_dtype == torch.float32 and (a.B, a.H, a.W) == (2, 20, 28) and a.batched
    assert (a.in_desc.dtype, a.in_desc.layout, a.in_desc.space) == (L.DT_U8, L.LAY_CHW_RGB, L.SP_PIXEL)
    a = F.tensor_io_args(_x((20, 28, 3), torch.float32), 0, layout="nhwc", space="norm", out_space="unit", out_layout="nchw",
                         pad_crop=True)
    assert a.out_shape == (3, 20, 28) and not a.batched and a.B == 1
    assert (a.out_desc.dtype, a.out_desc.layout, a.out_desc.space) == (L.DT_F32, L.LAY_CHW_RGB, L.SP_UNIT)
    a = F.tensor_io_args(_x(), 0, out_dtype=torch.uint8)
    assert a.out_desc.dtype == L.DT_U8


def test_validation_makes_input_contiguous():
    x = _OnGpu(torch.zeros((2, 20, 28, 3), dtype=torch.float32).permute(0, 3, 1, 2))
    assert not x.is_contiguous()
    a = F.tensor_io_args(x, 0)
    assert a.x.is_contiguous() and tuple(a.x.shape) == (2, 3, 20, 28)


@pytest.mark.parametrize("case", ["cpu", "other_device", "channels", "channels_nhwc", "rank", "dtype", "u8_unit", "u8_norm",
                                  "out_u8_norm", "out_u8_unit", "out_dtype", "space", "layout", "out_shape", "out_device", "empty"])
def test_validation_rejects(case):
    kw = {}
    x = _x()
    if case == "cpu":
        x = torch.zeros((2, 3, 20, 28), dtype=torch.uint8)
    elif case == "other_device":
        x = _OnGpu(torch.zeros((2, 3, 20, 28), dtype=torch.uint8), index=1)
    elif case == "channels":
        x = _x((2, 4, 20, 28))
    elif case == "channels_nhwc":
        x, kw = _x((2, 3, 20, 28)), dict(layout="nhwc")
    elif case == "rank":
        x = _x((3, 20))
    elif case == "dtype":
        x = _x(dtype=torch.float64)
    elif case == "u8_unit":
        kw = dict(space="unit")
    elif case == "u8_norm":
        kw = dict(space="norm")
    elif case == "out_u8_norm":
        kw = dict(out_dtype=torch.uint8, out_space="norm")
    elif case == "out_u8_unit":
        kw = dict(out_dtype=torch.uint8, out_space="unit")
    elif case == "out_dtype":
        kw = dict(out_dtype=torch.float16)
    elif case == "space":
        kw = dict(space="linear")
    elif case == "layout":
        kw = dict(layout="chw")
    elif case == "out_shape":
        kw = dict(out=_x((2, 3, 20, 28), torch.float32))
    elif case == "out_device":
        kw = dict(out=torch.zeros((2, 3, 16, 24)))
    elif case == "empty":
        x = _x((0, 3, 20, 28))
    with pytest.raises(ValueError):
        F.tensor_io_args(x, 0, **kw)


def test_package_imports_without_torch():
    """torch stays optional: the package and its framework module import in a process where torch cannot be imported."""
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, %r); import importlib; "
            "importlib.import_module('rerevst-code_amd.framework'); print('ok')" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr

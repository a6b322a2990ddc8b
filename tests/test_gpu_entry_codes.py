"""The return code of every transfer entry family for every single violation of its contract, on live handles: one call per
(family, violation), each refused before a kernel is launched.  The expected codes are literals, read from the checks each path
had of its own before check_xfer took them over: the file passes unchanged on both sides of that change.  Three handles: `bare`
has no weights, `ready` has weights and nothing else, `one` has style 0 prepared and computed and style 1 untouched.  The
buffers are host arrays of the stated size standing in for device ones (tests/test_mask_blend_abi.py does the same): the host
entries may copy them to the device before they find the handle's state wanting, nothing else reads them.  Run with -m gpu."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = importlib.import_module("rerevst-code_amd._lib")
OK, E_ARG, E_WEIGHTS, E_STATE = 0, -1, -3, -4
U8 = L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_PIXEL)
F32 = L.ImageDesc(L.DT_F32, L.LAY_HWC_BGR, L.SP_PIXEL)
BMAX = 65                                                   # the largest B a case passes
FRAMES = np.zeros((BMAX, 64, 64, 3), np.uint8)
OUT = np.zeros((BMAX, 64, 64, 3), np.float32)
WTS = np.full((BMAX, L.MAX_STYLES + 1), 0.5, np.float32)
MASK = np.full((2, 2, 64, 64), 0.5, np.float32)             # B = 2 and ns = 2 at the most where a mask is read; 64 x 64 host floats otherwise
FP, OP, WP, MP = (a.ctypes.data_as(C.c_void_p) for a in (FRAMES, OUT, WTS, MASK))


class Req:
    """the arguments of one call; a case changes one of them"""
    def __init__(self, **kw):
        self.fin, self.fout, self.B, self.H, self.W, self.ns, self.mi, self.flags = FP, OP, 2, 64, 64, 1, 1, 0
        self.__dict__.update(kw)


def _lib():
    return L.load()


WF, MF = (C.cast(p, C.POINTER(C.c_float)) for p in (WP, MP))


def _device(name):
    return lambda h, r: getattr(_lib(), name)(h, r.fin, r.B, r.H, r.W, r.fout)


def _image(extra=0):
    return lambda h, r: _lib().rrv_transfer_image_device(h, r.fin, U8, r.B, r.H, r.W, r.fout, F32, r.flags | extra, None)


def _image_blend(h, r):
    return _lib().rrv_transfer_image_blend_device(h, r.fin, U8, r.B, r.H, r.W, WP, r.ns, r.fout, F32, r.flags, None)


def _image_mask(h, r):
    return _lib().rrv_transfer_image_mask_device(h, r.fin, U8, r.B, r.H, r.W, MP, r.ns, r.mi, r.fout, F32, r.flags, None)


def _blend_batch(name, pad):
    return lambda h, r: getattr(_lib(), name)(h, r.fin, r.B, r.H, r.W, WF, r.ns, pad, r.fout)


def _mask_batch(name, pad):
    return lambda h, r: getattr(_lib(), name)(h, r.fin, r.B, r.H, r.W, MF, r.ns, r.mi, pad, r.fout)


# family -> (call, padded twin of the call or None, model, takes B up to 64 only)
FAMILIES = {
    "device": (_device("rrv_transfer_batch_device"), _device("rrv_transfer_frames_device"), "global", True),
    "device_u8": (_device("rrv_transfer_batch_device_u8"), _device("rrv_transfer_frames_device_u8"), "global", True),
    "frame_mode_device": (_device("rrv_transfer_frame_mode_batch_device"), _device("rrv_transfer_frame_mode_frames_device"), "frame", True),
    "image": (_image(), _image(L.TF_PAD_CROP), "global", True),
    "image_frame_mode": (_image(L.TF_FRAME_MODE), _image(L.TF_FRAME_MODE | L.TF_PAD_CROP), "frame", True),
    "image_blend": (_image_blend, lambda h, r: _image_blend(h, Req(**dict(r.__dict__, flags=r.flags | L.TF_PAD_CROP))), "blend", True),
    "image_mask": (_image_mask, lambda h, r: _image_mask(h, Req(**dict(r.__dict__, flags=r.flags | L.TF_PAD_CROP))), "mask", True),
    "host_batch": (_device("rrv_transfer_batch"), None, "global", False),
    "host_batch_u8": (_device("rrv_transfer_batch_u8"), None, "global", False),
    "host_frames": (_device("rrv_transfer_frames"), None, "global", False),                  # (pad and crop is what it does)
    "blend_batch": (_blend_batch("rrv_transfer_blend_batch", 0), _blend_batch("rrv_transfer_blend_batch", 1), "blend", False),
    "blend_batch_u8": (_blend_batch("rrv_transfer_blend_batch_u8", 0), _blend_batch("rrv_transfer_blend_batch_u8", 1), "blend", False),
    "mask_batch": (_mask_batch("rrv_transfer_mask_batch", 0), _mask_batch("rrv_transfer_mask_batch", 1), "mask", False),
    "mask_batch_u8": (_mask_batch("rrv_transfer_mask_batch_u8", 0), _mask_batch("rrv_transfer_mask_batch_u8", 1), "mask", False),
    "frame_mode_batch": (_device("rrv_transfer_frame_mode_batch"), None, "frame", False),
    "frame_mode_frames": (_device("rrv_transfer_frame_mode_frames"), None, "frame", False),
}


def _err(h):
    return (_lib().rrv_last_error(h) or b"").decode()


@pytest.fixture(scope="module")
def bare():
    h = C.c_void_p()
    assert _lib().rrv_create(0, C.byref(h)) == OK
    yield h
    _lib().rrv_destroy(h)


@pytest.fixture(scope="module")
def ready(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, style_num=2)
    yield s._h
    s.close()


@pytest.fixture(scope="module")
def one(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, style_num=2)
    s.prepare_style(pkg.synth_style(64, 64, kind="smooth", seed=7))
    s.clean()
    for i in (0, 2):
        s.add(pkg.synth_frame(i, 64, 64, kind="smooth"))
    s.compute()
    s.sync()
    yield s._h
    s.close()


def test_null_handle_is_an_argument_error():
    for name, (call, padded, _, _) in FAMILIES.items():
        assert call(None, Req()) == E_ARG, name
        if padded:
            assert padded(None, Req()) == E_ARG, name


def test_argument_violations(one):
    """every code here is RRV_E_ARG; style 0 is computed and prepared, so with ns = 1 the argument is the only violation"""
    for name, (call, padded, model, b64) in FAMILIES.items():
        cases = {"null input": Req(fin=None), "null output": Req(fout=None), "B = 0": Req(B=0), "H = 0": Req(H=0), "W = 0": Req(W=0),
                 "frame above the size limit": Req(H=5800, W=5800)}
        if b64:
            cases["B = 65"] = Req(B=65)
        if model in ("blend", "mask"):
            cases["ns = 0"] = Req(ns=0)
            cases["ns = RRV_MAX_STYLES + 1"] = Req(ns=L.MAX_STYLES + 1)
        if model == "mask":
            cases["mask_images = 3 with B = 2"] = Req(mi=3)
            cases["mask_images = 0"] = Req(mi=0)
        if name in ("image_blend", "image_mask"):
            cases["frame-mode flag"] = Req(flags=L.TF_FRAME_MODE)
        for what, r in cases.items():
            for kind, fn in (("", call), (" (pad and crop)", padded)):
                if fn is None:
                    continue
                rc = fn(one, r)
                print("%-18s %-28s%-16s -> %d" % (name, what, kind, rc))
                assert rc == E_ARG, (name, what + kind, _err(one))
                if what == "frame above the size limit":
                    assert "too large" in _err(one), (name, kind, _err(one))


def test_state_violations(ready, one):
    """RRV_E_STATE: the global model with no state computed, the frame-mode model before prepare_style (both on `ready`), and styles
    0..1 asked for with style 1 not computed (`one`)"""
    for name, (call, padded, model, _) in FAMILIES.items():
        for kind, fn in (("", call), (" (pad and crop)", padded)):
            if fn is None:
                continue
            if model in ("global", "frame"):
                rc = fn(ready, Req())
                print("%-18s nothing prepared%-16s -> %d" % (name, kind, rc))
                assert rc == E_STATE, (name, kind, _err(ready))
                if model == "global":
                    assert "state not computed" in _err(ready), (name, kind, _err(ready))
            else:
                rc = fn(one, Req(ns=2, mi=2))
                print("%-18s style 1 not computed%-16s -> %d" % (name, kind, rc))
                assert rc == E_STATE, (name, kind, _err(one))
                assert "state not computed" in _err(one), (name, kind, _err(one))


def test_weights_not_finalized(bare):
    """RRV_E_WEIGHTS from every family but one: a handle without weights has no computed style either, and rrv_transfer_mask_batch
    looks at the styles before the weights"""
    for name, (call, padded, model, _) in FAMILIES.items():
        want = E_STATE if name.startswith("mask_batch") else E_WEIGHTS
        for kind, fn in (("", call), (" (pad and crop)", padded)):
            if fn is None:
                continue
            rc = fn(bare, Req())
            print("%-18s no weights%-16s -> %d" % (name, kind, rc))
            assert rc == want, (name, kind, _err(bare))

"""rrv_deliver_view_device, the delivery stage alone, against tests/deliver_ref.py: one test per deliver_k<OUT> instantiation
(tests/test_deliver_host.py's ledger cites these tests by name), every shape of deliver_ref.SHAPES, B = 3, the output written through a
ragged view into a sentinel-filled canvas whose every element outside the planes' rows must keep the sentinel.

Float forms: within deliver_ref.tolerance (derived there) of the float64 reference of the launch's own input, in the PIXEL, UNIT and
NORM spaces.  Integer forms: bit for bit the reference conversion (to_uint8, chroma_ref.yuv_ref) of the float32 HWC PIXEL frame the same
kernel family delivers for the same input and sizes; with the float test this ties every code to the float64 reference, with no case
left out near a rounding boundary.  Identity sizes return the input (and its conversions) bit for bit; frame 1 of the B = 3 call equals
the B = 1 call on that frame."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chroma_ref
import deliver_ref as DR
import resample_ref as R
import view_ref as V
from conftest import load_golden

pytestmark = pytest.mark.gpu

RRV_OK, RRV_E_ARG, RRV_E_NOMEM = 0, -1, -5
L = importlib.import_module("rerevst-code_amd._lib")
B = 3
_SPACE = {"pixel": L.SP_PIXEL, "unit": L.SP_UNIT, "norm": L.SP_NORM}
_SENTINEL = {np.float32: np.float32(-12345.5), np.uint8: np.uint8(0xA5), np.uint16: np.uint16(0xA5A5)}
_VDT = {np.uint8: V.DT_U8, np.float32: V.DT_F32, np.uint16: V.DT_U16}
YUV8 = ("i420", "nv12", "i422", "nv16", "i444", "nv24")
YUV16 = ("i420p10", "p010", "i422p10", "p210", "i444p10", "p410", "p012")      # and one 12-bit format, the code in the high bits


def _torch():
    import torch
    return torch


def _dev(a):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


@pytest.fixture(scope="module")
def hip(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    s.set_state(load_golden("global_a")["state"])
    yield s
    s.close()


def _view_struct(v, space="pixel"):
    out = L.ImageView()
    out.desc = L.ImageDesc(v["dtype"], v["layout"], _SPACE[space])
    out.frame_stride = v["frame_stride"]
    for k in range(3):
        out.plane_offset[k], out.pitch[k] = v["plane_offset"][k], v["pitch"][k]
    return out


_inputs = {}


def _input(k):
    """shape k's working frames, random float32 in 0..255: (numpy [B][H][W][3], the device copy), made once and never changed"""
    if k not in _inputs:
        (H, W), _ = DR.SHAPES[k]
        px = np.random.default_rng(700 + k).uniform(0.0, 255.0, (B, H, W, 3)).astype(np.float32)
        _inputs[k] = (px, _dev(px))
    return _inputs[k]


def _addressed(view, layout, nb, H, W, chroma, n):
    """the elements of an n-element canvas that the planes' rows of nb frames cover"""
    m = np.zeros(n, bool)
    for b in range(nb):
        for k, (ln, rows) in enumerate(R.planes(layout, H, W, chroma)):
            for r in range(rows):
                at = b * view["frame_stride"] + view["plane_offset"][k] + r * view["pitch"][k]
                m[at:at + ln] = True
    return m


def _deliver(s, k, dtype, layout, space="pixel", chroma="420", nb=B, first=0):
    """One call on frames first .. first + nb - 1 of shape k's input, through the ragged view of the form: (rc, [nb][frame elements] as the
    view's rows hold them).  Everything outside those rows must still be the sentinel."""
    (H, W), (DH, DW) = DR.SHAPES[k]
    v = R.ragged(_VDT[dtype], layout, DH, DW, chroma)
    n = (nb - 1) * v["frame_stride"] + R.extent(v, layout, DH, DW, chroma) + 9
    d_canvas = _dev(np.full(n, _SENTINEL[dtype], dtype))
    d_in = _input(k)[1]
    _torch().cuda.synchronize()
    rc = L.load().rrv_deliver_view_device(s._h, C.c_void_p(d_in[first].data_ptr()), nb, H, W, DH, DW, C.c_void_p(d_canvas.data_ptr()),
                                          C.byref(_view_struct(v, space)), None)
    _torch().cuda.synchronize()
    canvas = d_canvas.cpu().numpy().view(dtype)
    inside = _addressed(v, layout, nb, DH, DW, chroma, n)
    assert (~inside).sum() > 20 and (canvas[~inside] == _SENTINEL[dtype]).all(), "stores outside the planes' rows"
    return rc, R.gather(canvas, v, layout, nb, DH, DW, chroma)


def _ok(s, rc):
    assert rc == RRV_OK, s._lib.rrv_last_error(s._h)


_pixel = {}


def _pixel_out(s, k):
    """the float32 HWC BGR PIXEL frames deliver_k delivers for shape k: [B][DH][DW][3], computed once"""
    if k not in _pixel:
        rc, got = _deliver(s, k, np.float32, V.LAY_HWC_BGR)
        _ok(s, rc)
        _pixel[k] = got.reshape((B,) + DR.SHAPES[k][1] + (3,))
    return _pixel[k]


def _batch_independent(s, k, got, dtype, layout, space="pixel", chroma="420"):
    rc, one = _deliver(s, k, dtype, layout, space, chroma, nb=1, first=1)
    _ok(s, rc)
    np.testing.assert_array_equal(one[0].view(np.uint8), got[1].view(np.uint8))


def _float_form(s, chw):
    layout = V.LAY_CHW_RGB if chw else V.LAY_HWC_BGR
    for k, ((H, W), (DH, DW)) in enumerate(DR.SHAPES):
        px = _input(k)[0]
        for space in DR.SPACES:
            rc, got = _deliver(s, k, np.float32, layout, space)
            _ok(s, rc)
            ref = DR.float_ref(px, DH, DW, space, chw).reshape(B, -1)
            tol = DR.tolerance(space, H, W, DH, DW)
            err = np.abs(got.astype(np.float64) - ref).max()
            print("%s %s %dx%d -> %dx%d: max |got - ref| = %.3g (bound %.3g)" % ("chw" if chw else "hwc", space, H, W, DH, DW, err, tol))
            assert ref.std() > 0.05 and err <= tol, (chw, space, k, err, tol)
            if space == "pixel" and (H, W) == (DH, DW):      # identity: the input, bit for bit
                want = px[..., ::-1].transpose(0, 3, 1, 2) if chw else px
                np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(want).reshape(B, -1).view(np.uint32))
            _batch_independent(s, k, got, np.float32, layout, space)


def test_deliver_f32_hwc_against_reference(hip):
    """deliver_k<0>: float32 HWC BGR in the three spaces against the float64 reference"""
    _float_form(hip, False)


def test_deliver_f32_chw_against_reference(hip):
    """deliver_k<1>: float32 planar RGB in the three spaces against the float64 reference"""
    _float_form(hip, True)


def _u8_form(s, chw):
    layout = V.LAY_CHW_RGB if chw else V.LAY_HWC_BGR
    for k, ((H, W), (DH, DW)) in enumerate(DR.SHAPES):
        rc, got = _deliver(s, k, np.uint8, layout)
        _ok(s, rc)
        np.testing.assert_array_equal(got, DR.u8_ref(_pixel_out(s, k), chw).reshape(B, -1))
        if (H, W) == (DH, DW):
            np.testing.assert_array_equal(got, DR.u8_ref(_input(k)[0], chw).reshape(B, -1))
        assert got.std() > 1.0
        _batch_independent(s, k, got, np.uint8, layout)


def test_deliver_u8_hwc_bit_exact(hip):
    """deliver_k<2>: uint8 HWC BGR equals to_uint8 of the float32 PIXEL frame the family delivers"""
    _u8_form(hip, False)


def test_deliver_u8_chw_bit_exact(hip):
    """deliver_k<3>: uint8 planar RGB equals to_uint8 of the float32 PIXEL frame the family delivers"""
    _u8_form(hip, True)


def _yuv_form(s, formats, dtype):
    try:
        for fmt in formats:
            lay, planar, chroma, bits = chroma_ref.FORMATS[fmt]
            if bits > 8:
                _ok(s, s._lib.rrv_set_yuv_depth(s._h, 0, bits))
            layout = lay & ~(chroma_ref.FLAG["422"] | chroma_ref.FLAG["444"])
            for k, ((H, W), (DH, DW)) in enumerate(DR.SHAPES):
                rc, got = _deliver(s, k, dtype, layout, chroma=chroma)
                _ok(s, rc)
                np.testing.assert_array_equal(got, DR.yuv_ref(_pixel_out(s, k), fmt), err_msg="%s shape %d" % (fmt, k))
                if (H, W) == (DH, DW):
                    np.testing.assert_array_equal(got, DR.yuv_ref(_input(k)[0], fmt))
                assert got.std() > 1.0
                _batch_independent(s, k, got, dtype, layout, chroma=chroma)
    finally:
        if dtype == np.uint16:
            s._lib.rrv_set_yuv_depth(s._h, 0, 10)


def test_deliver_yuv8_bit_exact(hip):
    """deliver_k<4>: the six 8-bit YUV formats equal chroma_ref.yuv_ref of the float32 PIXEL frame the family delivers"""
    _yuv_form(hip, YUV8, np.uint8)


def test_deliver_yuv16_bit_exact(hip):
    """deliver_k<5>: the six 10-bit formats and a 12-bit P form equal chroma_ref.yuv_ref of the float32 PIXEL frame the family delivers"""
    _yuv_form(hip, YUV16, np.uint16)


def test_argument_errors_leave_the_handle_usable(hip):
    lib, h = hip._lib, hip._h
    (H, W), (DH, DW) = DR.SHAPES[0]
    d_in = _input(0)[1]
    v = V.contiguous(V.DT_F32, V.LAY_HWC_BGR, DH, DW)
    t = _torch()
    out = t.zeros(B * DH * DW * 3, dtype=t.float32, device="cuda")

    def call(dh, dw, view=v, src=d_in.data_ptr(), dst=out.data_ptr(), nb=B):      # (every refusal comes before any GPU work: nothing is written)
        return lib.rrv_deliver_view_device(h, C.c_void_p(src), nb, H, W, dh, dw, C.c_void_p(dst), None if view is None else C.byref(_view_struct(view)), None)
    assert call(8 * H + 1, DW) == RRV_E_ARG and b"DH" in lib.rrv_last_error(h)           # ratio beyond 8 up
    assert call(DH, 8 * W + 1) == RRV_E_ARG and b"DW" in lib.rrv_last_error(h)
    assert call(1, DW) == RRV_E_ARG and b"DH" in lib.rrv_last_error(h)                   # and down: 16 / 1
    for dh, dw in ((0, DW), (-1, DW), (DH, 0)):
        assert call(dh, dw) == RRV_E_ARG and b"DH, DW" in lib.rrv_last_error(h), (dh, dw)
    short = dict(v, pitch=[3 * DW - 1, 0, 0])                                            # an output view too small for (DH, DW)
    assert call(DH, DW, view=short) == RRV_E_ARG and b"out.pitch[0]" in lib.rrv_last_error(h)
    small = V.contiguous(V.DT_F32, V.LAY_HWC_BGR, DH - 1, DW)                            # frames one row short: they would overlap
    assert call(DH, DW, view=small) == RRV_E_ARG and b"out.frame_stride" in lib.rrv_last_error(h)
    assert call(DH, DW, view=None) == RRV_E_ARG and b"null view" in lib.rrv_last_error(h)
    assert call(DH, DW, src=None) == RRV_E_ARG and b"null buffer" in lib.rrv_last_error(h)
    assert call(DH, DW, dst=None) == RRV_E_ARG and b"null buffer" in lib.rrv_last_error(h)
    assert call(DH, DW, nb=0) == RRV_E_ARG and call(DH, DW, nb=65) == RRV_E_ARG
    assert lib.rrv_deliver_view_device(None, C.c_void_p(d_in.data_ptr()), B, H, W, DH, DW, C.c_void_p(out.data_ptr()), C.byref(_view_struct(v)), None) == RRV_E_ARG
    rc, got = _deliver(hip, 0, np.float32, V.LAY_HWC_BGR)                                # and the handle works
    _ok(hip, rc)
    assert np.abs(got - DR.float_ref(_input(0)[0], DH, DW).reshape(B, -1)).max() <= DR.tolerance("pixel", H, W, DH, DW)


def test_out_of_memory_reserving_the_working_frames(pkg, weights):
    """rrv_transfer_deliver_view_device reserves the buffer of working frames before its first launch: with the workspace and the tables
    in place, the one allocation left is that buffer; made to fail, the call is RRV_E_NOMEM and has launched nothing, and the next call
    delivers what the delivery stage makes of the plain call's float32 frames."""
    from conftest import fixed_kernels
    t = _torch()
    H, W, DH, DW = 64, 72, 96, 100
    s = pkg.Stylization(weights, cuda=True)
    try:
        s.set_state(load_golden("global_a")["state"])
        lib, h = s._lib, s._h
        u8 = _dev(np.random.default_rng(77).integers(0, 256, (B, H, W, 3)).astype(np.uint8))
        vi = _view_struct(V.contiguous(V.DT_U8, V.LAY_HWC_BGR, H, W))
        vw = _view_struct(V.contiguous(V.DT_F32, V.LAY_HWC_BGR, H, W))
        vo = _view_struct(V.contiguous(V.DT_U8, V.LAY_HWC_BGR, DH, DW))
        mid = t.zeros((B, H, W, 3), dtype=t.float32, device="cuda")
        want, got = (t.zeros((B, DH, DW, 3), dtype=t.uint8, device="cuda") for _ in range(2))
        with fixed_kernels(s, mode=0):
            for _ in range(2):      # both workspace slots hold their plans, and the handle the tables
                _ok(s, lib.rrv_transfer_view_device(h, C.c_void_p(u8.data_ptr()), C.byref(vi), B, H, W, C.c_void_p(mid.data_ptr()), C.byref(vw), L.TF_ON_STREAM, None))
            _ok(s, lib.rrv_deliver_view_device(h, C.c_void_p(mid.data_ptr()), B, H, W, DH, DW, C.c_void_p(want.data_ptr()), C.byref(vo), None))
            t.cuda.synchronize()

            def call():
                return lib.rrv_transfer_deliver_view_device(h, C.c_void_p(u8.data_ptr()), C.byref(vi), B, 0, 0, H, W, DH, DW, C.c_void_p(got.data_ptr()),
                                                            C.byref(vo), L.TF_ON_STREAM, None)
            s.profile_begin()
            s.debug_fail_alloc(1)
            assert call() == RRV_E_NOMEM and b"out of device memory" in lib.rrv_last_error(h)
            assert len(s.profile_end()) == 0
            s.debug_fail_alloc(0)
            _ok(s, call())
            t.cuda.synchronize()
            s.sync()
        assert want.float().std().item() > 1.0
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    finally:
        s.close()

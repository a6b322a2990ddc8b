"""The delivering entries (include/rerevst_hip.h "Scaling, output size"): delivery comes behind everything else, so a delivering call
equals the float32 HWC BGR PIXEL call followed by the delivery stage (tests/test_gpu_deliver.py holds it to the reference) into the form
asked for.  Everything here is compared bit for bit, in a fixed kernel mode (conftest.fixed_kernels); tiny frames."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chroma_ref
from conftest import load_golden, fixed_kernels

pytestmark = pytest.mark.gpu

RRV_OK, RRV_E_ARG = 0, -1
D = importlib.import_module("rerevst-code_amd.driver")
L = importlib.import_module("rerevst-code_amd._lib")
# (dtype, layout, chroma): a frame is H * W * 3 elements, or the samples of the YUV format
F32_HWC, U8_HWC = (L.DT_F32, L.LAY_HWC_BGR, None), (L.DT_U8, L.LAY_HWC_BGR, None)
NV12, P010, P210 = (L.DT_U8, L.LAY_NV12, "420"), (L.DT_U16, L.LAY_P016, "420"), (L.DT_U16, L.LAY_P216, "422")
_NP = {L.DT_U8: np.uint8, L.DT_F32: np.float32, L.DT_U16: np.uint16}


def _torch():
    import torch
    return torch


def _dev(a):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _desc(form):
    return L.ImageDesc(form[0], form[1], L.SP_PIXEL)


def _contig(form, H, W):
    v = L.ImageView()
    assert L.load().rrv_image_view_contiguous(_desc(form), H, W, C.byref(v)) == RRV_OK
    return v


def _frame_elems(form, H, W):
    return H * W * 3 if form[2] is None else chroma_ref.frame_samples(H, W, form[2])


def _frames(seed, form, B, H, W):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (B, _frame_elems(form, H, W))).astype(np.uint8)      # (the source forms here are 8-bit)


def _working(H, W, flags):
    return (H, W) if flags & L.TF_PAD_CROP else (H // 8 * 8, W // 8 * 8)


def _empty_out(form, B, H, W):
    t = _torch()
    return t.zeros(B * _frame_elems(form, H, W) * np.dtype(_NP[form[0]]).itemsize, dtype=t.uint8, device="cuda")


def _bytes(s, t):
    _torch().cuda.synchronize()
    s.sync()
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _ok(s, rc):
    assert rc == RRV_OK, s._lib.rrv_last_error(s._h)


def _deliver_device(s, d_in, in_form, B, src, work, dst, out_form, flags, stream=None):
    """rrv_transfer_deliver_view_device; src None: the frames are `work` (SH = SW = 0)"""
    SH, SW = (0, 0) if src is None else src
    out = _empty_out(out_form, B, *dst)
    vi, vo = _contig(in_form, *(work if src is None else src)), _contig(out_form, *dst)
    _ok(s, s._lib.rrv_transfer_deliver_view_device(s._h, C.c_void_p(d_in.data_ptr()), C.byref(vi), B, SH, SW, work[0], work[1], dst[0], dst[1],
                                                   C.c_void_p(out.data_ptr()), C.byref(vo), flags | L.TF_ON_STREAM, stream))
    return out


def _two_parts(s, d_in, in_form, B, src, work, dst, out_form, flags):
    """the float32 HWC BGR PIXEL call, then rrv_deliver_view_device on its output"""
    t = _torch()
    WH, WW = _working(*work, flags)
    mid = t.zeros((B, WH, WW, 3), dtype=t.float32, device="cuda")
    out = _empty_out(out_form, B, *dst)
    vm, vo = _contig(F32_HWC, WH, WW), _contig(out_form, *dst)
    src_p, mid_p = C.c_void_p(d_in.data_ptr()), C.c_void_p(mid.data_ptr())
    if src is None:
        vi = _contig(in_form, *work)
        _ok(s, s._lib.rrv_transfer_view_device(s._h, src_p, C.byref(vi), B, work[0], work[1], mid_p, C.byref(vm), flags | L.TF_ON_STREAM, None))
    else:
        vi = _contig(in_form, *src)
        _ok(s, s._lib.rrv_transfer_scaled_view_device(s._h, src_p, C.byref(vi), B, src[0], src[1], work[0], work[1], mid_p, C.byref(vm),
                                                      flags | L.TF_ON_STREAM, None))
    _ok(s, s._lib.rrv_deliver_view_device(s._h, mid_p, B, WH, WW, dst[0], dst[1], C.c_void_p(out.data_ptr()), C.byref(vo), None))
    return _bytes(s, out), mid


@pytest.fixture(scope="module")
def hip(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    s.set_state(load_golden("global_a")["state"])
    yield s
    s.close()


@pytest.fixture(scope="module")
def frame_model(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, use_Global=False)
    s.prepare_style(pkg.synth_style(64, 64, kind="smooth", seed=7))
    yield s
    s.close()


# name: (model, source form, source size or None, working size, delivered size, output form, flags)
COMPOSE = {
    "global_padcrop_u8_to_nv12": ("hip", U8_HWC, (96, 128), (32, 48), (96, 128), NV12, L.TF_PAD_CROP),
    "global_unscaled_to_source": ("hip", U8_HWC, None, (70, 77), (70, 77), U8_HWC, 0),
    "frame_mode_to_p010": ("frame_model", U8_HWC, None, (64, 72), (95, 127), P010, L.TF_FRAME_MODE),
    "nv12_source_to_p210": ("hip", NV12, (96, 128), (48, 64), (96, 128), P210, 0),
}


@pytest.mark.parametrize("name", sorted(COMPOSE))
def test_delivering_call_equals_float_call_then_delivery(hip, frame_model, name):
    model, in_form, src, work, dst, out_form, flags = COMPOSE[name]
    s = {"hip": hip, "frame_model": frame_model}[model]
    d_in = _dev(_frames(len(name), in_form, 3, *(work if src is None else src)))
    with fixed_kernels(s, mode=0):
        want, mid = _two_parts(s, d_in, in_form, 3, src, work, dst, out_form, flags)
        got = _bytes(s, _deliver_device(s, d_in, in_form, 3, src, work, dst, out_form, flags))
    assert mid.std().item() > 1.0 and want.std() > 1.0
    np.testing.assert_array_equal(got, want)


def test_equal_size_is_the_plain_call(hip):
    """a delivered size equal to the working frame: the plain call's bits, and no `deliver` row in the profile log"""
    H, W = 70, 77
    d_in = _dev(_frames(5, U8_HWC, 3, H, W))
    with fixed_kernels(hip, mode=0):
        plain = _empty_out(NV12, 3, 64, 72)
        vi, vo = _contig(U8_HWC, H, W), _contig(NV12, 64, 72)
        hip.profile_begin()
        _ok(hip, hip._lib.rrv_transfer_view_device(hip._h, C.c_void_p(d_in.data_ptr()), C.byref(vi), 3, H, W, C.c_void_p(plain.data_ptr()), C.byref(vo),
                                                   L.TF_ON_STREAM, None))
        rows_plain = [r[0] for r in hip.profile_end()]
        want = _bytes(hip, plain)
        hip.profile_begin()
        same = _deliver_device(hip, d_in, U8_HWC, 3, None, (H, W), (64, 72), NV12, 0)
        rows_same = [r[0] for r in hip.profile_end()]
        got = _bytes(hip, same)
        hip.profile_begin()
        _deliver_device(hip, d_in, U8_HWC, 3, None, (H, W), (70, 77), NV12, 0)
        rows_other = [r[0] for r in hip.profile_end()]
    np.testing.assert_array_equal(got, want)
    assert rows_same == rows_plain and "deliver" not in rows_same and "conv_last" in rows_same
    assert rows_other == rows_plain + ["deliver"]


def test_argument_errors(hip):
    lib, h = hip._lib, hip._h
    H, W = 64, 72
    d_in = _dev(_frames(6, U8_HWC, 2, H, W))
    out = _empty_out(F32_HWC, 2, 128, 144)

    def call(DH, DW, vo=None, flags=0, src=d_in.data_ptr(), dst=out.data_ptr()):
        vi = _contig(U8_HWC, H, W)
        vo = _contig(F32_HWC, max(DH, 1), max(DW, 1)) if vo is None else vo
        return lib.rrv_transfer_deliver_view_device(h, C.c_void_p(src), C.byref(vi), 2, 0, 0, H, W, DH, DW, C.c_void_p(dst), C.byref(vo), flags, None)
    assert call(8 * H + 1, 144) == RRV_E_ARG and b"DH" in lib.rrv_last_error(h)
    assert call(128, 8) == RRV_E_ARG and b"DW" in lib.rrv_last_error(h)          # 72 / 8 = 9
    assert call(0, 144) == RRV_E_ARG and b"DH, DW" in lib.rrv_last_error(h)
    assert call(-1, 144) == RRV_E_ARG
    assert call(128, 144, vo=_contig(F32_HWC, 127, 144)) == RRV_E_ARG and b"out.frame_stride" in lib.rrv_last_error(h)
    short = _contig(F32_HWC, 128, 144)
    short.pitch[0] -= 1
    assert call(128, 144, vo=short) == RRV_E_ARG and b"out.pitch[0]" in lib.rrv_last_error(h)
    assert call(128, 144, flags=L.TF_WEIGHTS_DEVICE) == RRV_E_ARG
    assert call(128, 144, src=None) == RRV_E_ARG and call(128, 144, dst=None) == RRV_E_ARG
    fr = _frames(6, U8_HWC, 2, H, W)
    host = np.zeros(2 * 128 * 144 * 3, np.float32)
    args = (fr.ctypes.data_as(C.c_void_p), _desc(U8_HWC), 2, 0, 0, H, W)
    assert lib.rrv_transfer_deliver(h, *args, 8 * H + 1, 144, host.ctypes.data_as(C.c_void_p), _desc(F32_HWC), 0) == RRV_E_ARG
    assert lib.rrv_transfer_deliver(h, *args, 128, 144, host.ctypes.data_as(C.c_void_p), _desc(F32_HWC), L.TF_ON_STREAM) == RRV_E_ARG
    with fixed_kernels(hip, mode=0):
        _ok(hip, call(128, 144))                                                 # the handle works
        dev = _bytes(hip, out)
        _ok(hip, lib.rrv_transfer_deliver(h, *args, 128, 144, host.ctypes.data_as(C.c_void_p), _desc(F32_HWC), 0))
    assert host.std() > 1.0
    np.testing.assert_array_equal(host.view(np.uint8), dev)


@pytest.mark.parametrize("case", (("u8", U8_HWC, None, (70, 77), (140, 150), U8_HWC, 0), ("nv12_scaled", NV12, (96, 128), (48, 64), (96, 128), NV12, L.TF_PAD_CROP),
                                  ("two_sub_batches", U8_HWC, None, (256, 328), (2048, 2624), NV12, 0)), ids=lambda c: c[0])
def test_host_entry_equals_device_entry(hip, case):
    """B = 5; the last case delivers 5.4 Mpixel frames, so the delivered-size rule cuts the call into sub-batches of 4 and 1"""
    _, in_form, src, work, dst, out_form, flags = case
    B = 5
    frames = _frames(41, in_form, B, *(work if src is None else src))
    host_out = np.zeros(B * _frame_elems(out_form, *dst), _NP[out_form[0]])
    SH, SW = (0, 0) if src is None else src
    with fixed_kernels(hip, mode=0):
        want = _bytes(hip, _deliver_device(hip, _dev(frames), in_form, B, src, work, dst, out_form, flags))
        _ok(hip, hip._lib.rrv_transfer_deliver(hip._h, frames.ctypes.data_as(C.c_void_p), _desc(in_form), B, SH, SW, work[0], work[1], dst[0], dst[1],
                                               host_out.ctypes.data_as(C.c_void_p), _desc(out_form), flags))
    assert want.std() > 1.0
    np.testing.assert_array_equal(host_out.view(np.uint8), want)


def test_stream_order_covers_the_delivery(hip):
    """on a side stream with RRV_TF_ON_STREAM, a torch op queued behind the call sees the delivered frame: the bracket covers deliver_k"""
    t = _torch()
    H, W, DH, DW = 64, 72, 512, 576
    d_in = _dev(_frames(7, U8_HWC, 3, H, W))
    with fixed_kernels(hip, mode=0):
        want = _bytes(hip, _deliver_device(hip, d_in, U8_HWC, 3, None, (H, W), (DH, DW), U8_HWC, 0))
        side = t.cuda.Stream()
        t.cuda.synchronize()
        with t.cuda.stream(side):
            out = _deliver_device(hip, d_in, U8_HWC, 3, None, (H, W), (DH, DW), U8_HWC, 0, stream=C.c_void_p(side.cuda_stream))
            seen = out.clone()
        side.synchronize()
        got = seen.cpu().numpy()
        hip.sync()
    np.testing.assert_array_equal(got, want)


def test_python_out_size(hip, pkg):
    src, work = (70, 99), (37, 51)
    u8 = _frames(91, U8_HWC, 3, *src).reshape(3, *src, 3)
    nv = _frames(92, NV12, 3, *src)
    t = _torch()
    with fixed_kernels(hip, mode=0):
        a = hip.transfer_frames(u8, work_size=work, out_size="source")
        assert a.shape == u8.shape and a.dtype == np.float32 and a.std() > 1.0
        b = hip.transfer_tensor(_dev(u8), layout="nhwc", pad_crop=True, work_size=work, out_size=src)
        np.testing.assert_array_equal(b.cpu().numpy(), a)
        # deliver_tensor on the working frames is the second half, and equals the C entry
        y = hip.transfer_tensor(_dev(u8), layout="nhwc", pad_crop=True, work_size=work)
        two = hip.deliver_tensor(y, src)
        np.testing.assert_array_equal(two.cpu().numpy(), a)
        raw = t.zeros((3,) + src + (3,), dtype=t.float32, device="cuda")
        vo = _contig(F32_HWC, *src)
        _ok(hip, hip._lib.rrv_deliver_view_device(hip._h, C.c_void_p(y.data_ptr()), 3, work[0], work[1], src[0], src[1], C.c_void_p(raw.data_ptr()), C.byref(vo),
                                                  C.c_void_p(t.cuda.current_stream().cuda_stream)))
        np.testing.assert_array_equal(raw.cpu().numpy(), two.cpu().numpy())
        q = hip.deliver_tensor(y, (80, 60), out_dtype=t.uint8, out_layout="nchw")
        assert tuple(q.shape) == (3, 3, 80, 60) and q.dtype == t.uint8
        # without work_size and without pad_crop: H x W back from 8*(H//8) x 8*(W//8)
        c = hip.transfer_batch(u8, out_size="source", dtype=np.uint8)
        assert c.shape == u8.shape and c.dtype == np.uint8
        e = hip.transfer_batch(nv, in_format="nv12", size=src, out_format="nv12", work_size=(64, 72), out_size="source")
        assert e.shape == (3, chroma_ref.frame_samples(*src, "420")) and e.dtype == np.uint8
        f = hip.transfer_tensor(_dev(nv), layout="nv12", size=src, work_size=(64, 72), out_size="source")
        np.testing.assert_array_equal(f.cpu().numpy(), e)
        canvas = t.zeros((3, src[0] + 9, src[1] + 5, 3), dtype=t.uint8, device="cuda")      # a window of a larger canvas: a strided `out`
        win = canvas[:, 4:4 + src[0], 2:2 + src[1], :]
        g = hip.transfer_tensor(_dev(u8), layout="nhwc", out=win, out_size="source")
        assert g is win
        np.testing.assert_array_equal(win.cpu().numpy(), c)
        assert int(canvas.sum().item()) == int(win.sum().item())
        # out_size=None is the call without the keyword
        np.testing.assert_array_equal(hip.transfer_frames(u8, work_size=work, out_size=None), hip.transfer_frames(u8, work_size=work))
        np.testing.assert_array_equal(hip.transfer_tensor(_dev(u8), layout="nhwc", out_size=None).cpu().numpy(), hip.transfer_tensor(_dev(u8), layout="nhwc").cpu().numpy())
    for kw in (dict(style_weights=[1.0]), dict(style_masks=np.ones((1,) + src, np.float32))):
        with pytest.raises(ValueError):
            hip.transfer_frames(u8, out_size="source", **kw)
        with pytest.raises(ValueError):
            hip.transfer_tensor(_dev(u8), layout="nhwc", out_size=src, **kw)
    with pytest.raises(ValueError):
        hip.transfer_frames(u8, out_size=(37,))
    with pytest.raises(ValueError):
        hip.transfer_tensor(_dev(u8), layout="nhwc", out=t.zeros((3, 10, 10, 3), dtype=t.uint8, device="cuda"), out_size="source")


def test_python_out_size_image_view(hip, pkg):
    """transfer_tensor(out_size=, out=ImageView): a pitched NV12 surface of the delivered size, written in place"""
    t = _torch()
    src, work = (96, 128), (48, 64)
    nv = _frames(93, NV12, 2, *src)
    pitch = 160
    rows = src[0] + src[0] // 2
    store = t.full((2 * rows * pitch,), 7, dtype=t.uint8, device="cuda")
    view = pkg.ImageView(store, "nv12", src, pitch, plane_offset=(0, src[0] * pitch), frame_stride=rows * pitch, frames=2)
    with fixed_kernels(hip, mode=0):
        want = hip.transfer_tensor(_dev(nv), layout="nv12", size=src, work_size=work, pad_crop=True, out_size="source").cpu().numpy()
        got = hip.transfer_tensor(_dev(nv), layout="nv12", size=src, work_size=work, pad_crop=True, out_size="source", out=view)
        assert got is view
        with pytest.raises(ValueError):      # the view is checked against the delivered size, not the working size
            hip.transfer_tensor(_dev(nv), layout="nv12", size=src, work_size=work, pad_crop=True, out_size=(48, 64), out=view)
    surf = store.cpu().numpy().reshape(2, rows, pitch)
    np.testing.assert_array_equal(surf[:, :, :src[1]].reshape(2, -1), want)
    assert (surf[:, :, src[1]:] == 7).all()


def test_driver_out_size_y4m(tmp_path, pkg, weights):
    """Six frames of 96 x 128 in a .y4m, --work-size 64x48 --out-size source --video out.y4m --no-frames: the header says W128 H96 and the
    frames equal transfer_frames(work_size=(48, 64), out_size="source") on the same bytes with the same frames per call."""
    H, W, WH, WW = 96, 128, 48, 64
    buf = _frames(95, NV12, 6, H, W)      # (random bytes: the plane order does not matter to the comparison; read as I420)
    src = str(tmp_path / "in.y4m")
    w = D.Y4MWriter(src, 25, W, H)
    for fr in buf:
        w.append(fr, (H, W))
    w.release()
    D.write_image_bgr(str(tmp_path / "style.png"), pkg.synth_style(64, 64, kind="smooth", seed=7))

    class Kept(pkg.Stylization):
        calls, adds = [], []

        def close(self):                      # main() closes its model; the comparison below still needs it
            pass

        def add(self, patch, **kw):
            self.adds.append((kw.get("work_size"), "out_size" in kw))
            return super().add(patch, **kw)

        def transfer_frames(self, frames, **kw):
            self.calls.append((kw.get("size"), kw.get("work_size"), kw.get("out_size")))
            return super().transfer_frames(frames, **kw)
    models = []

    def factory(args, device):
        models.append(Kept(weights, cuda=True, device=device))
        return models[-1]
    video = str(tmp_path / "out.y4m")
    with fixed_kernels():
        rc = D.main(["--style", str(tmp_path / "style.png"), "--frames", src, "--checkpoint", "synthetic", "--out", str(tmp_path / "out"),
                     "--video", video, "--no-frames", "--chunk", "4", "--work-size", "%dx%d" % (WW, WH), "--out-size", "source"], model_factory=factory)
        assert rc == 0 and Kept.calls == [((H, W), (WH, WW), (H, W))] * 2 and Kept.adds and set(Kept.adds) == {((WH, WW), False)}
        s = models[0]
        ref = [np.array(s.transfer_frames(buf[c0:c0 + 4], in_format="i420", size=(H, W), out_format="i420", work_size=(WH, WW), out_size="source"))
               for c0 in (0, 4)]
    pkg.Stylization.close(s)
    assert not (tmp_path / "out").exists()
    with D.Y4MReader(video) as r:
        assert (r.width, r.height, len(r)) == (W, H, 6)
        got = [bytes(r.read(i)) for i in range(6)]
    with open(video, "rb") as f:
        assert b" W128 H96 " in f.readline()
    assert got == [bytes(fr) for chunk in ref for fr in chunk]

"""8-bit YUV 4:2:0 input read by the first kernel (conv_first_k<IN_YUV_I420 / IN_YUV_NV12>, the rrv_*_from_yuv entries,
Stylization.transfer*(in_format= / layout=, size=), add(in_format=)).  The invariant: a YUV call's result equals, bit for bit, the
result of the float32 PIXEL BGR twin fed with the frame tests/yuv_in_ref.py makes of the same bytes — over the device entries in
every kernel mode, between the host entries and the device twin in the fixed modes 0 and 2.  Inputs are random bytes over the
full range, so the 0..255 clamp of the conversion is reached in every frame."""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest

import yuv_in_ref as R
import yuv_ref as Y
from conftest import load_golden, fixed_kernels, IMG_ATOL

pytestmark = pytest.mark.gpu

RRV_E_ARG = -1
D = importlib.import_module("rerevst-code_amd.driver")
L = importlib.import_module("rerevst-code_amd._lib")
LAYOUTS = ("i420", "nv12")
LAY = {"i420": L.LAY_I420, "nv12": L.LAY_NV12}
N601 = R.input_matrix64("bt601", False).astype(np.float32)       # the handle's default input matrix
M601 = Y.matrix64("bt601", False).astype(np.float32)             # and its default output matrix


def _kernels(mode, *handles):
    return contextlib.nullcontext() if mode == "default" else fixed_kernels(*handles, mode=mode)


def _yuv(seed, B, H, W):
    return np.random.default_rng(seed).integers(0, 256, (B, R.frame_bytes(H, W)), dtype=np.uint8)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _twin(s, bgr, pad_crop, **kw):
    """the float32 PIXEL BGR twin: transfer_tensor(layout="nhwc", space="pixel") on yuv_in_ref's frames, float32 [B][OH][OW][3]"""
    return _host(s.transfer_tensor(_dev(bgr), layout="nhwc", space="pixel", pad_crop=pad_crop, **kw))


@pytest.fixture(scope="module")
def hip(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    s.set_state(load_golden("global_a")["state"])
    yield s
    s.close()


@pytest.fixture(scope="module")
def multi(pkg, weights):
    g = load_golden("multistyle_s2")
    s = pkg.Stylization(weights, cuda=True, style_num=2)
    s.set_state(g["state0"], 0)
    s.set_state(g["state1"], 1)
    yield s
    s.close()


@pytest.fixture(scope="module")
def frame_model(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, use_Global=False)
    s.prepare_style(pkg.synth_style(64, 64, kind="smooth", seed=7))
    yield s
    s.close()


# (H, W, pad_crop): 100 x 120 plain; 53 x 75 plain (odd chroma planes, 48 x 72 out, interior and border tiles); 37 x 51 and 40 x 56
# with pad / crop (padded 192 x 192: the reflections cross chroma blocks, 37 x 51 has a ragged last chroma row and column)
SHAPES = ((100, 120, False), (53, 75, False), (37, 51, True), (40, 56, True))


def _device_case(s, seed, H, W, pad_crop, **kw):
    import torch
    buf = _yuv(seed, 3, H, W)
    OH, OW = (H, W) if pad_crop else (H // 8 * 8, W // 8 * 8)
    for layout in LAYOUTS:
        bgr = R.bgr_ref(buf, H, W, N601, layout)
        assert bgr.min() == 0.0 and bgr.max() == 255.0, "the random bytes do not reach both clamps"
        f = _twin(s, bgr, pad_crop, **kw)
        assert f.shape == (3, OH, OW, 3)
        x = _dev(buf)
        got = s.transfer_tensor(x, layout=layout, size=(H, W), out_layout="nhwc", pad_crop=pad_crop, **kw)
        assert got.dtype == torch.float32
        np.testing.assert_array_equal(_host(got), f)
        got = s.transfer_tensor(x, layout=layout, size=(H, W), out_layout="nchw", out_dtype=torch.uint8, pad_crop=pad_crop, **kw)
        np.testing.assert_array_equal(_host(got), D.to_uint8(f)[..., ::-1].transpose(0, 3, 1, 2))
        other = "nv12" if layout == "i420" else "i420"
        got = s.transfer_tensor(x, layout=layout, size=(H, W), out_layout=other, pad_crop=pad_crop, **kw)
        assert tuple(got.shape) == (3, R.frame_bytes(OH, OW)) and got.dtype == torch.uint8
        np.testing.assert_array_equal(_host(got), Y.yuv_ref(f, M601, other))
        got = s.transfer_tensor(x, layout=layout, size=(H, W), pad_crop=pad_crop, **kw)          # the same layout out: decoder to encoder
        np.testing.assert_array_equal(_host(got), Y.yuv_ref(f, M601, layout))
    if not kw:
        one = s.transfer_tensor(x[0], layout="nv12", size=(H, W), pad_crop=pad_crop)              # unbatched in, unbatched out
        assert tuple(one.shape) == (R.frame_bytes(OH, OW),)
        np.testing.assert_array_equal(_host(one), Y.yuv_ref(f[:1], M601, "nv12")[0])


@pytest.mark.parametrize("mode", (0, 2, "default"))
def test_device_entries(hip, mode):
    """rrv_transfer_from_yuv_device, both layouts, B = 3, float32 / uint8 / I420 / NV12 out, every kernel mode."""
    with _kernels(mode, hip):
        for k, (H, W, pad) in enumerate(SHAPES):
            _device_case(hip, 10 + k, H, W, pad)


def _host_case(s, pkg, seed, B, H, W, pad_crop, io_modes=(0, 1, 3), **kw):
    buf = _yuv(seed, B, H, W)
    call = s.transfer_frames if pad_crop else s.transfer_batch
    for layout in LAYOUTS:
        f = _twin(s, R.bgr_ref(buf, H, W, N601, layout), pad_crop, **kw)
        yuv = Y.yuv_ref(f, M601, "i420")
        for io in io_modes:
            s.set_host_io(io)
            for pinned in (False, True):
                src = buf
                if pinned:
                    src = pkg.pinned_empty(buf.shape, np.uint8)
                    src[...] = buf
                out = pkg.pinned_empty(f.shape, np.float32) if pinned else np.full(f.shape, -1, np.float32)
                assert call(src, out=out, in_format=layout, size=(H, W), **kw) is out
                np.testing.assert_array_equal(out, f)
                np.testing.assert_array_equal(call(src, in_format=layout, size=(H, W), out_format="i420", **kw), yuv)
        s.set_host_io(0)
        np.testing.assert_array_equal(call(buf, in_format=layout, size=(H, W), dtype=np.uint8, **kw), D.to_uint8(f))
        np.testing.assert_array_equal(call(list(buf), in_format=layout, size=(H, W), out_format="nv12", **kw), Y.yuv_ref(f, M601, "nv12"))


@pytest.mark.parametrize("mode", (0, 2))
def test_host_entries(hip, pkg, mode):
    """rrv_transfer_from_yuv: both geometries, 19 frames (two host sub-batches), every host I/O mode, pageable and page-locked."""
    with fixed_kernels(hip, mode=mode):
        _host_case(hip, pkg, 20, 3, 37, 51, True)
        _host_case(hip, pkg, 21, 3, 53, 75, False)
        _host_case(hip, pkg, 22, 19, 64, 64, False)
        _host_case(hip, pkg, 23, 19, 64, 64, True, io_modes=(0, 1))


def test_frame_mode_blend_and_mask(frame_model, multi, pkg):
    """Mode 0: RRV_TF_FRAME_MODE, per-frame style weights (host and device) and a left / right mask, device and host entries, each
    against its float twin."""
    import torch
    with fixed_kernels(frame_model, multi, mode=0):
        _device_case(frame_model, 30, 37, 51, True)
        _device_case(frame_model, 31, 53, 75, False)
        _host_case(frame_model, pkg, 32, 3, 37, 51, True, io_modes=(0, 3))
        _host_case(frame_model, pkg, 33, 19, 64, 64, False, io_modes=(0,))
        w = np.array([[1.0, 0.0], [0.25, 0.75], [0.5, 0.5]], np.float32)
        _device_case(multi, 34, 37, 51, True, style_weights=w)
        _device_case(multi, 34, 37, 51, True, style_weights=torch.from_numpy(w).cuda())
        _host_case(multi, pkg, 35, 3, 53, 75, False, io_modes=(0, 1), style_weights=w)
        w19 = np.stack([np.linspace(0, 1, 19), 1 - np.linspace(0, 1, 19)], axis=1).astype(np.float32)
        _host_case(multi, pkg, 36, 19, 64, 64, True, io_modes=(0,), style_weights=w19)
        mask = np.zeros((2, 40, 56), np.float32)
        mask[0, :, :28], mask[1, :, 28:] = 1.0, 1.0
        _device_case(multi, 37, 40, 56, True, style_masks=torch.from_numpy(mask).cuda())
        _device_case(multi, 38, 40, 56, False, style_masks=mask)
        _host_case(multi, pkg, 39, 3, 40, 56, True, io_modes=(0, 3), style_masks=mask)


@pytest.mark.parametrize("H,W,layout", [(52, 44, "i420"), (37, 51, "nv12")])
def test_add_from_yuv(pkg, weights, H, W, layout):
    """add(in_format=) + compute give the state blob of add_tensor on yuv_in_ref's frames, bit for bit; the device entry too."""
    import torch
    buf = _yuv(40 + H, 3, H, W)
    bgr = R.bgr_ref(buf, H, W, N601, layout)
    style = pkg.synth_style(64, 64, kind="smooth", seed=7)
    s = pkg.Stylization(weights, cuda=True)
    try:
        s.prepare_style(style)
        s.clean()
        s.add_tensor(_dev(bgr), space="pixel", layout="nhwc")
        s.compute()
        ref = s.get_state()
        s.clean()
        s.add(buf[:2], in_format=layout, size=(H, W))
        s.add(buf[2], in_format=layout, size=(H, W))
        s.compute()
        np.testing.assert_array_equal(s.get_state(), ref)
        s.clean()
        x = _dev(buf)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for b in range(3):
            assert s._lib.rrv_add_from_yuv_device(s._h, C.c_void_p(x[b].data_ptr()), LAY[layout], H, W, stream) == 0
        s.compute()
        np.testing.assert_array_equal(s.get_state(), ref)
        for bad in (0, 1, 4, -1):
            assert s._lib.rrv_add_from_yuv(s._h, buf.ctypes.data_as(C.c_void_p), bad, H, W) == RRV_E_ARG
        assert s._lib.rrv_add_from_yuv(s._h, None, LAY[layout], H, W) == RRV_E_ARG
        with pytest.raises(ValueError):
            s.add(buf[0], in_format=layout)
        with pytest.raises(ValueError):
            s.add(buf[0, :-1], in_format=layout, size=(H, W))
    finally:
        s.close()


def test_against_the_cpu_oracle(hip, pkg, weights, oracle):
    """One 64 x 64 I420 frame in the default mode against the CPU oracle on yuv_in_ref's frame: the every-value image bound."""
    buf = _yuv(50, 1, 64, 64)
    frame = R.bgr_ref(buf, 64, 64, N601, "i420")[0]
    ref = oracle.Stylization(weights)
    ref.set_state(load_golden("global_a")["state"])
    want = ref.transfer(frame)
    got = hip.transfer_batch(buf, in_format="i420", size=(64, 64))[0]
    err = float(np.abs(got - want).max())
    print("YUV input vs the CPU oracle: max |d| = %.4f grey levels (bound %.2f)" % (err, IMG_ATOL))
    assert got.shape == want.shape == (64, 64, 3)
    assert err <= IMG_ATOL


def test_input_matrix(hip, pkg):
    """BT.709 full range changes the result to that matrix's reference; None restores the default; NaN / inf is RRV_E_ARG and
    replaces nothing.  The output matrix is independent of it."""
    H, W = 37, 51
    buf = _yuv(60, 2, H, W)
    with fixed_kernels(hip):
        f601 = _twin(hip, R.bgr_ref(buf, H, W, N601, "i420"), True)
        n = hip.set_yuv_input_matrix("bt709", True)
        np.testing.assert_array_equal(n, R.input_matrix64("bt709", True).astype(np.float32))
        f709 = _twin(hip, R.bgr_ref(buf, H, W, n, "i420"), True)
        assert (f709 != f601).any()
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420", size=(H, W)), f709)
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420", size=(H, W), out_format="i420"), Y.yuv_ref(f709, M601, "i420"))
        for k, v in ((0, np.nan), (7, np.inf), (11, -np.inf)):
            bad = N601.reshape(-1).copy()
            bad[k] = v
            assert hip._lib.rrv_set_yuv_input_matrix(hip._h, bad.ctypes.data_as(C.POINTER(C.c_float))) == RRV_E_ARG
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420", size=(H, W)), f709)      # the refused calls replaced nothing
        custom = (R.input_matrix64("bt601", True) * 0.5).astype(np.float32)
        hip.set_yuv_input_matrix(custom)
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="nv12", size=(H, W)), _twin(hip, R.bgr_ref(buf, H, W, custom, "nv12"), True))
        np.testing.assert_array_equal(hip.set_yuv_input_matrix(None), N601)
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420", size=(H, W)), f601)
        assert hip._lib.rrv_set_yuv_input_matrix(None, None) == RRV_E_ARG


def test_nothing_outside_the_frames_is_read(hip, pkg):
    """The same frames embedded at an odd offset in two larger buffers with different surrounding bytes give identical output,
    on the device (both geometries) and through the zero-copy host path."""
    import torch
    H, W = 37, 51
    buf = _yuv(70, 3, H, W)
    n, lead = buf.size, 13
    with fixed_kernels(hip):
        for layout in LAYOUTS:
            for pad in (True, False):
                outs = []
                for fill in (0x00, 0xFF):
                    whole = torch.full((n + lead + 4096,), fill, dtype=torch.uint8, device="cuda")
                    whole[lead:lead + n] = _dev(buf).reshape(-1)
                    outs.append(_host(hip.transfer_tensor(whole[lead:lead + n].view(3, -1), layout=layout, size=(H, W), out_layout="nhwc", pad_crop=pad)))
                np.testing.assert_array_equal(outs[0], outs[1])
                np.testing.assert_array_equal(outs[0], _twin(hip, R.bgr_ref(buf, H, W, N601, layout), pad))
        hip.set_host_io(1)
        try:
            outs = []
            for fill in (0x00, 0xFF):
                whole = pkg.pinned_empty((n + lead + 4096,), np.uint8)
                whole[...] = fill
                whole[lead:lead + n] = buf.reshape(-1)
                outs.append(np.array(hip.transfer_frames(whole[lead:lead + n].reshape(3, -1), in_format="nv12", size=(H, W))))
            np.testing.assert_array_equal(outs[0], outs[1])
        finally:
            hip.set_host_io(0)


def test_errors_leave_the_handle_usable(hip, multi, pkg):
    import torch
    lib, h = hip._lib, hip._h
    H = W = 64
    buf = _yuv(80, 2, H, W)
    bgr_u8 = np.stack([pkg.synth_frame(i, H, W, kind="noise") for i in range(2)])
    d_in = _dev(buf)
    d_out = torch.zeros(2 * H * W * 3 * 4, dtype=torch.uint8, device="cuda")
    f32 = L.ImageDesc(L.DT_F32, L.LAY_HWC_BGR, L.SP_PIXEL)
    u8_i420 = L.ImageDesc(L.DT_U8, L.LAY_I420, L.SP_PIXEL)
    ip, op = C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr())
    host_out = np.zeros((2, H, W, 3), np.float32)
    hp, hop = buf.ctypes.data_as(C.c_void_p), host_out.ctypes.data_as(C.c_void_p)
    wts = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    mask = np.full((1, 2, H, W), 0.5, np.float32)
    d_mask = _dev(mask)
    mp = mask.ctypes.data_as(C.POINTER(C.c_float))
    with fixed_kernels(hip, multi):
        before_u8 = np.array(hip.transfer_batch(bgr_u8))
        before_frames = np.array(hip.transfer_frames(bgr_u8, dtype=np.uint8))
        for bad in (0, 1, 4, -1):
            assert lib.rrv_transfer_from_yuv_device(h, ip, bad, 2, H, W, op, f32, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_blend_from_yuv_device(multi._h, ip, bad, 2, H, W, wts, 2, op, f32, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_mask_from_yuv_device(multi._h, ip, bad, 2, H, W, C.c_void_p(d_mask.data_ptr()), 2, 1, op, f32, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_from_yuv(h, hp, bad, 2, H, W, hop, f32, 0) == RRV_E_ARG
            assert lib.rrv_transfer_blend_from_yuv(multi._h, hp, bad, 2, H, W, wts, 2, hop, f32, 0) == RRV_E_ARG
            assert lib.rrv_transfer_mask_from_yuv(multi._h, hp, bad, 2, H, W, mp, 2, 1, hop, f32, 0) == RRV_E_ARG
            assert lib.rrv_last_error(h)
        for hh, ww in ((7, 64), (64, 7), (0, 0)):
            for flags in (0, L.TF_PAD_CROP):
                assert lib.rrv_transfer_from_yuv_device(h, ip, L.LAY_I420, 2, hh, ww, op, f32, flags, None) == RRV_E_ARG
                assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_NV12, 2, hh, ww, hop, f32, flags) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv_device(h, None, L.LAY_I420, 2, H, W, op, f32, 0, None) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv_device(h, ip, L.LAY_I420, 2, H, W, None, f32, 0, None) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv_device(None, ip, L.LAY_I420, 2, H, W, op, f32, 0, None) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv(h, None, L.LAY_I420, 2, H, W, hop, f32, 0) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_I420, 2, H, W, None, f32, 0) == RRV_E_ARG
        for flags in (16, 32, -1):
            assert lib.rrv_transfer_from_yuv_device(h, ip, L.LAY_I420, 2, H, W, op, f32, flags, None) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv_device(h, ip, L.LAY_I420, 2, H, W, op, f32, L.TF_WEIGHTS_DEVICE, None) == RRV_E_ARG
        for flags in (L.TF_ON_STREAM, L.TF_WEIGHTS_DEVICE, 16, -1):
            assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_I420, 2, H, W, hop, f32, flags) == RRV_E_ARG
        assert lib.rrv_transfer_blend_from_yuv(multi._h, hp, L.LAY_I420, 2, H, W, wts, 2, hop, f32, L.TF_FRAME_MODE) == RRV_E_ARG
        assert lib.rrv_transfer_blend_from_yuv_device(multi._h, ip, L.LAY_I420, 2, H, W, wts, 2, op, f32, L.TF_FRAME_MODE, None) == RRV_E_ARG
        for od in (L.ImageDesc(L.DT_F32, L.LAY_I420, L.SP_PIXEL), L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_UNIT), L.ImageDesc(L.DT_F32, 4, L.SP_PIXEL)):
            assert lib.rrv_transfer_from_yuv_device(h, ip, L.LAY_I420, 2, H, W, op, od, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_I420, 2, H, W, hop, od, 0) == RRV_E_ARG
        for od in (L.ImageDesc(L.DT_F32, L.LAY_CHW_RGB, L.SP_PIXEL), L.ImageDesc(L.DT_F32, L.LAY_HWC_BGR, L.SP_UNIT)):      # host: HWC BGR PIXEL or YUV only
            assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_I420, 2, H, W, hop, od, 0) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv_device(h, ip, L.LAY_I420, 65, H, W, op, f32, 0, None) == RRV_E_ARG
        with pytest.raises(ValueError):
            hip.transfer_batch(buf, in_format="i420")
        with pytest.raises(ValueError):
            hip.transfer_frames(buf[:, :-1], in_format="i420", size=(H, W))
        with pytest.raises(ValueError):
            hip.transfer_tensor(d_in, layout="nv12")
        with pytest.raises(ValueError):
            hip.transfer_tensor(d_in[:, :-2], layout="nv12", size=(H, W))
        with pytest.raises(ValueError):
            hip.transfer_tensor(d_in, layout="i420", size=(H, W), space="unit")
        # the next valid call of each entry delivers the right bytes
        f = _twin(hip, R.bgr_ref(buf, H, W, N601, "i420"), False)
        assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_I420, 2, H, W, hop, f32, 0) == 0
        np.testing.assert_array_equal(host_out, f)
        torch.cuda.synchronize()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rrv_transfer_from_yuv_device(h, ip, L.LAY_I420, 2, H, W, op, u8_i420, L.TF_ON_STREAM, stream) == 0
        ref = Y.yuv_ref(f, M601, "i420")
        np.testing.assert_array_equal(_host(d_out[:ref.size]).reshape(ref.shape), ref)
        fb = _twin(multi, R.bgr_ref(buf, H, W, N601, "nv12"), False, style_weights=[0.5, 0.5])
        assert lib.rrv_transfer_blend_from_yuv(multi._h, hp, L.LAY_NV12, 2, H, W, wts, 2, hop, f32, 0) == 0
        np.testing.assert_array_equal(host_out, fb)
        # and the uint8 BGR calls on the same handle give the bits they gave before
        np.testing.assert_array_equal(hip.transfer_batch(bgr_u8), before_u8)
        np.testing.assert_array_equal(hip.transfer_frames(bgr_u8, dtype=np.uint8), before_frames)


def test_driver_y4m_to_y4m(tmp_path, pkg, weights):
    """Five frames of 37 x 51 in a .y4m, --video out.y4m --no-frames: out.y4m's frames equal transfer_frames(in_format="i420",
    out_format="i420") with the same frames per call (chunks of 2, 2, 1), and the header carries the input's size and rate."""
    H, W = 37, 51
    buf = _yuv(90, 5, H, W)
    src = str(tmp_path / "in.y4m")
    w = D.Y4MWriter(src, 30000 / 1001, W, H)
    for fr in buf:
        w.append(fr, (H, W))
    w.release()
    D.write_image_bgr(str(tmp_path / "style.png"), pkg.synth_style(64, 64, kind="smooth", seed=7))

    class Kept(pkg.Stylization):
        calls = []

        def close(self):                      # main() closes its model; the comparison below still needs it
            pass

        def transfer_frames(self, frames, **kw):
            self.calls.append((kw.get("in_format"), kw.get("out_format"), kw.get("size")))
            return super().transfer_frames(frames, **kw)
    models = []

    def factory(args, device):
        models.append(Kept(weights, cuda=True, device=device))
        return models[-1]
    video = str(tmp_path / "out.y4m")
    with fixed_kernels():
        rc = D.main(["--style", str(tmp_path / "style.png"), "--frames", src, "--checkpoint", "synthetic", "--out", str(tmp_path / "out"),
                     "--video", video, "--no-frames", "--chunk", "2"], model_factory=factory)
        assert rc == 0 and Kept.calls == [("i420", "i420", (H, W))] * 3
        s = models[0]
        ref = [np.array(s.transfer_frames(buf[c0:c0 + 2], in_format="i420", size=(H, W), out_format="i420")) for c0 in (0, 2, 4)]
        twin = Y.yuv_ref(_twin(s, R.bgr_ref(buf[:2], H, W, N601, "i420"), True), M601, "i420")
    pkg.Stylization.close(s)
    np.testing.assert_array_equal(ref[0], twin)
    assert not (tmp_path / "out").exists()
    with D.Y4MReader(video) as r:
        assert (r.width, r.height, r.fps, r.colorspace, r.full_range, len(r)) == (W, H, (30000, 1001), "420jpeg", False, 5)
        got = [bytes(r.read(i)) for i in range(5)]
    assert got == [bytes(fr) for chunk in ref for fr in chunk]

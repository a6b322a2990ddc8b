"""10 / 12 / 16-bit YUV 4:2:0 on the GPU (RRV_LAY_I420_16 / RRV_LAY_P016: conv_last_k's uint16 store form, conv_first_k<IN_YUV_I420_16 /
IN_YUV_P016>).  Two invariants, both bit for bit, both against tests/yuv16_ref.py:
  output  a 16-bit entry's samples are yuv16_ref of its float32 twin's output for the same frames and frames per call
  input   a 16-bit call's result is that of the float32 PIXEL BGR twin fed with yuv16_ref's frame of the same samples
Shapes: 64 x 72 plain (B = 3); 37 x 51 with pad / crop (B = 3: OH*OW and frame_samples are odd, so frame 1 and the chroma planes start
on odd samples); 52 x 45 with pad / crop (B = 2: an odd width only).  Inputs are random codes over the whole 0..2^d - 1 range, so both
clamps of the input conversion fire; P016 inputs carry random low bits."""
import ctypes as C
import importlib

import numpy as np
import pytest

import yuv16_ref as R
import yuv_ref as Y8
from conftest import load_golden, fixed_kernels

pytestmark = pytest.mark.gpu

RRV_E_ARG = -1
D = importlib.import_module("rerevst-code_amd.driver")
L = importlib.import_module("rerevst-code_amd._lib")
# format name -> (yuv16_ref's layout, RRV_LAY_*, bits)
FMT = {"i420p10": ("i420", L.LAY_I420_16, 10), "i420p12": ("i420", L.LAY_I420_16, 12), "i420p16": ("i420", L.LAY_I420_16, 16),
       "p010": ("p016", L.LAY_P016, 10), "p012": ("p016", L.LAY_P016, 12), "p016": ("p016", L.LAY_P016, 16)}
SHAPES = ((64, 72, 3, False), (37, 51, 3, True), (52, 45, 2, True))
FP = C.POINTER(C.c_float)


def M(bits, std="bt601", full=False):
    return R.matrix64(std, full, bits).astype(np.float32)


def N(bits, std="bt601", full=False):
    return R.input_matrix64(std, full, bits).astype(np.float32)


def ref_out(f, fmt, m=None):
    lay, _, bits = FMT[fmt]
    return R.yuv_ref(f, M(bits) if m is None else m, lay, bits)


def ref_in(buf, H, W, fmt, n=None):
    lay, _, bits = FMT[fmt]
    return R.bgr_ref(buf, H, W, N(bits) if n is None else n, lay, bits)


def samples(seed, B, H, W, fmt):
    lay, _, bits = FMT[fmt]
    return R.random_samples(seed, B, H, W, lay, bits)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _out_hw(H, W, pad):
    return (H, W) if pad else (H // 8 * 8, W // 8 * 8)


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


def _bgr(pkg, B, H, W):
    return np.stack([pkg.synth_frame(i, H, W, kind="noise" if i & 1 else "smooth") for i in range(B)])


def _weights(B):
    return np.stack([np.linspace(1, 0, B), np.linspace(0, 1, B)], axis=1).astype(np.float32)


def _mask(H, W):
    mask = np.zeros((2, H, W), np.float32)
    mask[0, :, :W // 2], mask[1, :, W // 2:] = 1.0, 1.0
    return mask


@pytest.mark.parametrize("H,W,B,pad", SHAPES)
def test_output_host_entries(hip, multi, frame_model, pkg, H, W, B, pad):
    """rrv_transfer_yuv (flags 0 / PAD_CROP, and FRAME_MODE on top), the blend and the mask host forms: layouts 8 and 9, depths 10, 12, 16."""
    frames = _bgr(pkg, B, H, W)
    OH, OW = _out_hw(H, W, pad)
    cases = ((hip, {}), (frame_model, {}), (multi, {"style_weights": _weights(B)}), (multi, {"style_masks": _mask(H, W)}))
    with fixed_kernels(hip, multi, frame_model, mode=0):
        for s, kw in cases:
            call = s.transfer_frames if pad else s.transfer_batch
            f = np.array(call(frames, **kw))
            assert f.shape == (B, OH, OW, 3) and f.dtype == np.float32
            for fmt in FMT:
                got = call(frames, out_format=fmt, **kw)
                assert got.dtype == np.uint16 and got.shape == (B, R.frame_samples(OH, OW))
                np.testing.assert_array_equal(got, ref_out(f, fmt), err_msg="%s %r" % (fmt, sorted(kw)))


@pytest.mark.parametrize("H,W,B,pad", SHAPES)
def test_output_device_entries(hip, multi, frame_model, pkg, H, W, B, pad):
    """The three descriptor entries with out = {RRV_DT_U16, 8 | 9, RRV_SP_PIXEL}, the frame-mode flag included."""
    import torch
    x = _dev(_bgr(pkg, B, H, W))
    OH, OW = _out_hw(H, W, pad)
    cases = ((hip, {}), (frame_model, {}), (multi, {"style_weights": _dev(_weights(B))}), (multi, {"style_masks": _dev(_mask(H, W))}))
    with fixed_kernels(hip, multi, frame_model, mode=0):
        for s, kw in cases:
            f = _host(s.transfer_tensor(x, layout="nhwc", pad_crop=pad, **kw))
            for fmt in FMT:
                got = s.transfer_tensor(x, layout="nhwc", out_layout=fmt, pad_crop=pad, **kw)
                assert got.dtype == torch.uint16 and tuple(got.shape) == (B, R.frame_samples(OH, OW))
                np.testing.assert_array_equal(_host(got), ref_out(f, fmt), err_msg="%s %r" % (fmt, sorted(kw)))
        out = torch.zeros((B, R.frame_samples(OH, OW)), dtype=torch.int16, device="cuda")       # an int16 tensor holding the same bits
        assert hip.transfer_tensor(x, layout="nhwc", out_layout="p010", pad_crop=pad, out=out) is out
        f = _host(hip.transfer_tensor(x, layout="nhwc", pad_crop=pad))
        np.testing.assert_array_equal(_host(out).view(np.uint16), ref_out(f, "p010"))
        if not pad:                                                                                # the tap works as after the float twin
            hip.transfer_tensor(x, layout="nhwc", out_layout="i420p12")
            pre = hip.preclamp(OH, OW, image=B - 1)
            hip.transfer_tensor(x, layout="nhwc", out_layout="nhwc")
            np.testing.assert_array_equal(pre, hip.preclamp(OH, OW, image=B - 1))


def test_output_zero_copy_and_pinned(hip, pkg):
    """set_host_io(1): the last kernel stores the uint16 samples straight into page-locked host memory; 19 frames = two sub-batches."""
    H, W, B = 37, 51, 19
    frames = _bgr(pkg, B, H, W)
    with fixed_kernels(hip, mode=0):
        f = np.array(hip.transfer_frames(frames))
        want = ref_out(f, "p010")
        hip.set_host_io(1)
        try:
            out = pkg.pinned_empty(want.shape, np.uint16)
            out[...] = 0xFFFF
            assert hip.transfer_frames(frames, out=out, out_format="p010") is out
            np.testing.assert_array_equal(out, want)
            np.testing.assert_array_equal(hip.transfer_frames(frames, out_format="i420p12"), ref_out(f, "i420p12"))
        finally:
            hip.set_host_io(0)
        np.testing.assert_array_equal(hip.transfer_frames(frames, out_format="p010"), want)


def test_output_matrices(hip, pkg):
    """A custom matrix, BT.709 full range, NULL = BT.601 limited at the depth in force; the 8-bit matrix is another one."""
    H, W, B = 37, 51, 2
    frames = _bgr(pkg, B, H, W)
    with fixed_kernels(hip, mode=0):
        f = np.array(hip.transfer_frames(frames))
        m = hip.set_yuv_matrix("bt709", True, bits=12)
        np.testing.assert_array_equal(m, M(12, "bt709", True))
        np.testing.assert_array_equal(hip.transfer_frames(frames, out_format="i420p12"), ref_out(f, "i420p12", m))
        np.testing.assert_array_equal(hip.transfer_frames(frames, out_format="i420"), Y8.yuv_ref(f, Y8.matrix64("bt601", False).astype(np.float32), "i420"))
        custom = (M(10, "bt601", True) * np.float32(8)).astype(np.float32)      # a gain of 8 around mid-scale: values below 0 and above 1023 for the clamp
        custom[:, 3] -= np.float32(7 * 512)
        hip.set_yuv_matrix(custom, bits=10)
        want = ref_out(f, "p010", custom)
        print("custom matrix: codes %d..%d" % ((want >> 6).min(), (want >> 6).max()))
        np.testing.assert_array_equal(hip.transfer_frames(frames, out_format="p010"), want)
        for k, v in ((0, np.nan), (7, np.inf)):
            bad = custom.reshape(-1).copy()
            bad[k] = v
            assert hip._lib.rrv_set_yuv16_matrix(hip._h, bad.ctypes.data_as(FP)) == RRV_E_ARG
        np.testing.assert_array_equal(hip.transfer_frames(frames, out_format="p010"), want)      # the refused calls replaced nothing
        assert hip._lib.rrv_set_yuv16_matrix(hip._h, None) == 0
        for fmt in ("p010", "i420p16", "p012"):      # the default follows the depth in force
            np.testing.assert_array_equal(hip.transfer_frames(frames, out_format=fmt), ref_out(f, fmt))
        np.testing.assert_array_equal(hip.set_yuv_matrix(None, bits=16), M(16))


def test_eight_bit_forms_unchanged(hip, pkg):
    """I420 / NV12 bytes are identical before and after rrv_set_yuv_depth(h, 12, 12) and rrv_set_yuv16_[input_]matrix."""
    H, W, B = 37, 51, 3
    frames = _bgr(pkg, B, H, W)
    yuv8 = np.random.default_rng(3).integers(0, 256, (B, R.frame_samples(H, W)), dtype=np.uint8)
    with fixed_kernels(hip, mode=0):
        before = [np.array(hip.transfer_frames(frames, out_format=lay)) for lay in ("i420", "nv12")]
        before_in = np.array(hip.transfer_frames(yuv8, in_format="nv12", size=(H, W), out_format="nv12"))
        assert hip._lib.rrv_set_yuv_depth(hip._h, 12, 12) == 0
        wild = (np.arange(12, dtype=np.float32) - 5).astype(np.float32)
        assert hip._lib.rrv_set_yuv16_matrix(hip._h, wild.ctypes.data_as(FP)) == 0
        assert hip._lib.rrv_set_yuv16_input_matrix(hip._h, wild.ctypes.data_as(FP)) == 0
        try:
            for lay, b in zip(("i420", "nv12"), before):
                np.testing.assert_array_equal(hip.transfer_frames(frames, out_format=lay), b)
            np.testing.assert_array_equal(hip.transfer_frames(yuv8, in_format="nv12", size=(H, W), out_format="nv12"), before_in)
        finally:
            assert hip._lib.rrv_set_yuv16_matrix(hip._h, None) == 0
            assert hip._lib.rrv_set_yuv16_input_matrix(hip._h, None) == 0
            assert hip._lib.rrv_set_yuv_depth(hip._h, 10, 10) == 0


@pytest.mark.parametrize("H,W,B,pad", SHAPES)
def test_input_device_entries(hip, multi, pkg, H, W, B, pad):
    """rrv_transfer_from_yuv_device (and its blend / mask forms) in the default kernel mode, against the float32 PIXEL twin."""
    import torch
    for k, fmt in enumerate(FMT):
        buf = samples(100 + k, B, H, W, fmt)
        bgr = ref_in(buf, H, W, fmt)
        assert bgr.min() == 0.0 and bgr.max() == 255.0, "the random codes do not reach both clamps"
        f = _host(hip.transfer_tensor(_dev(bgr), layout="nhwc", pad_crop=pad))
        got = hip.transfer_tensor(_dev(buf), layout=fmt, size=(H, W), out_layout="nhwc", pad_crop=pad)
        assert got.dtype == torch.float32
        np.testing.assert_array_equal(_host(got), f, err_msg=fmt)
        if FMT[fmt][0] == "p016" and FMT[fmt][2] < 16:      # the low bits are ignored
            clean = buf & ~np.uint16(2 ** (16 - FMT[fmt][2]) - 1)
            assert (clean != buf).any()
            np.testing.assert_array_equal(_host(hip.transfer_tensor(_dev(clean), layout=fmt, size=(H, W), out_layout="nhwc", pad_crop=pad)), f)
    with fixed_kernels(multi, mode=0):
        buf = samples(120, B, H, W, "p010")
        bgr = _dev(ref_in(buf, H, W, "p010"))
        for kw in ({"style_weights": _dev(_weights(B))}, {"style_masks": _dev(_mask(H, W))}):
            f = _host(multi.transfer_tensor(bgr, layout="nhwc", pad_crop=pad, **kw))
            got = multi.transfer_tensor(_dev(buf).view(torch.int16), layout="p010", size=(H, W), out_layout="nhwc", pad_crop=pad, **kw)
            np.testing.assert_array_equal(_host(got), f)


@pytest.mark.parametrize("mode", (0, 2))
def test_input_host_entries(hip, frame_model, multi, pkg, mode):
    """rrv_transfer_from_yuv and its blend / mask forms against the device twin, in the fixed modes; zero-copy input once."""
    with fixed_kernels(hip, frame_model, multi, mode=mode):
        for k, (H, W, B, pad) in enumerate(SHAPES):
            for j, fmt in enumerate(FMT):
                buf = samples(200 + 10 * k + j, B, H, W, fmt)
                bgr = _dev(ref_in(buf, H, W, fmt))
                models = (hip, frame_model) if j % 3 == 0 else (hip,)
                for s in models:
                    call = s.transfer_frames if pad else s.transfer_batch
                    f = _host(s.transfer_tensor(bgr, layout="nhwc", pad_crop=pad))
                    np.testing.assert_array_equal(call(buf, in_format=fmt, size=(H, W)), f, err_msg=fmt)
                    np.testing.assert_array_equal(call(list(buf), in_format=fmt, size=(H, W), dtype=np.uint8), D.to_uint8(f))
        H, W, B, pad = SHAPES[1]
        buf = samples(260, B, H, W, "i420p10")
        bgr = _dev(ref_in(buf, H, W, "i420p10"))
        for kw_h, kw_d in (({"style_weights": _weights(B)}, {"style_weights": _weights(B)}), ({"style_masks": _mask(H, W)}, {"style_masks": _mask(H, W)})):
            f = _host(multi.transfer_tensor(bgr, layout="nhwc", pad_crop=True, **kw_d))
            np.testing.assert_array_equal(multi.transfer_frames(buf, in_format="i420p10", size=(H, W), **kw_h), f)
        f = _host(hip.transfer_tensor(bgr, layout="nhwc", pad_crop=True))
        hip.set_host_io(2)
        try:
            src = pkg.pinned_empty(buf.shape, np.uint16)
            src[...] = buf
            np.testing.assert_array_equal(hip.transfer_frames(src, in_format="i420p10", size=(H, W)), f)
        finally:
            hip.set_host_io(0)


def test_input_pad_crop_is_reflect_padding_the_converted_frame(hip, pkg):
    """On the odd sizes the reflection acts on the pixel coordinates first: the result equals pad -> plain transfer -> crop of the
    converted frame (numpy 'symmetric' = cv2.BORDER_REFLECT)."""
    V = importlib.import_module("rerevst-code_amd.video")
    with fixed_kernels(hip, mode=0):
        for (H, W, B, _), fmt in zip(SHAPES[1:], ("p010", "i420p12")):
            buf = samples(300 + H, B, H, W, fmt)
            bgr = ref_in(buf, H, W, fmt)
            padded = np.stack([V.reflect_pad(fr, V.padded_size(H), V.padded_size(W)) for fr in bgr])
            want = _host(hip.transfer_tensor(_dev(padded), layout="nhwc"))[:, 64:64 + H, 64:64 + W]
            got = _host(hip.transfer_tensor(_dev(buf), layout=fmt, size=(H, W), out_layout="nhwc", pad_crop=True))
            np.testing.assert_array_equal(got, want)


def test_input_matrices(hip, pkg):
    H, W, B = 37, 51, 2
    with fixed_kernels(hip, mode=0):
        buf = samples(400, B, H, W, "i420p12")
        twin = lambda n, fmt="i420p12", b=buf: _host(hip.transfer_tensor(_dev(ref_in(b, H, W, fmt, n)), layout="nhwc", pad_crop=True))
        n = hip.set_yuv_input_matrix("bt709", True, bits=12)
        np.testing.assert_array_equal(n, N(12, "bt709", True))
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420p12", size=(H, W)), twin(n))
        custom = (N(12, "bt601", True) * np.float32(0.5)).astype(np.float32)
        hip.set_yuv_input_matrix(custom, bits=12)
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420p12", size=(H, W)), twin(custom))
        bad = custom.reshape(-1).copy()
        bad[3] = np.nan
        assert hip._lib.rrv_set_yuv16_input_matrix(hip._h, bad.ctypes.data_as(FP)) == RRV_E_ARG
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420p12", size=(H, W)), twin(custom))
        np.testing.assert_array_equal(hip.set_yuv_input_matrix(None, bits=12), N(12))
        np.testing.assert_array_equal(hip.transfer_frames(buf, in_format="i420p12", size=(H, W)), twin(None))
        b16 = samples(401, B, H, W, "p016")       # NULL: the default follows the depth in force
        np.testing.assert_array_equal(hip.transfer_frames(b16, in_format="p016", size=(H, W)), twin(None, "p016", b16))


@pytest.mark.parametrize("H,W,fmt", [(52, 44, "i420p10"), (37, 51, "p012")])
def test_add_from_yuv(pkg, weights, H, W, fmt):
    """add(in_format=) + compute give the state of add_tensor (rrv_add_image_device) on the converted float frames; the device entry too."""
    import torch
    buf = samples(500 + H, 3, H, W, fmt)
    bgr = ref_in(buf, H, W, fmt)
    s = pkg.Stylization(weights, cuda=True)
    try:
        s.prepare_style(pkg.synth_style(64, 64, kind="smooth", seed=7))
        s.clean()
        s.add_tensor(_dev(bgr), space="pixel", layout="nhwc")
        s.compute()
        ref = s.get_state()
        s.clean()
        s.add(buf[:2], in_format=fmt, size=(H, W))
        s.add(buf[2], in_format=fmt, size=(H, W))
        s.compute()
        np.testing.assert_array_equal(s.get_state(), ref)
        s.clean()
        x = _dev(buf)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for b in range(3):
            assert s._lib.rrv_add_from_yuv_device(s._h, C.c_void_p(x[b].data_ptr()), FMT[fmt][1], H, W, stream) == 0
        s.compute()
        np.testing.assert_array_equal(s.get_state(), ref)
        for bad in (4, 5, 6, 7, 10):
            assert s._lib.rrv_add_from_yuv(s._h, buf.ctypes.data_as(C.c_void_p), bad, H, W) == RRV_E_ARG
        with pytest.raises(ValueError):
            s.add(buf[0].astype(np.uint8), in_format=fmt, size=(H, W))
    finally:
        s.close()


def test_both_ends(hip, pkg):
    """P010 -> P010 (decoder to encoder) and i420p10 -> 8-bit NV12, through transfer_frames and transfer_tensor."""
    import torch
    H, W, B = 37, 51, 3
    m8 = Y8.matrix64("bt601", False).astype(np.float32)
    with fixed_kernels(hip, mode=0):
        for fmt, out_fmt in (("p010", "p010"), ("i420p10", "nv12")):
            buf = samples(600, B, H, W, fmt)
            f = _host(hip.transfer_tensor(_dev(ref_in(buf, H, W, fmt)), layout="nhwc", pad_crop=True))
            want = ref_out(f, out_fmt) if out_fmt in FMT else Y8.yuv_ref(f, m8, out_fmt)
            got = hip.transfer_frames(buf, in_format=fmt, size=(H, W), out_format=out_fmt)
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want)
            t = hip.transfer_tensor(_dev(buf), layout=fmt, size=(H, W), out_layout=out_fmt, pad_crop=True)
            assert t.dtype == (torch.uint16 if out_fmt in FMT else torch.uint8)
            np.testing.assert_array_equal(_host(t), want)
        buf = samples(601, B, H, W, "p010")
        t = hip.transfer_tensor(_dev(buf), layout="p010", size=(H, W), pad_crop=True)          # out_layout defaults to the input's
        f = _host(hip.transfer_tensor(_dev(ref_in(buf, H, W, "p010")), layout="nhwc", pad_crop=True))
        np.testing.assert_array_equal(_host(t), ref_out(f, "p010"))
        frames = _bgr(pkg, B, H, W)                                                                # 8-bit in -> 10-bit out
        yuv8 = Y8.yuv_ref(frames.astype(np.float32), m8, "nv12")
        f8 = np.array(hip.transfer_frames(yuv8, in_format="nv12", size=(H, W)))
        np.testing.assert_array_equal(hip.transfer_frames(yuv8, in_format="nv12", size=(H, W), out_format="i420p10"), ref_out(f8, "i420p10"))


def test_errors_leave_the_handle_usable(hip, multi, pkg):
    import torch
    lib, h = hip._lib, hip._h
    H = W = 64
    B = 2
    n = R.frame_samples(H, W)
    buf = samples(700, B, H, W, "p010")
    bgr_u8 = _bgr(pkg, B, H, W)
    d_yuv, d_bgr = _dev(buf), _dev(bgr_u8)
    d_out = torch.zeros(B * H * W * 3 * 4, dtype=torch.uint8, device="cuda")
    yp, bp, op = C.c_void_p(d_yuv.data_ptr()), C.c_void_p(d_bgr.data_ptr()), C.c_void_p(d_out.data_ptr())
    desc = L.ImageDesc
    u8_bgr, f32 = desc(L.DT_U8, L.LAY_HWC_BGR, L.SP_PIXEL), desc(L.DT_F32, L.LAY_HWC_BGR, L.SP_PIXEL)
    good16 = desc(L.DT_U16, L.LAY_P016, L.SP_PIXEL)
    host_out = np.zeros((B, n), np.uint16)
    hp, hop, fp = buf.ctypes.data_as(C.c_void_p), host_out.ctypes.data_as(C.c_void_p), bgr_u8.ctypes.data_as(C.c_void_p)
    wts = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    d_mask = _dev(np.full((1, 2, H, W), 0.5, np.float32))
    bad_out = [desc(L.DT_U16, L.LAY_HWC_BGR, L.SP_PIXEL), desc(L.DT_U16, L.LAY_CHW_RGB, L.SP_PIXEL), desc(L.DT_U16, L.LAY_I420, L.SP_PIXEL),
               desc(L.DT_U16, L.LAY_I420_16, L.SP_UNIT), desc(L.DT_U16, L.LAY_P016, L.SP_NORM),
               desc(L.DT_U8, L.LAY_I420_16, L.SP_PIXEL), desc(L.DT_F32, L.LAY_P016, L.SP_PIXEL), desc(L.DT_U8, L.LAY_P016, L.SP_PIXEL),
               desc(L.DT_U16, 5, L.SP_PIXEL), desc(L.DT_U8, 6, L.SP_PIXEL), desc(L.DT_U16, 7, L.SP_PIXEL), desc(L.DT_U8, 4, L.SP_PIXEL),
               desc(3, L.LAY_I420_16, L.SP_PIXEL)]
    with fixed_kernels(hip, multi, mode=0):
        f = np.array(hip.transfer_batch(bgr_u8))
        assert lib.rrv_set_yuv_depth(h, 10, 10) == 0 and lib.rrv_set_yuv_depth(h, 0, 0) == 0      # (0 leaves a side as it is)
        for od in bad_out:
            assert lib.rrv_transfer_image_device(h, bp, u8_bgr, B, H, W, op, od, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_image_blend_device(multi._h, bp, u8_bgr, B, H, W, wts, 2, op, od, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_image_mask_device(multi._h, bp, u8_bgr, B, H, W, C.c_void_p(d_mask.data_ptr()), 2, 1, op, od, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_from_yuv_device(h, yp, L.LAY_P016, B, H, W, op, od, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_P016, B, H, W, hop, od, 0) == RRV_E_ARG
            assert lib.rrv_last_error(h)
        for lay in (L.LAY_I420_16, L.LAY_P016):           # layouts 8 / 9 as a descriptor INPUT
            for dt in (L.DT_U16, L.DT_U8):
                assert lib.rrv_transfer_image_device(h, yp, desc(dt, lay, L.SP_PIXEL), B, H, W, op, f32, 0, None) == RRV_E_ARG
                assert lib.rrv_add_image_device(h, yp, desc(dt, lay, L.SP_PIXEL), H, W, None) == RRV_E_ARG
        assert lib.rrv_transfer_image_device(h, yp, desc(L.DT_U16, L.LAY_HWC_BGR, L.SP_PIXEL), B, H, W, op, f32, 0, None) == RRV_E_ARG
        for lay in (4, 5, 6, 7, 10, -1):
            assert lib.rrv_transfer_yuv(h, fp, B, H, W, 0, lay, hop) == RRV_E_ARG
            assert lib.rrv_transfer_blend_batch_yuv(multi._h, fp, B, H, W, wts, 2, 0, lay, hop) == RRV_E_ARG
            assert lib.rrv_transfer_from_yuv_device(h, yp, lay, B, H, W, op, f32, 0, None) == RRV_E_ARG
            assert lib.rrv_transfer_from_yuv(h, hp, lay, B, H, W, hop, good16, 0) == RRV_E_ARG
        for a, b in ((9, 10), (10, 9), (8, 8), (14, 0), (-10, 10), (0, 17)):
            assert lib.rrv_set_yuv_depth(h, a, b) == RRV_E_ARG
        nan = M(10).reshape(-1).copy()
        nan[5] = np.nan
        assert lib.rrv_set_yuv16_matrix(h, nan.ctypes.data_as(FP)) == RRV_E_ARG
        assert lib.rrv_set_yuv16_input_matrix(h, nan.ctypes.data_as(FP)) == RRV_E_ARG
        assert lib.rrv_transfer_yuv(h, None, B, H, W, 0, L.LAY_P016, hop) == RRV_E_ARG
        assert lib.rrv_transfer_yuv(h, fp, B, H, W, 0, L.LAY_P016, None) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv_device(h, None, L.LAY_P016, B, H, W, op, good16, 0, None) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv_device(h, yp, L.LAY_P016, B, H, W, None, good16, 0, None) == RRV_E_ARG
        assert lib.rrv_transfer_from_yuv(h, None, L.LAY_I420_16, B, H, W, hop, good16, 0) == RRV_E_ARG
        with pytest.raises(ValueError):
            hip.transfer_batch(bgr_u8, out_format="i420p14")
        with pytest.raises(ValueError):
            hip.transfer_batch(bgr_u8, out_format="p010", out=np.zeros((B, n), np.uint8))
        with pytest.raises(ValueError):
            hip.transfer_frames(buf.astype(np.uint8), in_format="p010", size=(H, W))
        with pytest.raises(ValueError):
            hip.transfer_tensor(d_yuv.view(torch.uint8), layout="p010", size=(H, W))
        with pytest.raises(ValueError):
            hip.transfer_tensor(d_bgr, layout="nhwc", out_layout="p010", out_dtype=torch.uint8)
        with pytest.raises(ValueError):
            hip.transfer_tensor(d_bgr, layout="nhwc", out_layout="i420p10", out_space="unit")
        # every refused call left the depth (10), the matrices and the handle as they were: the next good calls deliver the right samples
        assert lib.rrv_transfer_yuv(h, fp, B, H, W, 0, L.LAY_P016, hop) == 0
        np.testing.assert_array_equal(host_out, ref_out(f, "p010"))
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rrv_transfer_image_device(h, bp, u8_bgr, B, H, W, op, desc(L.DT_U16, L.LAY_I420_16, L.SP_PIXEL), L.TF_ON_STREAM, stream) == 0
        got = _host(d_out[:2 * B * n]).view(np.uint16).reshape(B, n)
        np.testing.assert_array_equal(got, ref_out(f, "i420p10"))
        fin = _host(hip.transfer_tensor(_dev(ref_in(buf, H, W, "p010")), layout="nhwc"))
        assert lib.rrv_transfer_from_yuv(h, hp, L.LAY_P016, B, H, W, hop, good16, 0) == 0
        np.testing.assert_array_equal(host_out, ref_out(fin, "p010"))
        np.testing.assert_array_equal(hip.transfer_batch(bgr_u8), f)


def test_driver_y4m_p10_to_y4m_p10(tmp_path, pkg, weights):
    """Four frames of 80 x 48 in a C420p10 .y4m, --video out.y4m --no-frames: the output keeps the input's depth and its frames equal
    transfer_frames(in_format="i420p10", out_format="i420p10") with the same frames per call."""
    H, W = 48, 80
    buf = samples(800, 4, H, W, "i420p10")
    src = str(tmp_path / "in.y4m")
    w = D.Y4MWriter(src, 25, W, H, bits=10)
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
                     "--video", video, "--no-frames", "--chunk", "3"], model_factory=factory)
        assert rc == 0 and Kept.calls == [("i420p10", "i420p10", (H, W))] * 2
        s = models[0]
        ref = [np.array(s.transfer_frames(buf[c0:c0 + 3], in_format="i420p10", size=(H, W), out_format="i420p10")) for c0 in (0, 3)]
        f = _host(s.transfer_tensor(_dev(ref_in(buf[:3], H, W, "i420p10")), layout="nhwc", pad_crop=True))
    pkg.Stylization.close(s)
    np.testing.assert_array_equal(ref[0], ref_out(f, "i420p10"))
    assert not (tmp_path / "out").exists()
    with D.Y4MReader(video, high_depth=True) as r:
        assert (r.width, r.height, r.fps, r.colorspace, r.bits, r.full_range, len(r)) == (W, H, (25, 1), "420p10", 10, False, 4)
        got = np.stack([r.read(i) for i in range(4)])
    np.testing.assert_array_equal(got, np.concatenate(ref))
    assert int(got.max()) <= 1023

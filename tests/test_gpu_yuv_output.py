"""8-bit YUV 4:2:0 output converted in the last kernel (the rrv_*_yuv host entries, out.layout = RRV_LAY_I420 / RRV_LAY_NV12 on the
descriptor entries, Stylization.transfer*(out_format= / out_layout=)).  The invariant: a YUV call's bytes equal tests/yuv_ref.py
applied to the float32 twin's output for the same frames, entry and frames per call, bit for bit, in the fixed kernel modes 0 and
2 and in the default mode; nothing is stored outside the B * frame_bytes bytes and every byte inside is written."""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest

import yuv_ref as Y
from conftest import load_golden, fixed_kernels

pytestmark = pytest.mark.gpu

RRV_E_ARG = -1
D = importlib.import_module("rerevst-code_amd.driver")
L = importlib.import_module("rerevst-code_amd._lib")
MODES = (0, 2, "default")
LAYOUTS = ("i420", "nv12")
BT601 = Y.matrix64("bt601", False).astype(np.float32)        # the handle's default
TAIL, SENTINEL = 256, 0xA5


def _kernels(mode, *handles):
    return contextlib.nullcontext() if mode == "default" else fixed_kernels(*handles, mode=mode)


def _noise(pkg, seed, n, H, W):
    return np.stack([pkg.synth_frame(seed + i, H, W, kind="noise" if i % 2 else "smooth") for i in range(n)])


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


def _guarded(pkg, ref, pinned):
    """(whole buffer, the [B][frame_bytes] view to hand in): every byte inside differs from the reference, the tail is a sentinel"""
    n = ref.size
    whole = pkg.pinned_empty((n + TAIL,), np.uint8) if pinned else np.empty(n + TAIL, np.uint8)
    whole[:n] = ref.reshape(-1) ^ 0xFF
    whole[n:] = SENTINEL
    return whole, whole[:n].reshape(ref.shape)


def _check_guarded(whole, ref):
    n = ref.size
    np.testing.assert_array_equal(whole[:n].reshape(ref.shape), ref)          # every byte written, each the reference's
    assert (whole[n:] == SENTINEL).all(), "bytes behind the last frame were written"


def _host_case(s, pkg, call, frames, io_modes=(0, 1, 3), **kw):
    """`call` = s.transfer_batch / s.transfer_frames: float32 twin once, then both layouts x host_io x pageable / page-locked out"""
    f = call(frames, **kw)
    B, OH, OW, _ = f.shape
    for layout in LAYOUTS:
        ref = Y.yuv_ref(f, BT601, layout)
        assert ref.shape == (B, pkg.yuv_frame_bytes(OH, OW))
        for io in io_modes:
            s.set_host_io(io)
            for pinned in (False, True):
                whole, out = _guarded(pkg, ref, pinned)
                assert call(frames, out=out, out_format=layout, **kw) is out
                _check_guarded(whole, ref)
        s.set_host_io(0)
        got = call(frames, out_format=layout, **kw)                          # the library's own output array
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, ref)
    return f


@pytest.mark.parametrize("mode", MODES)
def test_global_host_entries(hip, pkg, mode):
    """rrv_transfer_yuv: 3 frames of 100 x 437 in the plain geometry (96 x 432 out), 3 of 37 x 51 with pad / crop (both odd: a ragged
    last chroma row, column and corner, 37 x 51 + 2 x 19 x 26 bytes per frame), 19 of 64 x 64 (more than one host sub-batch)."""
    with _kernels(mode, hip):
        f = _host_case(hip, pkg, hip.transfer_batch, _noise(pkg, 10, 3, 100, 437))
        assert f.shape == (3, 96, 432, 3)
        f = _host_case(hip, pkg, hip.transfer_frames, _noise(pkg, 20, 3, 37, 51))
        assert f.shape == (3, 37, 51, 3)
        _host_case(hip, pkg, hip.transfer_batch, _noise(pkg, 30, 19, 64, 64))
        _host_case(hip, pkg, hip.transfer_frames, _noise(pkg, 30, 19, 64, 64), io_modes=(0, 1))


@pytest.mark.parametrize("mode", (0, "default"))
def test_frame_mode_blend_and_mask_host_entries(frame_model, multi, pkg, mode):
    """rrv_transfer_yuv with RRV_TF_FRAME_MODE, rrv_transfer_blend_batch_yuv and rrv_transfer_mask_batch_yuv, both geometries; 19
    frames in frame mode and blended: two launch sequences of the grouped models."""
    odd, many = _noise(pkg, 40, 3, 37, 51), _noise(pkg, 50, 19, 64, 64)
    with _kernels(mode, frame_model, multi):
        _host_case(frame_model, pkg, frame_model.transfer_frames, odd, io_modes=(0, 3))
        _host_case(frame_model, pkg, frame_model.transfer_batch, many, io_modes=(0,))
        w = np.stack([np.linspace(0, 1, 19), 1 - np.linspace(0, 1, 19)], axis=1).astype(np.float32)
        _host_case(multi, pkg, multi.transfer_batch, many, io_modes=(0, 1), style_weights=w)
        _host_case(multi, pkg, multi.transfer_frames, odd, io_modes=(0,), style_weights=[0.3, 0.7])
        mask = np.zeros((2, 37, 51), np.float32)
        mask[0, :, :25], mask[1, :, 25:] = 1.0, 1.0
        _host_case(multi, pkg, multi.transfer_frames, odd, io_modes=(0, 3), style_masks=mask)


def _tensor_case(s, x, H, W, pad_crop, **kw):
    """transfer_tensor on NCHW float UNIT input: the float32 NHWC BGR PIXEL twin, then both layouts into guarded device buffers"""
    import torch
    f = s.transfer_tensor(x, space="unit", out_layout="nhwc", pad_crop=pad_crop, **kw)
    torch.cuda.synchronize()
    f = f.cpu().numpy()
    B = f.shape[0]
    OH, OW = (H, W) if pad_crop else (H // 8 * 8, W // 8 * 8)
    assert f.shape == (B, OH, OW, 3)
    fb = Y.frame_bytes(OH, OW)
    for layout in LAYOUTS:
        ref = Y.yuv_ref(f, BT601, layout)
        whole = torch.empty(B * fb + TAIL, dtype=torch.uint8, device="cuda")
        whole[:B * fb] = torch.from_numpy(ref.reshape(-1) ^ 0xFF).cuda()
        whole[B * fb:] = SENTINEL
        out = whole[:B * fb].view(B, fb)
        assert s.transfer_tensor(x, space="unit", out_layout=layout, pad_crop=pad_crop, out=out, **kw) is out
        torch.cuda.synchronize()
        _check_guarded(whole.cpu().numpy(), ref)
    got = s.transfer_tensor(x[0], space="unit", out_layout="i420", pad_crop=pad_crop,
                            **{k: (v[0] if k == "style_weights" and getattr(v, "ndim", 1) == 2 else v) for k, v in kw.items() if k != "style_masks"})
    assert tuple(got.shape) == (fb,) and got.dtype == torch.uint8                      # unbatched in, unbatched out
    return f


def _unit_nchw(frames):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(frames[..., ::-1])).cuda().permute(0, 3, 1, 2).float() / 255.0).contiguous()


@pytest.mark.parametrize("mode", MODES)
def test_descriptor_entries(hip, multi, frame_model, pkg, mode):
    """rrv_transfer_image_device / _blend_device / _mask_device with out.layout = I420 / NV12: NCHW float UNIT input; style weights
    (B = 3, S = 2, host and device); a left / right mask; RRV_TF_FRAME_MODE; RRV_TF_PAD_CROP at 40 x 56 and 37 x 51."""
    import torch
    a, b, c = _noise(pkg, 60, 3, 100, 120), _noise(pkg, 70, 3, 40, 56), _noise(pkg, 80, 3, 37, 51)
    with _kernels(mode, hip, multi, frame_model):
        _tensor_case(hip, _unit_nchw(a), 100, 120, False)
        _tensor_case(hip, _unit_nchw(b), 40, 56, True)
        _tensor_case(hip, _unit_nchw(c), 37, 51, True)
        _tensor_case(frame_model, _unit_nchw(b), 40, 56, False)
        _tensor_case(frame_model, _unit_nchw(c), 37, 51, True)
        w = np.array([[1.0, 0.0], [0.25, 0.75], [0.5, 0.5]], np.float32)
        f_host = _tensor_case(multi, _unit_nchw(c), 37, 51, True, style_weights=w)
        f_dev = _tensor_case(multi, _unit_nchw(c), 37, 51, True, style_weights=torch.from_numpy(w).cuda())
        np.testing.assert_array_equal(f_host, f_dev)
        mask = np.zeros((2, 40, 56), np.float32)
        mask[0, :, :28], mask[1, :, 28:] = 1.0, 1.0
        _tensor_case(multi, _unit_nchw(b), 40, 56, False, style_masks=torch.from_numpy(mask).cuda())
        _tensor_case(multi, _unit_nchw(b), 40, 56, True, style_masks=mask)


def test_matrices(hip, pkg):
    """The four standard matrices, one with every coefficient doubled (the nine multipliers of R, G, B; the offsets stay, so chroma
    is 128 + twice the colour difference and both clamps are reached), and NULL = the default again.  Frames whose stylized form
    has a Cb near 35 and luma above 128: the CPU oracle's output for them reaches 0 and 255 with a wide margin."""
    frames = np.stack([pkg.synth_frame(4, 37, 51, kind="smooth"), pkg.synth_frame(7, 37, 51, kind="noise")])
    with fixed_kernels(hip):
        f = hip.transfer_frames(frames)
        for standard in ("bt601", "bt709"):
            for full in (False, True):
                m = hip.set_yuv_matrix(standard, full)
                np.testing.assert_array_equal(m, Y.matrix64(standard, full).astype(np.float32))
                for layout in LAYOUTS:
                    np.testing.assert_array_equal(hip.transfer_frames(frames, out_format=layout), Y.yuv_ref(f, m, layout))
        big = Y.matrix64("bt709", True)
        big[:, :3] *= 2
        big = big.astype(np.float32)
        hip.set_yuv_matrix(big)
        ref = Y.yuv_ref(f, big, "i420")
        assert (ref == 0).any() and (ref == 255).any(), "the doubled matrix does not reach both clamps on these frames"
        np.testing.assert_array_equal(hip.transfer_frames(frames, out_format="i420"), ref)
        assert hip._lib.rrv_set_yuv_matrix(hip._h, None) == 0
        got = hip.transfer_frames(frames, out_format="nv12")
        np.testing.assert_array_equal(got, Y.yuv_ref(f, BT601, "nv12"))
        assert (got != Y.yuv_ref(f, big, "nv12")).any()
        hip.set_yuv_matrix("bt709", True)
        np.testing.assert_array_equal(hip.set_yuv_matrix(None), BT601)


def test_existing_forms_are_untouched(hip, pkg):
    """float32, I420, float32, uint8 on one handle: the float outputs are the same bits, uint8 == to_uint8(float), and the pre-clamp
    tap after the YUV call is the float call's."""
    frames = _noise(pkg, 100, 2, 100, 150)
    with fixed_kernels(hip):
        f0 = np.array(hip.transfer_batch(frames))
        pre = np.array(hip.preclamp(96, 144, image=1))
        yuv = hip.transfer_batch(frames, out_format="i420")
        np.testing.assert_array_equal(hip.preclamp(96, 144, image=1), pre)
        f1 = hip.transfer_batch(frames)
        np.testing.assert_array_equal(f1, f0)
        np.testing.assert_array_equal(hip.transfer_batch(frames, dtype=np.uint8), D.to_uint8(f0))
        np.testing.assert_array_equal(yuv, Y.yuv_ref(f0, BT601, "i420"))
        y, cb, cr = pkg.yuv_planes(yuv, 96, 144, "i420")
        assert y.shape == (2, 96, 144) and cb.shape == cr.shape == (2, 48, 72)


def test_errors_leave_the_handle_usable(hip, multi, pkg):
    import torch
    lib, h = hip._lib, hip._h
    frames = _noise(pkg, 110, 2, 64, 64)
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.zeros(2 * 64 * 64 * 3 * 4, dtype=torch.uint8, device="cuda")
    u8_bgr = L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_PIXEL)

    def image(in_desc, out_desc):
        return lib.rrv_transfer_image_device(h, C.c_void_p(d_in.data_ptr()), in_desc, 2, 64, 64, C.c_void_p(d_out.data_ptr()), out_desc, 0, None)
    assert image(u8_bgr, L.ImageDesc(L.DT_F32, L.LAY_I420, L.SP_PIXEL)) == RRV_E_ARG
    assert image(u8_bgr, L.ImageDesc(L.DT_F32, L.LAY_NV12, L.SP_PIXEL)) == RRV_E_ARG
    assert image(u8_bgr, L.ImageDesc(L.DT_U8, L.LAY_I420, L.SP_UNIT)) == RRV_E_ARG
    assert image(u8_bgr, L.ImageDesc(L.DT_F32, L.LAY_I420, L.SP_UNIT)) == RRV_E_ARG
    assert image(u8_bgr, L.ImageDesc(L.DT_F32, L.LAY_NV12, L.SP_NORM)) == RRV_E_ARG
    assert image(L.ImageDesc(L.DT_U8, L.LAY_I420, L.SP_PIXEL), u8_bgr) == RRV_E_ARG
    assert image(L.ImageDesc(L.DT_U8, L.LAY_NV12, L.SP_PIXEL), u8_bgr) == RRV_E_ARG
    assert image(u8_bgr, L.ImageDesc(L.DT_U8, 4, L.SP_PIXEL)) == RRV_E_ARG
    assert image(u8_bgr, L.ImageDesc(L.DT_U8, -1, L.SP_PIXEL)) == RRV_E_ARG
    assert image(u8_bgr, L.ImageDesc(L.DT_U8, L.LAY_I420, L.SP_PIXEL)) == 0            # the valid form of the same call
    out = np.zeros((2, Y.frame_bytes(64, 64)), np.uint8)
    fp, op = frames.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    wts = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    mask = np.full((1, 2, 64, 64), 0.5, np.float32)
    mp = mask.ctypes.data_as(C.POINTER(C.c_float))
    for bad in (L.LAY_HWC_BGR, L.LAY_CHW_RGB, 4, -1):
        assert lib.rrv_transfer_yuv(h, fp, 2, 64, 64, 0, bad, op) == RRV_E_ARG
        assert lib.rrv_transfer_blend_batch_yuv(multi._h, fp, 2, 64, 64, wts, 2, 0, bad, op) == RRV_E_ARG
        assert lib.rrv_transfer_mask_batch_yuv(multi._h, fp, 2, 64, 64, mp, 2, 1, 0, bad, op) == RRV_E_ARG
    for flags in (L.TF_ON_STREAM, L.TF_WEIGHTS_DEVICE, 16, -1):
        assert lib.rrv_transfer_yuv(h, fp, 2, 64, 64, flags, L.LAY_I420, op) == RRV_E_ARG
    assert lib.rrv_transfer_yuv(h, fp, 2, 64, 64, 0, L.LAY_I420, None) == RRV_E_ARG
    assert lib.rrv_transfer_yuv(None, fp, 2, 64, 64, 0, L.LAY_I420, op) == RRV_E_ARG
    for k, v in ((0, np.nan), (7, np.inf), (11, -np.inf)):
        m = BT601.reshape(-1).copy()
        m[k] = v
        assert lib.rrv_set_yuv_matrix(h, m.ctypes.data_as(C.POINTER(C.c_float))) == RRV_E_ARG
    with pytest.raises(ValueError):
        hip.transfer_batch(frames, out_format="yv12")
    with pytest.raises(ValueError):
        hip.transfer_batch(frames, out_format="i420", out=np.zeros((2, 64, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        hip.transfer_tensor(d_in, layout="nhwc", out_layout="i420", out_space="unit")
    with pytest.raises(ValueError):
        hip.transfer_tensor(d_in, layout="nhwc", out_layout="i420", out_dtype=torch.float32)
    # the next valid call of each entry delivers the right bytes, with the matrix the refused calls did not replace
    with fixed_kernels(hip, multi):
        ref = Y.yuv_ref(hip.transfer_batch(frames), BT601, "i420")
        assert lib.rrv_transfer_yuv(h, fp, 2, 64, 64, 0, L.LAY_I420, op) == 0
        np.testing.assert_array_equal(out, ref)
        torch.cuda.synchronize()
        assert image(u8_bgr, L.ImageDesc(L.DT_U8, L.LAY_I420, L.SP_PIXEL)) == 0
        hip.sync()
        np.testing.assert_array_equal(d_out[:ref.size].cpu().numpy().reshape(ref.shape), ref)
        f = multi.transfer_batch(frames, style_weights=[0.5, 0.5])
        assert lib.rrv_transfer_blend_batch_yuv(multi._h, fp, 2, 64, 64, wts, 2, 0, L.LAY_NV12, op) == 0
        np.testing.assert_array_equal(out, Y.yuv_ref(f, BT601, "nv12"))


def test_driver_writes_the_gpu_bytes(tmp_path, pkg, weights):
    """--no-frames --video out.y4m: the file parses, holds no image files next to it, and its frames are yuv_ref of transfer_frames'
    float output with the same frames per call (chunks of 2, 2, 1)."""
    src = tmp_path / "in"
    src.mkdir()
    frames = np.stack([pkg.synth_frame(i, 48, 80, kind="smooth") for i in range(5)])
    for i, f in enumerate(frames):
        D.write_image_bgr(str(src / ("f%02d.png" % i)), f)
    D.write_image_bgr(str(tmp_path / "style.png"), pkg.synth_style(64, 64, kind="smooth", seed=7))

    class Kept(pkg.Stylization):
        calls = []

        def close(self):                      # main() closes its model; the comparison below still needs it
            pass

        def transfer_frames(self, frames, **kw):
            self.calls.append(kw.get("out_format"))
            return super().transfer_frames(frames, **kw)
    models = []

    def factory(args, device):
        models.append(Kept(weights, cuda=True, device=device))
        return models[-1]
    video = str(tmp_path / "out.y4m")
    with fixed_kernels():
        rc = D.main(["--style", str(tmp_path / "style.png"), "--frames", str(src / "*.png"), "--checkpoint", "synthetic", "--out", str(tmp_path / "out"),
                     "--video", video, "--no-frames", "--chunk", "2", "--io-threads", "2"], model_factory=factory)
        assert rc == 0 and Kept.calls == ["i420"] * 3
        s = models[0]
        ref = [Y.yuv_ref(s.transfer_frames(frames[c0:c0 + 2]), BT601, "i420") for c0 in (0, 2, 4)]
    pkg.Stylization.close(s)
    assert not (tmp_path / "out").exists()
    fields, got = D.read_y4m(video)
    assert fields == [b"W80", b"H48", b"F24:1", b"Ip", b"A1:1", b"C420jpeg", b"XCOLORRANGE=LIMITED"]
    assert got == [bytes(r) for chunk in ref for r in chunk]

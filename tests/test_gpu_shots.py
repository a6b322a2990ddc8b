"""Shots on the GPU (include/rerevst_hip.h "Shots"): shot_sig_k against video.shot_signature word for word, the view entry and the host
twins against the entries they are defined by, the detector end to end on the synthetic video of tests/test_shots_host.py, and the
driver's per-shot flow against running each shot as a video of its own, bit for bit in a fixed kernel mode.

Every comparison here is exact: the signature is integer arithmetic on values both sides share, and the entries that are compared
run the same kernels on the same bytes."""
import ctypes as C
import importlib

import numpy as np
import pytest

import jpeg_dec_ref
from conftest import fixed_kernels
from test_shots_host import CUTS, synthetic_video, video_and_signatures

pytestmark = pytest.mark.gpu

RRV_OK, RRV_E_ARG, RRV_E_NOMEM = 0, -1, -5
L = importlib.import_module("rerevst-code_amd._lib")
F = importlib.import_module("rerevst-code_amd.framework")
V = importlib.import_module("rerevst-code_amd.video")
D = importlib.import_module("rerevst-code_amd.driver")
# one pixel per cell; odd; odd with several rows per wave; cells of one wave step; a cell wider than a workgroup (275 columns: five steps
# of 64 lanes, the last ragged); the thumbnail of a 1080p frame
SIZES = ((4, 4), (5, 7), (37, 53), (48, 64), (8, 1100), (270, 480))
SPECIALS = (0.5, 1.5, 2.5, 254.5, 255.5, -3.0, 300.0, np.nan, np.inf, -np.inf, -0.0, 7.5, 8.5, 127.5, 128.5)


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def hip(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    yield s
    s.close()


def _kernel(s, frames):
    """rrv_shot_signature_device on float32 [B][H][W][3]; the output starts as 0xFFFFFFFF words between two guard bands"""
    t = _torch()
    x = t.from_numpy(np.ascontiguousarray(frames, np.float32)).cuda() if isinstance(frames, np.ndarray) else frames.contiguous()
    B, H, W, _ = x.shape
    buf = t.full((B + 2, 16, 32), -1, dtype=t.int32, device="cuda")
    t.cuda.synchronize()
    rc = s._lib.rrv_shot_signature_device(s._h, C.c_void_p(x.data_ptr()), B, H, W, C.c_void_p(buf.data_ptr() + 2048), None)
    t.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    assert rc == RRV_OK, s._lib.rrv_last_error(s._h)
    assert (host[0] == 0xFFFFFFFF).all() and (host[-1] == 0xFFFFFFFF).all(), "stores outside the output"
    return host[1:-1]


def _contents(H, W):
    rng = np.random.default_rng(1000 * H + W)
    rand = rng.uniform(-20, 280, (3, H, W, 3)).astype(np.float32)                    # non-integer floats on both sides of the clamp
    const = np.full((3, H, W, 3), (17.25, 203.5, 96.75), np.float32)                 # every lane of every wave hits one LDS word
    const[1], const[2] = 255.0, 0.0
    spec = np.resize(np.array(SPECIALS, np.float32), (3, H, W, 3)).copy()
    spec[1] = np.roll(spec[1].reshape(-1), 1).reshape(H, W, 3)
    spec[2, ::2] = rng.uniform(0, 255, spec[2, ::2].shape)
    return {"random": rand, "constant": const, "specials": spec}


@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_equals_the_numpy_restatement(hip, H, W):
    for name, frames in _contents(H, W).items():
        want = np.stack([V.shot_signature(f) for f in frames])
        got3 = _kernel(hip, frames)
        np.testing.assert_array_equal(got3, want, err_msg="%s, B = 3" % name)
        for b in range(3):      # frame b of the B = 3 call is its B = 1 call
            np.testing.assert_array_equal(_kernel(hip, frames[b:b + 1])[0], got3[b], err_msg="%s, frame %d alone" % (name, b))


def test_kernel_entry_refusals(hip):
    t = _torch()
    x = t.zeros((1, 4, 4, 3), dtype=t.float32, device="cuda")
    sig = t.zeros((1, 16, 32), dtype=t.int32, device="cuda")
    f = hip._lib.rrv_shot_signature_device
    for args in ((x.data_ptr(), 1, 3, 4, sig.data_ptr()), (x.data_ptr(), 1, 4, 3, sig.data_ptr()), (x.data_ptr(), 0, 4, 4, sig.data_ptr()),
                 (x.data_ptr(), 65, 4, 4, sig.data_ptr()), (None, 1, 4, 4, sig.data_ptr()), (x.data_ptr(), 1, 4, 4, None)):
        assert f(hip._h, *args, None) == RRV_E_ARG, args
    assert f(hip._h, x.data_ptr(), 1, 4, 4, sig.data_ptr(), None) == RRV_OK
    t.cuda.synchronize()
    # a frame whose thumbnail falls below 4 x 4 (513 x 4 -> 257 x 2)
    with pytest.raises(hip_error()) as e:
        hip.shot_signatures_tensor(t.zeros((513, 4, 3), dtype=t.uint8, device="cuda"), layout="nhwc")
    assert e.value.code == RRV_E_ARG and "257 x 2" in str(e.value)


def hip_error():
    return importlib.import_module("rerevst-code_amd").RRVError


def _view_case(name):
    """(x, keywords of the tensor entries, frames) of a view-entry case"""
    t = _torch()
    rng = np.random.default_rng(len(name))
    if name == "u8-nhwc-64x96":
        return t.from_numpy(rng.integers(0, 256, (3, 64, 96, 3), dtype=np.uint8)).cuda(), dict(layout="nhwc"), 3, (64, 96)
    if name == "nv12-520x24":
        return t.from_numpy(rng.integers(0, 256, (3, 520 * 24 * 3 // 2), dtype=np.uint8)).cuda(), dict(layout="nv12", size=(520, 24)), 3, (520, 24)
    H, W, pitch, rows = 40, 56, 64, 48      # a pitched P010 surface: rows of 64 samples, the luma plane 48 rows tall, three frames 6400 samples apart
    stride = pitch * rows + pitch * (rows // 2) + 256
    store = (rng.integers(0, 1024, (3 * stride,), dtype=np.uint16) << 6).astype(np.uint16)
    view = F.ImageView(t.from_numpy(store.view(np.int16)).cuda(), "p010", (H, W), pitch, plane_offset=(0, pitch * rows), frame_stride=stride, frames=3)
    return view, {}, 3, (H, W)


@pytest.mark.parametrize("name", ["u8-nhwc-64x96", "nv12-520x24", "p010-pitched"])
def test_view_entry_is_the_resampler_then_the_kernel(hip, name):
    x, kw, B, size = _view_case(name)
    thumb = F.shot_plan(*size)
    assert thumb == {"u8-nhwc-64x96": (64, 96), "nv12-520x24": (260, 12), "p010-pitched": (40, 56)}[name]
    hip.set_yuv_input_matrix("bt709", False, **({"bits": 10} if name == "p010-pitched" else {}))
    got = hip.shot_signatures_tensor(x, **kw)
    assert tuple(got.shape) == (B, 16, 32) and str(got.dtype) == "torch.int32"
    want = _kernel(hip, hip.resample_tensor(x, thumb, **kw))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want)
    assert want.sum() == B * thumb[0] * thumb[1]


def test_host_twin_equals_the_device_entry_across_a_sub_batch(hip):
    t = _torch()
    rng = np.random.default_rng(3)
    B, H, W = 20, 36, 52
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    got = hip.shot_signatures(frames)
    assert got.shape == (B, 16, 32) and got.dtype == np.uint32
    np.testing.assert_array_equal(got, hip.shot_signatures_tensor(t.from_numpy(frames).cuda(), layout="nhwc").cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(got, [V.shot_signature(f) for f in frames])      # ratio 1: the thumbnail is the frame
    np.testing.assert_array_equal(hip.shot_signatures([f for f in frames]), got)      # a list
    mixed = [frames[0], frames[1], frames[2, :20, :30], frames[3, :20, :30], frames[4]]      # a list of mixed sizes: runs of equal size
    np.testing.assert_array_equal(hip.shot_signatures(mixed), [V.shot_signature(f) for f in mixed])
    hip.set_yuv_input_matrix("bt601", False)
    yuv = rng.integers(0, 256, (B, V.yuv_frame_bytes(H, W)), dtype=np.uint8)
    got = hip.shot_signatures(yuv, in_format="i420", size=(H, W))
    np.testing.assert_array_equal(got, hip.shot_signatures_tensor(t.from_numpy(yuv).cuda(), layout="i420", size=(H, W)).cpu().numpy().view(np.uint32))
    n = V.yuv_input_matrix("bt601", False)
    np.testing.assert_array_equal(got[:2], [V.shot_signature(f) for f in V.yuv420_to_bgr(yuv[:2], H, W, n)])      # and the numpy conversion, ratio 1


def test_jpeg_twin_equals_decode_then_the_view_entry(hip, pkg):
    rng = np.random.default_rng(4)
    frames = [jpeg_dec_ref.pillow_stream(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), 90, chroma, restart_marker_blocks=4) for chroma in ("420",) * 18]
    hip.set_yuv_input_matrix("bt709", False)      # whatever the handle holds: the twin installs JFIF's matrix for the call
    got = hip.shot_signatures(frames, in_format="jpeg")
    assert got.shape == (18, 16, 32)
    planes, layout = hip.decode_jpeg_tensor(frames)
    hip.set_yuv_input_matrix("bt601", True)
    want = hip.shot_signatures_tensor(planes, layout=layout, size=(40, 56)).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, want)
    hip.set_yuv_input_matrix("bt709", False)
    np.testing.assert_array_equal(hip.shot_signatures(frames[:3], in_format="jpeg"), want[:3])      # the handle's matrix came back, and does not matter
    # runs of one size and chroma format
    other = jpeg_dec_ref.pillow_stream(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8), 90, "444")
    mixed = hip.shot_signatures([frames[0], other, other, frames[1]], in_format="jpeg")
    np.testing.assert_array_equal(mixed[[0, 3]], want[:2])
    np.testing.assert_array_equal(mixed[1], mixed[2])
    # a truncated stream: ValueError with its index; the handle stays usable
    bad = list(frames)
    bad[17] = bad[17][:len(bad[17]) // 2]
    with pytest.raises(ValueError, match="frame 17"):
        hip.shot_signatures(bad, in_format="jpeg")
    with pytest.raises(ValueError, match="frame 1"):
        hip.shot_signatures([frames[0], b"not a jpeg"], in_format="jpeg")
    with pytest.raises(ValueError, match="frame 3 is corrupt"):      # the index in the caller's list, not in the run of equal size that starts at 2
        hip.shot_signatures([other, other, frames[0], bad[17]], in_format="jpeg")
    np.testing.assert_array_equal(hip.shot_signatures(frames, in_format="jpeg"), want)


def test_out_of_memory_on_the_thumbnails_leaves_the_handle_usable(pkg, weights):
    t = _torch()
    s = pkg.Stylization(weights, cuda=True)
    try:
        x = t.from_numpy(np.random.default_rng(5).integers(0, 256, (4, 24, 40, 3), dtype=np.uint8)).cuda()
        one = s.shot_signatures_tensor(x[:1], layout="nhwc")      # the tap tables and a thumbnail buffer of one frame now exist
        s.debug_fail_alloc(1)                                     # the next allocation: the buffer growing to four frames
        with pytest.raises(pkg.RRVError) as e:
            s.shot_signatures_tensor(x, layout="nhwc")
        assert e.value.code == RRV_E_NOMEM
        s.debug_fail_alloc(0)
        got = s.shot_signatures_tensor(x, layout="nhwc").cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, [V.shot_signature(f) for f in x.cpu().numpy()])
        np.testing.assert_array_equal(one.cpu().numpy().view(np.uint32)[0], got[0])
    finally:
        s.close()


@pytest.mark.parametrize("H,W", [(48, 64), (37, 53)])
def test_detector_end_to_end_on_the_synthetic_video(hip, H, W):
    frames, sigs = video_and_signatures(H, W)
    got = hip.shot_signatures(frames)
    np.testing.assert_array_equal(got, sigs)
    assert V.detect_cuts(V.shot_distances(got, [(H, W)] * len(frames))) == CUTS


# ---- the driver: a per-shot run equals each shot run as a video of its own
def _two_shot_frames():
    v = synthetic_video(48, 64)
    return v[:5] + v[11:18]      # five dark frames, seven bright ones


def _read_all(paths):
    return [D.read_image_bgr(p) for p in paths]


def test_driver_per_shot_equals_each_shot_alone_files(tmp_path, pkg, weights):
    frames = _two_shot_frames()
    src = tmp_path / "in"
    src.mkdir()
    for i, f in enumerate(frames):
        D.write_image_bgr(str(src / ("f%02d.png" % i)), f)
    D.write_image_bgr(str(tmp_path / "style.png"), pkg.synth_style(64, 64, kind="smooth", seed=7))
    paths = D.list_frames(str(src / "*.png"))
    s = pkg.Stylization(weights, cuda=True)
    kw = dict(chunk=4, io_threads=2, log=lambda *_: None)
    try:
        with fixed_kernels(s, mode=0):
            run = lambda name, p, **k: _read_all(D.stylize_files(s, str(tmp_path / "style.png"), p, str(tmp_path / name), **kw, **k))
            two = run("two", paths, shots=[(0, 5), (5, 12)])
            alone = run("a", paths[:5]) + run("b", paths[5:])
            one = run("one", paths, shots=[(0, 12)])
            none = run("none", paths)
            auto = run("auto", paths, shots="auto", shot_params=dict(min_len=4))
    finally:
        s.close()
    assert len(two) == 12
    for i in range(12):
        np.testing.assert_array_equal(two[i], alone[i], err_msg="frame %d: per shot vs the shot alone" % i)
        np.testing.assert_array_equal(one[i], none[i], err_msg="frame %d: one shot vs no shots" % i)
        np.testing.assert_array_equal(auto[i], two[i], err_msg="frame %d: detected vs given" % i)
    assert any((two[i] != none[i]).any() for i in range(12)), "two states and one state gave the same frames"


def test_driver_per_shot_equals_each_shot_alone_y4m(tmp_path, pkg, weights):
    frames = _two_shot_frames()
    m = V.yuv_matrix("bt601", False)

    def write(name, fs):
        w = D.Y4MWriter(str(tmp_path / name), 24, 64, 48)
        for f in fs:
            w.append(V.bgr_to_yuv420(f, m), (48, 64))
        w.release()
        return str(tmp_path / name)
    whole, a, b = write("in.y4m", frames), write("a.y4m", frames[:5]), write("b.y4m", frames[5:])
    D.write_image_bgr(str(tmp_path / "style.png"), pkg.synth_style(64, 64, kind="smooth", seed=7))
    s = pkg.Stylization(weights, cuda=True)
    kw = dict(write_frames=False, chunk=4, io_threads=2, log=lambda *_: None)
    try:
        with fixed_kernels(s, mode=0):
            def run(name, path, **k):
                out = str(tmp_path / (name + ".y4m"))
                D.stylize_y4m(s, str(tmp_path / "style.png"), path, str(tmp_path / name), video_path=out, **kw, **k)
                return D.read_y4m(out)[1]
            two = run("two", whole, shots=[(0, 5), (5, 12)])
            alone = run("oa", a) + run("ob", b)
            one = run("one", whole, shots=[(0, 12)])
            none = run("none", whole)
            auto = run("auto", whole, shots="auto", shot_params=dict(min_len=4))
    finally:
        s.close()
    assert len(two) == 12 and two == alone and one == none and auto == two
    assert two != none, "two states and one state gave the same frames"

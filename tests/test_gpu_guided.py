"""Guided delivery on the GPU (include/rerevst_hip.h "Guided delivery").

The stage alone (gf_coeff_k, gf_apply_k through rrv_deliver_guided_view_device) against the float64 reference of its own inputs
(tests/guided_ref.py), on the smallest shapes that can go wrong.  The stage is bit-exact to nothing; its bound per case is
guided_ref.TOL_FACTOR times the largest error of the plain float32 numpy restatement on the same inputs (guided_ref.NAIVE_ERR, measured on
the CPU and recorded in profiles/guided.txt; tests/test_guided_host.py keeps the table equal to what the restatement gives).
Then the entries, bit for bit in a fixed kernel mode (conftest.fixed_kernels): tiny frames."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import chroma_ref
import guided_ref as G
from conftest import load_golden, fixed_kernels

pytestmark = pytest.mark.gpu

RRV_OK, RRV_E_ARG, RRV_E_NOMEM = 0, -1, -5
L = importlib.import_module("rerevst-code_amd._lib")
F32_HWC, U8_HWC = (L.DT_F32, L.LAY_HWC_BGR), (L.DT_U8, L.LAY_HWC_BGR)


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _host(s, t):
    _torch().cuda.synchronize()
    s.sync()
    _torch().cuda.synchronize()
    if t.dtype == _torch().uint16:
        return t.view(_torch().int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _ok(s, rc):
    assert rc == RRV_OK, s._lib.rrv_last_error(s._h)


def _contig(form, H, W):
    v = L.ImageView()
    assert L.load().rrv_image_view_contiguous(L.ImageDesc(form[0], form[1], L.SP_PIXEL), H, W, C.byref(v)) == RRV_OK
    return v


def _u8_frames(seed, B, H, W):
    """smooth blobs plus noise, so that the guide has edges and flat parts"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros((B, H, W, 3))
    for b in range(B):
        for c in range(3):
            cy, cx, rad = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.15, 0.4) * min(H, W)
            out[b, ..., c] = np.where((yy - cy) ** 2 + (xx - cx) ** 2 < rad * rad, 190.0, 60.0) + 0.4 * xx + rng.uniform(-12, 12, (H, W))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def hip(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    s.set_state(load_golden("global_a")["state"])
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    work, dst, r = G.CASES[case]
    return G.inputs(kind, 1, work, dst)


@functools.lru_cache(maxsize=None)
def _reference(case, kind, eps):
    P, lo, hi = _case(case, kind)
    ref = G.stage(P, lo, hi, G.CASES[case][2], eps)
    ref.setflags(write=False)
    return ref


# ---- the stage alone
@pytest.mark.parametrize("eps", G.EPS)
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("case", sorted(G.CASES))
def test_stage_against_float64(hip, case, kind, eps):
    work, dst, r = G.CASES[case]
    P, lo, hi = _case(case, kind)
    got = _host(hip, hip.deliver_tensor(_dev(P), dst, guide_lo=_dev(lo), guide_hi=_dev(hi), guide_radius=r, guide_eps=eps))
    assert got.shape == (1, *dst, 3) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - _reference(case, kind, eps)).max())
    bound = G.TOL_FACTOR * G.NAIVE_ERR[case, kind, eps]
    print("guided %s %s eps=%g: max|d| = %.3e, naive float32 %.3e, bound %.3e" % (case, kind, eps, err, G.NAIVE_ERR[case, kind, eps], bound))
    assert err <= bound


def _tile(case):
    work, dst, r = G.CASES[case]
    out = [C.c_int(-1) for _ in range(5)]
    assert L.load().rrv_guided_tile(*work, *dst, r, *[C.byref(v) for v in out]) == RRV_OK
    return tuple(v.value for v in out)      # tw, sy, sx, gf_apply_k's LDS bytes, gf_coeff_k's


def test_the_new_cases_run_the_tiles_they_are_for():
    """What the library launches for cases e, f and g of test_stage_against_float64, from the library itself: gf_apply_k with 32 columns per
    tile (e, g), and with 64 at the largest LDS request that fits, far above the 64 KB a launch gets without the attribute (f)"""
    assert _tile("e")[:4] == (32, 18, 34, 120000)
    assert _tile("f")[:4] == (64, 18, 66, 147840) and 65536 < 147840 <= 152 * 1024
    assert _tile("g")[:4] == (32, 15, 30, 103776)
    assert all(_tile(c)[0] == 64 and _tile(c)[3] <= 65536 for c in G.CASES if c not in ("e", "f", "g"))
    assert _tile("d")[4] == _tile("e")[4] == 98304      # gf_coeff_k at r = 16: above 64 KB as well


def test_one_working_pixel_is_delivered_bit_for_bit(hip):
    """(1, 1) -> (8, 8): every window is the one pixel, so covariance and variance are exactly 0, a = 0, b = P, and Q[y][x][c] = P[0][0][c] bit for
    bit, whatever the guide, the radius and eps"""
    rng = np.random.default_rng(17)
    P = rng.uniform(1.0, 255.0, (3, 1, 1, 3)).astype(np.float32)
    lo = rng.uniform(0.0, 255.0, (3, 1, 1, 3)).astype(np.float32)
    hi = rng.uniform(0.0, 255.0, (3, 8, 8, 3)).astype(np.float32)
    want = np.broadcast_to(P, (3, 8, 8, 3))
    for r in (1, 5, 16):
        for eps in (1e-6,) + G.EPS:
            assert np.array_equal(G.stage(P, lo, hi, r, eps, np.float32), want) and np.array_equal(G.stage(P, lo, hi, r, eps), want)
            got = _host(hip, hip.deliver_tensor(_dev(P), (8, 8), guide_lo=_dev(lo), guide_hi=_dev(hi), guide_radius=r, guide_eps=eps))
            np.testing.assert_array_equal(got, want)


def test_the_batch_limit_equals_one_call_per_frame(hip):
    """B = 64, the entry's limit: frame b's bits are those of the call on frame b alone"""
    work, dst, r = (8, 8), (16, 24), 4
    P, lo, hi = (_dev(a) for a in G.inputs("noise", 64, work, dst, seed=4))
    kw = dict(guide_radius=r, guide_eps=1e-3)
    whole = _host(hip, hip.deliver_tensor(P, dst, guide_lo=lo, guide_hi=hi, **kw))
    ones = [hip.deliver_tensor(P[b], dst, guide_lo=lo[b], guide_hi=hi[b], **kw) for b in range(64)]
    ones = _host(hip, _torch().stack(ones))
    assert whole.shape == (64, *dst, 3) and not np.array_equal(whole[0], whole[63])
    np.testing.assert_array_equal(whole, ones)


def test_each_frame_equals_its_own_call(hip):
    """B = 3 distinct frames: frame b's bits are those of the call on frame b alone"""
    work, dst, r = (40, 72), (97, 131), 4
    P, lo, hi = (_dev(a) for a in G.inputs("noise", 3, work, dst, seed=3))
    assert not np.array_equal(P[0].cpu().numpy(), P[1].cpu().numpy())
    kw = dict(guide_radius=r, guide_eps=1e-3)
    whole = _host(hip, hip.deliver_tensor(P, dst, guide_lo=lo, guide_hi=hi, **kw))
    for b in range(3):
        one = _host(hip, hip.deliver_tensor(P[b], dst, guide_lo=lo[b], guide_hi=hi[b], **kw))
        np.testing.assert_array_equal(whole[b], one)


# ---- the entries
# name: (source size, working size or None = unscaled, pad_crop)
COMPOSE = {"scaled": ((96, 128), (48, 64), False), "scaled_pad_crop_odd": ((70, 99), (37, 51), True), "unscaled_equal_size": ((64, 72), None, False)}


@pytest.mark.parametrize("name", sorted(COMPOSE))
def test_guided_call_equals_three_steps(hip, name):
    """transfer_tensor(.., guide="source") == the float32 call at the working size, resample_tensor for both guides, deliver_tensor(guide_lo=, guide_hi=)"""
    src, work, pad = COMPOSE[name]
    x = _dev(_u8_frames(len(name), 3, *src))
    kw = dict(layout="nhwc", pad_crop=pad, **({} if work is None else {"work_size": work}))
    gk = dict(guide_radius=3, guide_eps=2e-3)
    with fixed_kernels(hip, mode=0):
        got = _host(hip, hip.transfer_tensor(x, out_size="source", guide="source", **kw, **gk))
        y = hip.transfer_tensor(x, **kw)
        hi = hip.resample_tensor(x, src, layout="nhwc")
        lo = hi if work is None else hip.resample_tensor(x, work, layout="nhwc")
        assert tuple(y.shape) == tuple(lo.shape)
        want = _host(hip, hip.deliver_tensor(y, src, guide_lo=lo, guide_hi=hi, **gk))
        plain = _host(hip, hip.transfer_tensor(x, out_size="source", **kw))
    assert got.shape == (3, *src, 3) and got.std() > 1.0
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, plain)      # (and it is not the bilinear delivery)


def test_host_entry_equals_device_entry(hip):
    src, work = (96, 128), (48, 64)
    u8 = _u8_frames(11, 5, *src)
    gk = dict(work_size=work, out_size="source", guide="source", guide_radius=4, guide_eps=1e-3)
    with fixed_kernels(hip, mode=0):
        want = _host(hip, hip.transfer_tensor(_dev(u8), layout="nhwc", **gk))
        got = hip.transfer_batch(u8, **gk)
        want_pad = _host(hip, hip.transfer_tensor(_dev(u8), layout="nhwc", pad_crop=True, **gk))
        got_pad = hip.transfer_frames(u8, **gk)
    assert got.dtype == np.float32 and got.std() > 1.0
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_pad, want_pad)


@pytest.mark.parametrize("form", ("uint8", "nv12", "p010"))
def test_output_forms_are_the_delivery_of_q(hip, form):
    """the guided call into an integer form == deliver_tensor of its float32 Q at equal size into that form"""
    t = _torch()
    src, work = (96, 128), (48, 64)
    x = _dev(_u8_frames(12, 2, *src))
    gk = dict(layout="nhwc", work_size=work, out_size="source", guide="source", guide_radius=2, guide_eps=1e-3)
    ok = dict(out_dtype=t.uint8) if form == "uint8" else dict(out_layout=form)
    with fixed_kernels(hip, mode=0):
        q = hip.transfer_tensor(x, **gk)
        got = _host(hip, hip.transfer_tensor(x, **gk, **ok))
        want = _host(hip, hip.deliver_tensor(q, src, **ok))
    assert got.shape == ((2, *src, 3) if form == "uint8" else (2, chroma_ref.frame_samples(*src, "420")))
    assert got.astype(np.float64).std() > 1.0
    np.testing.assert_array_equal(got, want)


def test_argument_errors_leave_the_handle_usable(hip):
    t = _torch()
    lib, h = hip._lib, hip._h
    SH, SW, H, W = 96, 128, 48, 64
    u8 = _u8_frames(13, 2, SH, SW)
    d_in = _dev(u8)
    out = t.zeros((2, SH, SW, 3), dtype=t.float32, device="cuda")
    vi, vo = _contig(U8_HWC, SH, SW), _contig(F32_HWC, SH, SW)

    def call(r=4, eps=1e-3, sh=SH, sw=SW, hh=H, ww=W, dh=SH, dw=SW, flags=0, view_in=vi, view_out=vo):
        return lib.rrv_transfer_guided_view_device(h, C.c_void_p(d_in.data_ptr()), C.byref(view_in), 2, sh, sw, hh, ww, dh, dw, r, eps,
                                                   C.c_void_p(out.data_ptr()), C.byref(view_out), flags | L.TF_ON_STREAM, None)
    for bad in (dict(r=0), dict(r=17), dict(r=-1)):
        assert call(**bad) == RRV_E_ARG and b"r must be" in lib.rrv_last_error(h)
    for bad in (dict(eps=0.0), dict(eps=-1e-3), dict(eps=float("nan"))):
        assert call(**bad) == RRV_E_ARG and b"eps" in lib.rrv_last_error(h)
    # the delivered size is the source's
    assert call(dh=SH - 8, view_out=_contig(F32_HWC, SH - 8, SW)) == RRV_E_ARG and b"DH x DW" in lib.rrv_last_error(h)
    assert call(dh=0, dw=0) == RRV_E_ARG and b"DH" in lib.rrv_last_error(h)
    # unscaled: H x W is the source, and the delivered size must be H x W
    v96 = _contig(F32_HWC, 2 * SH, 2 * SW)
    assert call(sh=0, sw=0, hh=SH, ww=SW, dh=2 * SH, dw=2 * SW, view_out=v96) == RRV_E_ARG and b"DH x DW" in lib.rrv_last_error(h)
    # the working frame is delivered whole: multiples of 8 without RRV_TF_PAD_CROP
    assert call(hh=H + 3) == RRV_E_ARG and b"multiples of 8" in lib.rrv_last_error(h)
    assert call(flags=L.TF_WEIGHTS_DEVICE) == RRV_E_ARG
    # the stage alone
    P, lo, hi = (_dev(a) for a in G.inputs("noise", 2, (H, W), (SH, SW)))

    def alone(r=4, eps=1e-3, dh=SH, dw=SW, p=P.data_ptr(), view=vo):
        return lib.rrv_deliver_guided_view_device(h, C.c_void_p(p), C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), 2, H, W, dh, dw, r, eps,
                                                  C.c_void_p(out.data_ptr()), C.byref(view), None)
    assert alone(r=0) == RRV_E_ARG and alone(r=17) == RRV_E_ARG and alone(eps=0.0) == RRV_E_ARG
    assert alone(dh=H - 1, view=_contig(F32_HWC, H - 1, SW)) == RRV_E_ARG and b"DH" in lib.rrv_last_error(h)
    assert alone(dw=8 * W + 1, view=_contig(F32_HWC, SH, 8 * W + 1)) == RRV_E_ARG and b"DW" in lib.rrv_last_error(h)
    assert alone(p=None) == RRV_E_ARG
    assert alone(view=_contig(F32_HWC, SH - 1, SW)) == RRV_E_ARG and b"out.frame_stride" in lib.rrv_last_error(h)
    # the host twin
    host = np.zeros(2 * SH * SW * 3, np.float32)
    desc_in, desc_out = L.ImageDesc(*U8_HWC, L.SP_PIXEL), L.ImageDesc(*F32_HWC, L.SP_PIXEL)

    def twin(r=4, eps=1e-3, flags=0):
        return lib.rrv_transfer_guided(h, u8.ctypes.data_as(C.c_void_p), desc_in, 2, SH, SW, H, W, SH, SW, r, eps, host.ctypes.data_as(C.c_void_p), desc_out, flags)
    assert twin(r=0) == RRV_E_ARG and twin(eps=0.0) == RRV_E_ARG and twin(flags=L.TF_ON_STREAM) == RRV_E_ARG
    # Python refuses what names no guide or no delivered size
    with pytest.raises(ValueError):
        hip.transfer_batch(u8, work_size=(H, W), out_size="source", guide="luma")
    with pytest.raises(ValueError):
        hip.transfer_batch(u8, work_size=(H, W), guide="source")
    with pytest.raises(ValueError):
        hip.deliver_tensor(P, (SH, SW), guide_lo=lo)
    with fixed_kernels(hip, mode=0):      # the handle works
        _ok(hip, call())
        dev = _host(hip, out)
        _ok(hip, twin())
    assert host.std() > 1.0
    np.testing.assert_array_equal(host.reshape(dev.shape), dev)


def test_out_of_memory_reserving_the_guided_buffers(hip, pkg, weights):
    """X_hi, the coefficient planes and Q are reserved before the call's first launch.  With the workspace, the working-frame buffers and the
    scaling tables in place (a bilinear delivering call), a guided call allocates the two identity tables and then the three buffers: each
    made to fail in turn is RRV_E_NOMEM with nothing launched; afterwards the plain call returns the bits it returned before and the guided
    call the bits of an untroubled handle."""
    src, work = (96, 128), (48, 64)
    u8 = _u8_frames(14, 2, *src)
    kw = dict(layout="nhwc", work_size=work, out_size="source")
    gk = dict(guide="source", guide_radius=4, guide_eps=1e-3)
    s = pkg.Stylization(weights, cuda=True)
    try:
        s.set_state(load_golden("global_a")["state"])
        with fixed_kernels(s, hip, mode=0):
            want = _host(hip, hip.transfer_tensor(_dev(u8), **kw, **gk))
            x = _dev(u8)
            before = _host(s, s.transfer_tensor(x, **kw))      # slot 0: its plans, both buffers of working frames, the tables
            s.profile_begin()                                  # (profiled launches stay on slot 0)
            for nth in (3, 2, 2):                              # X_hi behind the two tables; then X_hi exists: the planes; then Q
                s.debug_fail_alloc(nth)
                with pytest.raises(pkg.RRVError) as e:
                    s.transfer_tensor(x, **kw, **gk)
                s.debug_fail_alloc(0)
                assert e.value.code == RRV_E_NOMEM and "out of device memory" in str(e.value)
            assert len(s.profile_end()) == 0
            after = _host(s, s.transfer_tensor(x, **kw))
            got = _host(s, s.transfer_tensor(x, **kw, **gk))
            again = _host(s, s.transfer_tensor(x, **kw))
    finally:
        s.close()
    np.testing.assert_array_equal(after, before)
    np.testing.assert_array_equal(again, before)      # the same call without `guide` returns the bits it returned before
    np.testing.assert_array_equal(got, want)


def test_driver_guided_y4m(tmp_path, pkg, weights):
    """Six frames of 96 x 128 in a .y4m, --work-size 64x48 --out-size source --guided 3:2e-3 --video out.y4m --no-frames: the frames equal
    transfer_frames(work_size=(48, 64), out_size="source", guide="source", guide_radius=3, guide_eps=2e-3) on the same bytes with the same
    frames per call, and differ from the bilinear delivery."""
    D = importlib.import_module("rerevst-code_amd.driver")
    H, W, WH, WW = 96, 128, 48, 64
    bgr = _u8_frames(21, 6, H, W)
    V = importlib.import_module("rerevst-code_amd.video")
    m = V.yuv_matrix("bt601", False)
    buf = np.stack([np.asarray(V.bgr_to_yuv420(f, m, "i420"), np.uint8).reshape(-1) for f in bgr])
    src = str(tmp_path / "in.y4m")
    w = D.Y4MWriter(src, 25, W, H)
    for fr in buf:
        w.append(fr, (H, W))
    w.release()
    D.write_image_bgr(str(tmp_path / "style.png"), pkg.synth_style(64, 64, kind="smooth", seed=7))

    class Kept(pkg.Stylization):
        calls = []

        def close(self):                      # main() closes its model; the comparison below still needs it
            pass

        def transfer_frames(self, frames, **kw):
            self.calls.append({k: kw.get(k) for k in ("work_size", "out_size", "guide", "guide_radius", "guide_eps")})
            return super().transfer_frames(frames, **kw)
    models = []

    def factory(args, device):
        models.append(Kept(weights, cuda=True, device=device))
        return models[-1]
    video = str(tmp_path / "out.y4m")
    kw = dict(in_format="i420", size=(H, W), out_format="i420", work_size=(WH, WW), out_size="source")
    with fixed_kernels():
        rc = D.main(["--style", str(tmp_path / "style.png"), "--frames", src, "--checkpoint", "synthetic", "--out", str(tmp_path / "out"), "--video", video,
                     "--no-frames", "--chunk", "4", "--work-size", "%dx%d" % (WW, WH), "--out-size", "source", "--guided", "3:2e-3"], model_factory=factory)
        assert rc == 0 and Kept.calls == [dict(work_size=(WH, WW), out_size=(H, W), guide="source", guide_radius=3, guide_eps=2e-3)] * 2
        s = models[0]
        ref = [np.array(s.transfer_frames(buf[c0:c0 + 4], guide="source", guide_radius=3, guide_eps=2e-3, **kw)) for c0 in (0, 4)]
        plain = np.array(s.transfer_frames(buf[:4], **kw))
    pkg.Stylization.close(s)
    with D.Y4MReader(video) as r:
        assert (r.width, r.height, len(r)) == (W, H, 6)
        got = [bytes(r.read(i)) for i in range(6)]
    assert got == [bytes(fr) for chunk in ref for fr in chunk]
    assert not np.array_equal(ref[0], plain)

"""Guided delivery without a GPU: tests/guided_ref.py against what the arithmetic must do on inputs with a known answer, its committed
yardstick against what the float32 restatement gives, the ledger of librerevst_guided.so (every kernel symbol of its gfx950 code object
is named here and held by one test of tests/test_gpu_guided.py; the rule of tests/kernel_ledger.py, only symbol names are read), and the
guide= / --guided argument handling and video.guided_upsample."""
import importlib
import os

import numpy as np
import pytest

import guided_ref as G
import kernel_ledger as KL
import resample_ref as R

L = importlib.import_module("rerevst-code_amd._lib")
assert "rrv_deliver_guided_view_device" in L.SYMBOLS      # this file is about the guided stage the library offers: without its entries nothing here is collected
FW = importlib.import_module("rerevst-code_amd.framework")
D = importlib.import_module("rerevst-code_amd.driver")
V = importlib.import_module("rerevst-code_amd.video")

GPU = "tests/test_gpu_guided.py::"
GUIDED_LEDGER = {
    "gf_coeff_k": GPU + "test_stage_against_float64",
    "gf_apply_k": GPU + "test_each_frame_equals_its_own_call",      # (and test_stage_against_float64: both kernels run in every case)
}


def test_guided_library_ledger():
    build = importlib.import_module("rerevst-code_amd.build")
    build.build_lib(verbose=False)
    symbols = KL.symbols(build.GUIDED_LIB)
    assert len(symbols) == len(set(symbols))
    assert set(symbols) == set(GUIDED_LEDGER), (sorted(set(symbols) - set(GUIDED_LEDGER)), sorted(set(GUIDED_LEDGER) - set(symbols)))
    for key, ref in GUIDED_LEDGER.items():
        path, name = ref.split("::")
        assert os.path.isfile(os.path.join(KL.ROOT, path)), (key, ref)
        mod = importlib.import_module(os.path.splitext(os.path.basename(path))[0])
        assert callable(getattr(mod, name, None)), (key, ref)
    # and the other three libraries hold none of them: their own ledgers stay what they were
    for lib in (build.LIB, build.SCALE_LIB, build.DELIVER_LIB):
        assert not [s for s in KL.symbols(lib) if s.startswith("gf_")]


def test_a_linear_model_is_recovered():
    """P_c = alpha_c g_lo + beta_c: as eps -> 0 the fit is exact in every window, so Q = alpha g_hi + beta"""
    work, dst = (12, 20), (31, 47)
    _, lo, hi = G.inputs("noise", 2, work, dst, seed=5)
    alpha, beta = np.array([0.7, -0.4, 1.3]), np.array([20.0, 180.0, -15.0])
    P = (alpha * G.luma(lo)[..., None] + beta).astype(np.float32)
    Pd = np.asarray(P, np.float64)
    a, b = G.coefficients(P, lo, 3, 1e-13)
    # (P is rounded to float32: the fit sees alpha g + beta up to 2^-24 |P|, against a variance of thousands)
    assert np.abs(a - alpha).max() < 1e-6 and np.abs(b - beta).max() < 1e-4
    want = alpha * G.luma(hi)[..., None] + beta
    assert np.abs(G.stage(P, lo, hi, 3, 1e-13) - want).max() < 1e-3
    assert np.abs(Pd - (alpha * G.luma(lo)[..., None] + beta)).max() < 2e-5


def test_a_constant_guide_gives_the_twice_averaged_frame():
    """g constant: covariance and variance vanish, a = 0, b = M(P), Q = up(M(M(P)))"""
    work, dst, r = (10, 14), (23, 40), 2
    P, _, _ = G.inputs("noise", 1, work, dst, seed=6)
    lo, hi = np.full((1, *work, 3), 77.0, np.float32), np.full((1, *dst, 3), 77.0, np.float32)
    want = G.upsample(G.box_mean(G.box_mean(P.astype(np.float64), r), r), *dst)
    assert np.abs(G.stage(P, lo, hi, r, 1e-3) - want).max() < 1e-9
    # and the upsampling is the delivery stage's: the tables of resample_ref up to their float32 rounding
    assert np.abs(G.upsample(P.astype(np.float64), *dst) - R.resample(P, *dst)).max() < 255 * 2.0 ** -22


def test_window_counts():
    assert G.window_count(8, 1).tolist() == [2, 3, 3, 3, 3, 3, 3, 2]
    assert G.window_count(8, 3).tolist() == [4, 5, 6, 7, 7, 6, 5, 4]
    assert G.window_count(5, 9).tolist() == [5] * 5                      # a radius larger than the frame: every window is the frame
    assert G.window_count(1, 16).tolist() == [1]
    f = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    m = G.box_mean(f, 1)
    assert m[0, 0, 0] == f[0, :2, :2].mean() and m[0, 2, 3] == f[0, 1:, 2:].mean() and m[1, 1, 1] == f[1, :, :3].mean()
    np.testing.assert_allclose(G.box_mean(f, 7), np.broadcast_to(f.mean(axis=(1, 2), keepdims=True), f.shape), rtol=1e-15)
    c = G.box_mean(np.stack([f, 2 * f], -1), 1)                         # channels ride along
    np.testing.assert_array_equal(c[..., 0], m)
    np.testing.assert_array_equal(c[..., 1], 2 * m)


def test_the_yardstick_is_what_the_restatement_gives():
    """guided_ref.NAIVE_ERR (and profiles/guided.txt) are the float32 restatement's errors on the GPU test's inputs, to the digits written"""
    assert set(G.NAIVE_ERR) == {(c, k, e) for c in G.CASES for k in G.KINDS for e in G.EPS}
    for (case, kind, eps), err in G.NAIVE_ERR.items():
        assert float("%.3e" % G.naive_error(case, kind, eps)) == err, (case, kind, eps)
    with open(os.path.join(KL.ROOT, "profiles", "guided.txt")) as f:
        text = f.read()
    for (case, kind, eps), err in G.NAIVE_ERR.items():
        assert "%-5s %-6s %-7g %.3e" % (case, kind, eps, err) in text, (case, kind, eps)


def test_guide_arguments():
    assert FW._guide_args("source", 4, 1e-3, "source") == (4, 1e-3)
    assert FW._guide_args("source", np.int64(16), np.float32(0.5), (96, 128)) == (16, 0.5)
    for bad in ("Source", "luma", True, 1):
        with pytest.raises(ValueError):
            FW._guide_args(bad, 4, 1e-3, "source")
    with pytest.raises(ValueError):      # no delivered size: nothing to guide
        FW._guide_args("source", 4, 1e-3, None)


def test_driver_guided_argument(tmp_path):
    assert D.parse_guided("4") == (4, 1e-3) and D.parse_guided("16:0.01") == (16, 0.01) and D.parse_guided("1:1e-6") == (1, 1e-6)
    for bad in ("", "0", "17", "4:", "4:0", "4:-1", "4:x", "a", "4:1:2", "2.5", "4:inf"):
        with pytest.raises(ValueError):
            D.parse_guided(bad)
    base = ["--style", "a.png", "--frames", str(tmp_path / "*.png"), "--checkpoint", "synthetic", "--out", str(tmp_path / "out")]

    def no_model(args, device):
        raise AssertionError("refused before a model is built")
    for argv in (["--guided"], ["--guided", "4:1e-3", "--work-size", "64x48"], ["--guided", "--out-size", "128x96"], ["--guided", "0", "--out-size", "source"]):
        with pytest.raises(SystemExit):      # refused without a delivered size equal to the source's
            D.main(base + argv, model_factory=no_model)


def test_video_guided_upsample_restates_the_reference():
    work, dst, r, eps = (20, 28), (41, 84), 3, 2e-3
    for kind in G.KINDS:
        P, lo, hi = G.inputs(kind, 1, work, dst, seed=8)
        got = V.guided_upsample(P[0], lo[0], hi[0], radius=r, eps=eps)
        assert got.shape == (*dst, 3) and got.dtype == np.float64
        # (its tap weights are the double values, the reference's their float32 roundings; its window sums are differences of running sums)
        assert np.abs(got - G.stage(P, lo, hi, r, eps)[0]).max() < 1e-3
    with pytest.raises(ValueError):
        V.guided_upsample(P[0], lo[0], hi[0], radius=0)
    with pytest.raises(ValueError):
        V.guided_upsample(P[0], hi[0], hi[0])

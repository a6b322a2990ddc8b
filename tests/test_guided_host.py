"""Guided delivery without a GPU: tests/guided_ref.py against what the arithmetic must do on inputs with a known answer, its committed
yardstick against what the float32 restatement gives, the stage's ledger (every gf_ kernel symbol of librerevst_stages.so's gfx950 code
object is named here and held by one test of tests/test_gpu_guided.py; the rule of tests/kernel_ledger.py, only symbol names are read), and the
guide= / --guided argument handling and video.guided_upsample.  Then what gf_apply_k's correctness rests on and no GPU is needed for: the
tile rule (rrv_guided_tile against guided_ref.tile), the span bound on every table the library builds, and five deliberate flaws that the
GPU test's bounds must reject."""
import ctypes as C
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

RRV_OK, RRV_E_ARG = 0, -1
GPU = "tests/test_gpu_guided.py::"
GUIDED_LEDGER = {
    "gf_coeff_k": GPU + "test_stage_against_float64",
    # (and test_stage_against_float64: both kernels run in every case.  gf_apply_k at tw = 32 runs in its cases e and g, at the largest LDS request
    # in case f; test_the_new_cases_run_the_tiles_they_are_for holds them to that through rrv_guided_tile)
    "gf_apply_k": GPU + "test_each_frame_equals_its_own_call",
}


def test_guided_library_ledger():
    KL.check_stage_ledger(GUIDED_LEDGER, "gf_", one_test_each=False)


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


def test_new_yardsticks_are_above_one_ulp_at_255():
    """a bound of a few float32 ulps of a grey level would decide the test by rounding alone"""
    assert min(G.NAIVE_ERR.values()) >= 2.0 ** -16


# ---- the tile of gf_apply_k: rrv_guided_tile against the restatement of csrc/guided.h in guided_ref
def _lib_tile(H, W, DH, DW, r):
    out = [C.c_int(-7) for _ in range(5)]
    rc = L.load().rrv_guided_tile(H, W, DH, DW, r, *[C.byref(v) for v in out])
    return rc, tuple(v.value for v in out)


def test_tile_query_refuses_what_the_entries_refuse():
    lib = L.load()
    assert _lib_tile(24, 80, 24, 80, 16)[0] == RRV_OK
    for bad in ((24, 80, 24, 80, 0), (24, 80, 24, 80, 17), (24, 80, 24, 80, -1), (0, 80, 24, 80, 4), (24, 0, 24, 80, 4), (24, 80, 23, 80, 4),
                (24, 80, 24, 79, 4), (24, 80, 193, 80, 4), (24, 80, 24, 641, 4), (-1, -1, -1, -1, 4)):
        rc, out = _lib_tile(*bad)
        assert rc == RRV_E_ARG and out == (-7,) * 5, bad      # and nothing is written
    assert _lib_tile(24, 80, 192, 640, 4)[0] == RRV_OK
    ok = [C.c_int(-7) for _ in range(5)]
    for k in range(5):      # each null pointer
        args = [C.byref(v) for v in ok]
        args[k] = None
        assert lib.rrv_guided_tile(24, 80, 24, 80, 4, *args) == RRV_E_ARG
    assert [v.value for v in ok] == [-7] * 5


def test_tile_rule_pinned_facts():
    assert G.span(80, 80, 64) == 66 and G.span(80, 80, 32) == 34 and G.span(24, 24, 16) == 18 and G.span(1, 8, 16) == 1 and G.span(8, 64, 16) == 4
    for (work, dst, r), want in ((((24, 80), (24, 80), 16), (32, 18, 34, 120000)), (((24, 80), (24, 80), 11), (64, 18, 66, 147840)),
                                 (((24, 80), (30, 90), 16), (32, 15, 30, 103776))):
        assert G.tile(*work, *dst, r) == want
        rc, out = _lib_tile(*work, *dst, r)
        assert rc == RRV_OK and out == want + (G.coeff_lds_bytes(r),)
    # what makes case f the limit: at tw = 64 the radius above it no longer fits, and the rejected tw = 64 tile of case e is as the header's formula says
    assert G.apply_lds_bytes(16, 18, 66) == 196800 > G.LDS_MAX >= 147840 and G.tile(24, 80, 24, 80, 12)[0] == 32
    assert G.coeff_lds_bytes(16) == (4 * 48 * 64 + 8 * 48 * 32) * 4
    for case, (work, dst, r) in G.CASES.items():      # every case the GPU test runs
        rc, out = _lib_tile(*work, *dst, r)
        assert rc == RRV_OK and out == G.tile(*work, *dst, r) + (G.coeff_lds_bytes(r),), case
    assert {c: G.tile(*w, *d, r)[0] for c, (w, d, r) in G.CASES.items() if G.tile(*w, *d, r)[0] != 64} == {"e": 32, "g": 32}
    assert max(G.tile(*G.CASES[c][0], *G.CASES[c][1], G.CASES[c][2])[3] for c in ("a_r1", "a_r4", "a_r9", "b", "c", "d")) == 44928      # without e, f, g: under 64 KB


def test_tile_rule_sweep():
    """r in 1..16, working sizes 1..96 per axis, ratios 1, 1.25, 2, 3.7 and 8 (the same on both axes, and every pair of them on a coarser grid of
    sizes): the library's tile is the restatement's, a tile always exists, and only tw = 64 and 32 are ever chosen"""
    ratios = (1.0, 1.25, 2.0, 3.7, 8.0)
    chosen, n = set(), 0
    coarse = (1, 2, 7, 16, 17, 31, 33, 64, 80, 96)

    def one(H, W, DH, DW, r):
        want = G.tile(H, W, DH, DW, r)
        rc, out = _lib_tile(H, W, DH, DW, r)
        assert want is not None and rc == RRV_OK and out == want + (G.coeff_lds_bytes(r),), (H, W, DH, DW, r, out, want)
        assert want[3] <= G.LDS_MAX and want[1] == G.span(H, DH, 16) and want[2] == G.span(W, DW, want[0])
        chosen.add(want[0])
    for r in range(1, G.R_MAX + 1):
        for q in ratios:
            for H in range(1, 97):
                for W in range(1, 97):
                    one(H, W, max(H, int(H * q)), max(W, int(W * q)), r)
                    n += 1
        for qy in ratios:
            for qx in ratios:
                if qx != qy:
                    for H in coarse:
                        for W in coarse:
                            one(H, W, max(H, int(H * qy)), max(W, int(W * qx)), r)
    assert n == 16 * 5 * 96 * 96 and chosen == {64, 32}


# ---- the span bound on the library's own tables: gf_apply_k leaves out every tap beyond the sy x sx working samples its LDS holds
_TAP_CAP = 4
_TAP_BUF = (np.zeros(8 * 1080, np.int32), np.zeros(8 * 1080, np.int32), np.zeros(8 * 1080 * _TAP_CAP, np.float32))


def _tables(S, D):
    first, count, w = _TAP_BUF
    rc = L.load().rrv_resample_taps(S, D, first.ctypes.data_as(C.POINTER(C.c_int)), count.ctypes.data_as(C.POINTER(C.c_int)),
                                    w.ctypes.data_as(C.POINTER(C.c_float)), _TAP_CAP)
    assert rc == RRV_OK, (S, D)      # (a row of more than _TAP_CAP taps is refused: an upscale has three at the most)
    return first[:D], count[:D], w[:D * _TAP_CAP].reshape(D, _TAP_CAP)


def _check_axis(S, D):
    """-> (tiles checked, tiles whose span equals the bound, samples with a third tap)"""
    first, count, w = _tables(S, D)
    assert (np.diff(first) >= 0).all() and count.min() >= 1 and count.max() <= 3 and (first + count <= S).all(), (S, D)
    assert not w[:, 2:].any(), (S, D)      # a third tap weighs exactly 0.0f: the kernel's two taps are all of the sum
    end = first + count
    tiles = tight = 0
    for T in (16, 64, 32):      # GF_AT_H rows; the two widths guided_tile() ever chooses
        i0 = np.arange(0, D, T)
        i1 = np.minimum(i0 + T, D) - 1
        used = end[i1] - first[i0]
        bound = G.span(S, D, T)
        assert (used <= bound).all(), (S, D, T, int(i0[np.argmax(used)]), int(used.max()), bound)
        tiles += len(i0)
        tight += int((used == bound).sum())
    return tiles, tight, int((count == 3).sum())


def test_span_bound_holds_on_every_table():
    """every S in 1..128 and D in S..8S, every tile origin i0 = k T: first[i1] + count[i1] - first[i0] <= span(S, D, T) for the tile's last sample
    i1; first is non-decreasing, no sample has more than three taps and the third weighs nothing.  Then the sizes of real video."""
    tiles = tight = third = 0
    for S in range(1, 129):
        for D in range(S, 8 * S + 1):
            a, b, c = _check_axis(S, D)
            tiles, tight, third = tiles + a, tight + b, third + c
    for S in (360, 540, 720, 1080):
        for D in (1080, 2160):
            if S <= D <= 8 * S:
                a, b, c = _check_axis(S, D)
                tiles, tight, third = tiles + a, tight + b, third + c
    print("span bound: %d tiles, %d with no slack, %d samples with a third tap" % (tiles, tight, third))
    assert tight > 0 and third > 0      # the bound is met with equality somewhere, and three-tap samples exist: neither assertion above is vacuous
    first, count, w = _tables(7, 55)      # the example of csrc/deliver_k.h
    assert count[27] == 3 and w[27, 1] == 1.0 and w[27, 2] == 0.0 and 0.0 < w[27, 0] < 1e-15


# ---- the bounds reject wrong arithmetic: five flawed float32 restatements against the float64 reference
def _flawed_upsample(drop_col=False, early_row=False):
    """guided_ref.upsample with the second tap of every 32nd delivered column (31, 63, ..: a 32-column tile's last) dropped, or the last delivered
    row's taps starting one working row early"""
    def up(f, DH, DW):
        dt = f.dtype.type
        for axis, D in ((2, DW), (1, DH)):
            first, count, w = R.taps(f.shape[axis], D)
            w = w.astype(np.float32).astype(f.dtype)
            if drop_col and axis == 2:
                w[31::32, 1] = 0
            if early_row and axis == 1:
                first = first.copy()
                first[-1] = max(first[-1] - 1, 0)
            shape = [1] * f.ndim
            shape[axis] = D
            out = np.zeros(f.shape[:axis] + (D,) + f.shape[axis + 1:], f.dtype)
            for j in range(int(count.max())):
                idx = np.minimum(first + j, f.shape[axis] - 1)
                out = out + np.where(j < count, w[:, j], dt(0)).reshape(shape) * np.take(f, idx, axis=axis)
            f = out
        return f
    return up


def _border_box_mean(f, r):
    """guided_ref.box_mean with the corner window divided by one pixel too many"""
    H, W = f.shape[1:3]
    cnt = (G.window_count(H, r)[:, None] * G.window_count(W, r)[None, :]).astype(f.dtype)
    cnt[0, 0] += 1
    s = G._axis_sum(G._axis_sum(f, r, 2), r, 1)
    return s / (cnt[..., None] if f.ndim == 4 else cnt)


def _wrong_e(orig):
    return lambda P, x_lo, r, eps, dtype=np.float64: orig(P, x_lo, r, eps * 65536.0 / 65025.0, dtype)


FLAWS = {
    "border_window_one_pixel_more": lambda: ("box_mean", _border_box_mean),
    "luma_b_and_r_swapped": lambda: ("LUMA", (G.LUMA[2], G.LUMA[1], G.LUMA[0])),
    "e_is_eps_65536": lambda: ("coefficients", _wrong_e(G.coefficients)),
    "second_tap_of_every_32nd_column_dropped": lambda: ("upsample", _flawed_upsample(drop_col=True)),
    "last_row_one_working_row_early": lambda: ("upsample", _flawed_upsample(early_row=True)),
}


def _can_show(flaw, case):
    (H, W), (DH, DW), r = G.CASES[case]
    if flaw == "second_tap_of_every_32nd_column_dropped":      # needs a column 31 with two taps: an upscale along the row and DW >= 32
        return DW > W and DW >= 32
    if flaw == "last_row_one_working_row_early":                # needs two working rows whose means differ: with r >= H - 1 every window holds every
        return r < H - 1                                        # row, A and B are the same in all of them, and which row a tap reads changes nothing
    return True


@pytest.mark.parametrize("flaw", sorted(FLAWS))
def test_the_bounds_reject_a_flawed_restatement(flaw, monkeypatch):
    """Each flaw, in the float32 restatement only (the float64 reference is computed first, from the clean module): in every case that can show
    it the error exceeds TOL_FACTOR x NAIVE_ERR for at least one (kind, eps); in a case that cannot, the flawed restatement's error is the
    clean one's, which is what "cannot" means.  A GPU kernel with the same flaw would fail test_stage_against_float64 in the same cases."""
    shows = {c for c in G.CASES if _can_show(flaw, c)}
    if flaw == "second_tap_of_every_32nd_column_dropped":
        assert shows == {"b", "d", "g", "h_row", "j", "k"}      # (h_col delivers 8 columns; case k, DW = 80, does show it)
    elif flaw == "last_row_one_working_row_early":
        assert shows == set(G.CASES) - {"a_r9", "d", "h_row"}   # (8 rows under r = 9 and r = 16, and the one-row frame)
    else:
        assert shows == set(G.CASES)
    clean = {}
    for case, (work, dst, r) in G.CASES.items():
        for kind in G.KINDS:
            P, lo, hi = G.inputs(kind, 1, work, dst)
            for eps in G.EPS:
                clean[case, kind, eps] = (P, lo, hi, G.stage(P, lo, hi, r, eps))
    name, value = FLAWS[flaw]()
    monkeypatch.setattr(G, name, value)
    worst = {}
    for (case, kind, eps), (P, lo, hi, ref) in clean.items():
        err = float(np.abs(G.stage(P, lo, hi, G.CASES[case][2], eps, np.float32).astype(np.float64) - ref).max())
        if case in shows:
            worst[case] = max(worst.get(case, 0.0), err / (G.TOL_FACTOR * G.NAIVE_ERR[case, kind, eps]))
        else:
            assert float("%.3e" % err) == G.NAIVE_ERR[case, kind, eps], (flaw, case, kind, eps)
    print(flaw, {c: "%.3g" % v for c, v in sorted(worst.items())})
    assert set(worst) == shows and all(v > 1.0 for v in worst.values()), (flaw, worst)


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

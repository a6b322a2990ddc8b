"""Compositing (include/rerevst_hip.h "Compositing") without a GPU: the ledger of librerevst_compose.so, video.composite on inputs with known
answers, the launch rule, and the Python and driver surface.  The refusals that need a handle are in tests/test_gpu_composite.py."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import kernel_ledger

L = importlib.import_module("rerevst-code_amd._lib")
assert "rrv_composite_view_device" in L.SYMBOLS

F = importlib.import_module("rerevst-code_amd.framework")
V = importlib.import_module("rerevst-code_amd.video")
D = importlib.import_module("rerevst-code_amd.driver")
BUILD = importlib.import_module("rerevst-code_amd.build")

RRV_OK, RRV_E_ARG = 0, -1
GC = "tests/test_gpu_composite.py::"
# kernel symbol of librerevst_compose.so -> the GPU test that holds THAT instantiation to video.composite, bit for bit (its matte parameter)
COMPOSE_LEDGER = {
    "composite_k<0>": GC + "test_stage_equals_the_float32_restatement",      # [none-*]
    "composite_k<1>": GC + "test_stage_equals_the_float32_restatement",      # [f32-*]
    "composite_k<2>": GC + "test_stage_equals_the_float32_restatement",      # [u8-*]
}


def test_compose_ledger_matches_the_library():
    """kernel_ledger.check_stage_ledger against the third library: its kernels are exactly the ledger's keys, every cited test exists, and the
    other two libraries hold no compositing kernel"""
    BUILD.build_lib(verbose=False)
    mine = kernel_ledger.symbols(BUILD.COMPOSE_LIB)
    assert len(mine) == len(set(mine))
    assert set(mine) == set(COMPOSE_LEDGER), (sorted(set(mine) - set(COMPOSE_LEDGER)), sorted(set(COMPOSE_LEDGER) - set(mine)))
    for key, ref in COMPOSE_LEDGER.items():
        path, name = ref.split("::")
        assert os.path.isfile(os.path.join(kernel_ledger.ROOT, path)), (key, ref)
        mod = importlib.import_module(os.path.splitext(os.path.basename(path))[0])
        assert callable(getattr(mod, name, None)), (key, ref)
        assert key.split("<")[1].rstrip(">") in {str(v) for v in mod.MATTE_FORMS.values()}      # the test is parametrised over this instantiation
    for lib in (BUILD.LIB, BUILD.STAGES_LIB):
        assert not [s for s in kernel_ledger.symbols(lib) if "composite" in s]


# ---- video.composite on inputs with known answers
def _pair(seed, shape=(2, 5, 7, 3)):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 255, shape).astype(np.float32), rng.uniform(0, 255, shape).astype(np.float32))


def _luma(v):
    return 0.114 * v[..., 0].astype(np.float64) + 0.587 * v[..., 1] + 0.299 * v[..., 2]


def test_strength_end_points_are_the_inputs():
    P, S = _pair(1)
    np.testing.assert_array_equal(V.composite(P, S, strength=0.0), S)
    np.testing.assert_array_equal(V.composite(P, S, strength=1.0).view(np.uint32), P.view(np.uint32))
    np.testing.assert_array_equal(V.composite(P, S).view(np.uint32), P.view(np.uint32))
    per = V.composite(P, S, strength=[0.0, 1.0])
    np.testing.assert_array_equal(per[0], S[0])
    np.testing.assert_array_equal(per[1], P[1])
    half = V.composite(P, S, strength=0.5)
    assert half.dtype == np.float32
    np.testing.assert_allclose(half, 0.5 * P.astype(np.float64) + 0.5 * S, rtol=0, atol=1e-4)
    one = V.composite(P[0], S[0], strength=0.25)      # unbatched
    np.testing.assert_array_equal(one, V.composite(P, S, strength=0.25)[0])


def test_a_hard_uint8_matte_is_np_where():
    P, S = _pair(2)
    m = (np.random.default_rng(3).integers(0, 2, (2, 5, 7)) * 255).astype(np.uint8)
    np.testing.assert_array_equal(V.composite(P, S, matte=m), np.where(m[..., None] == 255, P, S))
    np.testing.assert_array_equal(V.composite(P, S, matte=m[:1]), np.where(m[:1, ..., None] == 255, P, S))      # one matte for every frame
    np.testing.assert_array_equal(V.composite(P, S, matte=(m / 255).astype(np.float32)), np.where(m[..., None] == 255, P, S))
    soft = V.composite(P, S, matte=np.full((1, 5, 7), 51, np.uint8), strength=0.5)      # 0.5 * 51 / 255 = 0.1
    np.testing.assert_allclose(soft, 0.1 * P.astype(np.float64) + 0.9 * S, rtol=0, atol=1e-4)


@pytest.mark.parametrize("keep", ("colour", "color", "luma"))
def test_keep_swaps_luminance_and_colour(keep):
    P, S = _pair(4)
    out = V.composite(P, S, keep=keep)
    lum, col = (P, S) if keep != "luma" else (S, P)      # whose luminance, whose colour differences
    np.testing.assert_allclose(_luma(out), _luma(lum), rtol=0, atol=2e-4)      # (the three weights sum to 1 up to float32 rounding)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        np.testing.assert_allclose(out[..., a].astype(np.float64) - out[..., b], col[..., a].astype(np.float64) - col[..., b], rtol=0, atol=1e-4)


def test_a_grey_source_keeps_the_result_grey():
    P, _ = _pair(5)
    S = np.repeat(np.random.default_rng(6).uniform(0, 255, (2, 5, 7, 1)).astype(np.float32), 3, axis=3)
    out = V.composite(P, S, keep="colour")
    np.testing.assert_array_equal(out[..., 0], out[..., 1])
    np.testing.assert_array_equal(out[..., 1], out[..., 2])


def test_composite_refuses_what_the_library_refuses():
    P, S = _pair(7)
    for kw in (dict(strength=-0.1), dict(strength=1.5), dict(strength=float("nan")), dict(keep="hue"), dict(matte=np.zeros((3, 5, 7), np.float32)),
               dict(matte=np.zeros((2, 5, 6), np.float32)), dict(matte=np.zeros((2, 5, 7), np.float64)), dict(strength=[0.5, 0.5, 0.5])):
        with pytest.raises(ValueError):
            V.composite(P, S, **kw)
    with pytest.raises(ValueError):
        V.composite(P, S[:1])


# ---- the launch rule, through the real library (no handle, no GPU)
def _grid(B, DH, DW):
    g, ppp = C.c_uint(0), C.c_int(0)
    assert L.load().rrv_composite_grid(B, DH, DW, C.byref(g), C.byref(ppp)) == RRV_OK
    return g.value, ppp.value


def test_composite_grid_is_the_launch_rule():
    for B in (1, 2, 3, 16, 64):
        for DH, DW in ((1, 1), (1, 3), (5, 7), (16, 64), (32, 32), (37, 53), (512, 512), (1080, 1920), (2160, 3840)):
            grid, ppp = _grid(B, DH, DW)
            groups = -(-B * DH * DW // 4)                    # a thread takes 4 consecutive pixels of the flat run per step
            want = min(max(-(-groups // 256), 1), 2048)      # 256 threads, capped: the rest is grid-strided
            assert grid == want and grid >= 1 and ppp == grid * 256 * 4, (B, DH, DW)
    assert _grid(1, 1024, 2048) == (2048, 2048 * 1024) and _grid(1, 1024, 2049)[0] == 2048


def test_composite_grid_refuses_bad_arguments():
    lib = L.load()
    g, ppp = C.c_uint(0), C.c_int(0)
    assert lib.rrv_composite_grid(1, 4, 4, None, C.byref(ppp)) == RRV_E_ARG
    assert lib.rrv_composite_grid(1, 4, 4, C.byref(g), None) == RRV_E_ARG
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert lib.rrv_composite_grid(*bad, C.byref(g), C.byref(ppp)) == RRV_E_ARG


def test_the_request_struct_is_the_headers():
    """rrv_composite as include/rerevst_hip.h declares it: two pointers and three ints"""
    assert [n for n, _ in L.Composite._fields_] == ["strength", "matte", "matte_dtype", "matte_frames", "keep"]
    assert C.sizeof(L.Composite) == 2 * C.sizeof(C.c_void_p) + 4 * C.sizeof(C.c_int)      # (three ints and the tail padding)
    assert (L.KEEP_NONE, L.KEEP_COLOUR, L.KEEP_LUMA) == (0, 1, 2)
    header = open(os.path.join(kernel_ledger.ROOT, "include", "rerevst_hip.h")).read()
    for name in ("rrv_composite_view_device", "rrv_transfer_composite_view_device", "rrv_transfer_composite", "rrv_composite_grid"):
        assert name in L.SYMBOLS and "int %s(" % name in header


# ---- the Python keywords
def test_python_keyword_validation():
    ok = F.CompositeArgs(0.5, np.zeros((1, 5, 7), np.uint8), "color", 3, 5, 7)
    assert ok.keep == L.KEEP_COLOUR and ok.frames == 1 and ok.dtype == L.DT_U8 and ok.strength.tolist() == [0.5] * 3
    per = F.CompositeArgs([0.0, 0.5, 1.0], np.zeros((3, 5, 7), np.float32), "luma", 3, 5, 7)
    assert per.keep == L.KEEP_LUMA and per.frames == 3 and per.dtype == L.DT_F32 and per.step == 5 * 7 * 4
    req = per.request(1, 2)
    assert req.matte_frames == 2 and req.matte == per.matte.ctypes.data + per.step and req.strength[0] == 0.5 and req.strength[1] == 1.0
    assert F.CompositeArgs(None, np.zeros((5, 7), np.uint8), None, 3, 5, 7).frames == 1      # [H][W]: one matte for every frame
    for bad in (dict(strength=-0.1), dict(strength=1.5), dict(strength=float("nan")), dict(strength=[0.5, 0.5]), dict(keep="hue"),
                dict(matte=np.zeros((2, 5, 7), np.float32)), dict(matte=np.zeros((3, 5, 8), np.float32)), dict(matte=np.zeros((3, 5, 7), np.float64))):
        kw = dict(strength=None, matte=None, keep=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            F.CompositeArgs(kw["strength"], kw["matte"], kw["keep"], 3, 5, 7)
    # no keyword: nothing is built, the call is what it was; with styles: refused in words
    assert F._composite_args(None, None, None, [1.0], None, 3, 5, 7) is None
    for styles in (([1.0], None), (None, np.ones((1, 5, 7), np.float32))):
        with pytest.raises(ValueError, match="blended and masked compositing are not offered"):
            F._composite_args(0.5, None, None, *styles, 3, 5, 7)


# ---- the driver's flags
def test_fade_ramp_is_pinned():
    got = D.fade_strengths(10, 0.8, 3)
    want = [0.0, 0.8 / 3, 1.6 / 3, 0.8, 0.8, 0.8, 0.8, 1.6 / 3, 0.8 / 3, 0.0]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert D.fade_strengths(4, 0.6, 0) == [0.6] * 4
    assert D.fade_strengths(3, 1.0, 5) == [0.0, 0.2, 0.0]      # a fade longer than the video never reaches S
    # by the absolute frame number: the shards of a two-GPU run hold the two halves of the one list
    lo, hi = V.shard_range(10, 1, 2)
    assert D.Compositing(10, strength=0.8, fade=3).kw(range(lo, hi), (4, 4))["strength"] == got[lo:hi]
    for bad in ((10, 1.5, 0), (10, -0.1, 0), (10, float("nan"), 0), (10, 0.5, -1)):
        with pytest.raises(ValueError):
            D.fade_strengths(*bad)


def _grey(path, value, size=(6, 8)):
    D._pil().fromarray(np.full(size, value, np.uint8)).save(path)


def test_matte_directory_order_and_size_check(tmp_path):
    d = tmp_path / "mattes"
    d.mkdir()
    for name, v in (("m_002.png", 30), ("m_000.png", 10), ("m_001.png", 20)):
        _grey(str(d / name), v)
    assert [os.path.basename(p) for p in D.list_mattes(str(d), 3)] == ["m_000.png", "m_001.png", "m_002.png"]
    comp = D.Compositing(3, matte=str(d), keep="luma")
    kw = comp.kw([2, 0], (6, 8))
    assert kw["matte"].shape == (2, 6, 8) and kw["matte"].dtype == np.uint8 and kw["matte"][:, 0, 0].tolist() == [30, 10]
    assert kw["keep"] == "luma" and "strength" not in kw
    with pytest.raises(ValueError, match="one per frame"):
        D.list_mattes(str(d), 4)
    with pytest.raises(ValueError, match="delivered frame"):
        comp.kw([0], (6, 9))
    one = tmp_path / "one.png"
    _grey(str(one), 200)
    shared = D.Compositing(5, strength=0.5, matte=str(one))
    kw = shared.kw([3, 4], (6, 8))
    assert kw["matte"].shape == (1, 6, 8) and int(kw["matte"][0, 0, 0]) == 200 and kw["strength"] == [0.5, 0.5]
    with pytest.raises(ValueError):
        D.list_mattes(str(tmp_path / "missing.png"), 2)
    # an RGB matte is read as its grey
    D.write_image_bgr(str(tmp_path / "rgb.png"), np.full((6, 8, 3), 255, np.uint8))
    assert (D.read_matte(str(tmp_path / "rgb.png"), (6, 8)) == 255).all()


def test_driver_flags_reach_the_flows(tmp_path, monkeypatch):
    """main() hands --strength / --fade / --matte / --keep to the flow it picks, and refuses them in words where they cannot apply"""
    style = tmp_path / "style.png"
    D.write_image_bgr(str(style), np.zeros((8, 8, 3), np.uint8))
    _grey(str(tmp_path / "m.png"), 255)
    seen = {}
    monkeypatch.setattr(D, "stylize_files", lambda *a, **kw: seen.update(files=kw))
    monkeypatch.setattr(D, "stylize_y4m", lambda *a, **kw: seen.update(y4m=kw))
    monkeypatch.setattr(D, "list_frames", lambda pattern: ["a.png"])
    base = ["--style", str(style), "--checkpoint", "synthetic", "--out", str(tmp_path / "out")]
    factory = lambda args, device: object()
    assert D.main(base + ["--frames", "x*.png", "--strength", "0.6", "--fade", "3", "--matte", str(tmp_path / "m.png"), "--keep", "colour"], model_factory=factory) == 0
    assert seen["files"]["composite"] == dict(strength=0.6, fade=3, matte=str(tmp_path / "m.png"), keep="colour")
    assert D.main(base + ["--frames", "in.y4m", "--keep", "luma", "--work-size", "64x48", "--out-size", "source", "--guided"], model_factory=factory) == 0
    assert seen["y4m"]["composite"] == dict(strength=None, fade=0, matte=None, keep="luma") and seen["y4m"]["guided"] == (4, 1e-3)
    assert D.main(base + ["--frames", "x*.png"], model_factory=factory) == 0 and seen["files"]["composite"] is None
    for bad in (["--strength", "1.5"], ["--strength", "nan"], ["--fade", "-1"], ["--matte", str(tmp_path / "none.png")], ["--keep", "hue"]):
        with pytest.raises(SystemExit):
            D.main(base + ["--frames", "x*.png"] + bad, model_factory=factory)
    with pytest.raises(SystemExit):      # multi-style interpolation: as the neighbouring options
        D.main(["--style", str(style), str(style), "--checkpoint", "synthetic", "--out", str(tmp_path / "out"), "--frames", "x*.png", "--strength", "0.5"],
               model_factory=factory)

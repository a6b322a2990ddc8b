"""CPU checks of the masked multi-style entries (rrv_transfer_image_mask_device, rrv_transfer_mask_batch[_u8]; transfer_batch /
transfer_frames / transfer_tensor with style_masks): declared in the header with the stated prototypes, listed in the ctypes
table, exported by the built library; the Python check of `style_masks` rejects a wrong shape, a wrong dtype and
style_weights given as well before the library is called; and the numpy reference of the model (tests/mask_ref.py) agrees
with the oracle's per-frame multi-style interpolation for a mask that is constant over the frame.

The last two tests (the block means of an aligned mask, mask_ref against the oracle) exercise tests/mask_ref.py and the oracle only:
they validate the REFERENCE the GPU tests are held against, not the feature, and pass without the library.  The tests above them
need the new symbols and keywords.  The C-level RRV_E_ARG cases below need a device to create a handle and return early without
one; tests/test_gpu_mask_blend.py repeats them on a live handle."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from conftest import assert_pre_close, IMG_ATOL
import mask_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("rerevst-code_amd._lib")
F = importlib.import_module("rerevst-code_amd.framework")
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rerevst_hip.h")).read(), flags=re.S)
RRV_E_ARG = -1
NEW = ("rrv_transfer_image_mask_device", "rrv_transfer_mask_batch", "rrv_transfer_mask_batch_u8")


def _lib():
    importlib.import_module("rerevst-code_amd.build").build_lib(verbose=False)
    return L.load()


def _params(name):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, HDR)
    assert m, "%s is not declared" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_table_and_library_carry_the_entries():
    assert _params("rrv_transfer_image_mask_device") == [
        "rrv_handle h", "const void* d_in", "rrv_image_desc in", "int B", "int H", "int W", "const float* d_mask", "int n_styles",
        "int mask_images", "void* d_out", "rrv_image_desc out", "int flags", "void* hip_stream"]
    host = ["rrv_handle h", "const uint8_t* frames_bgr", "int B", "int H", "int W", "const float* mask", "int n_styles", "int mask_images",
            "int pad_crop"]
    assert _params("rrv_transfer_mask_batch") == host + ["float* out_bgr"]
    assert _params("rrv_transfer_mask_batch_u8") == host + ["uint8_t* out_bgr"]
    assert L.SYMBOLS["rrv_transfer_mask_batch_u8"] == L.SYMBOLS["rrv_transfer_mask_batch"] and "rrv_transfer_mask_batch" in L.U8_TWINS
    assert len(L.SYMBOLS["rrv_transfer_image_mask_device"][1]) == 13 and len(L.SYMBOLS["rrv_transfer_mask_batch"][1]) == 10
    assert L.SYMBOLS["rrv_transfer_image_mask_device"][1][2] is L.ImageDesc and L.SYMBOLS["rrv_transfer_image_mask_device"][1][10] is L.ImageDesc
    lib = _lib()
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(lib, name), name


def test_argument_checks_need_no_device():
    lib = _lib()
    u8 = L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_PIXEL)
    f32 = L.ImageDesc(L.DT_F32, L.LAY_HWC_BGR, L.SP_PIXEL)
    frames = np.zeros((2, 64, 64, 3), np.uint8)
    out = np.zeros((2, 64, 64, 3), np.float32)
    mask = np.full((2, 2, 64, 64), 0.5, np.float32)
    fp, op, mp = (a.ctypes.data_as(C.c_void_p) for a in (frames, out, mask))
    mf = mask.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.rrv_transfer_image_mask_device(None, fp, u8, 2, 64, 64, mp, 2, 2, op, f32, 0, None) == RRV_E_ARG
    for fn in (lib.rrv_transfer_mask_batch, lib.rrv_transfer_mask_batch_u8):
        assert fn(None, fp, 2, 64, 64, mf, 2, 2, 0, op) == RRV_E_ARG
    h = C.c_void_p()
    if lib.rrv_create(0, C.byref(h)) != 0:
        return                                      # no GPU here: a handle cannot exist
    try:      # (the host buffers stand in for device ones: every call below is refused before anything reads them)
        img = lib.rrv_transfer_image_mask_device
        assert img(h, fp, u8, 2, 64, 64, None, 2, 2, op, f32, 0, None) == RRV_E_ARG                   # null mask
        assert img(h, None, u8, 2, 64, 64, mp, 2, 2, op, f32, 0, None) == RRV_E_ARG
        for mi in (0, 3, -1):
            assert img(h, fp, u8, 2, 64, 64, mp, 2, mi, op, f32, 0, None) == RRV_E_ARG, mi
        for ns in (0, -1, L.MAX_STYLES + 1):
            assert img(h, fp, u8, 2, 64, 64, mp, ns, 2, op, f32, 0, None) == RRV_E_ARG, ns
        assert img(h, fp, u8, 2, 64, 64, mp, 2, 2, op, f32, L.TF_FRAME_MODE, None) == RRV_E_ARG
        assert img(h, fp, u8, 2, 64, 64, mp, 2, 2, op, f32, L.TF_WEIGHTS_DEVICE, None) == RRV_E_ARG
        for fn in (lib.rrv_transfer_mask_batch, lib.rrv_transfer_mask_batch_u8):
            assert fn(h, fp, 2, 64, 64, None, 2, 2, 0, op) == RRV_E_ARG
            assert fn(h, fp, 2, 64, 64, mf, 2, 3, 0, op) == RRV_E_ARG
            for ns in (0, L.MAX_STYLES + 1):
                assert fn(h, fp, 2, 64, 64, mf, ns, 2, 0, op) == RRV_E_ARG
    finally:
        lib.rrv_destroy(h)


def test_framework_signatures():
    for name in ("transfer_batch", "transfer_frames", "transfer_tensor"):
        for cls in (F.Stylization, F.MultiStyleStylization):
            assert inspect.signature(getattr(cls, name)).parameters["style_masks"].default is None, (cls.__name__, name)


def test_style_mask_args_accepts():
    m = np.ones((3, 2, 16, 24), np.float32)
    a = F.style_mask_args(m, None, 3, 16, 24, 2, 0)
    assert a.S == 2 and a.images == 3 and a.dev is None and a.host.dtype == np.float32 and a.host.flags.c_contiguous
    a = F.style_mask_args(m[0], None, 5, 16, 24, 4, 0)
    assert a.S == 2 and a.images == 1
    a = F.style_mask_args(np.ones((4, 8, 16), np.float32)[:, :, ::2], None, 1, 8, 8, 4, 0)      # not contiguous: copied
    assert a.host.flags.c_contiguous and a.host.shape == (4, 8, 8)


@pytest.mark.parametrize("case", ["wrong_B", "wrong_H", "wrong_W", "rank2", "rank5", "float64", "uint8", "list", "too_many_styles",
                                  "above_max_styles", "no_styles", "with_weights", "frame_mode"])
def test_style_mask_args_rejects(case):
    m, w, B, sn, ug = np.ones((3, 2, 16, 24), np.float32), None, 3, 2, True
    if case == "wrong_B":
        B = 4
    elif case == "wrong_H":
        m = np.ones((3, 2, 15, 24), np.float32)
    elif case == "wrong_W":
        m = np.ones((2, 16, 25), np.float32)
    elif case == "rank2":
        m = np.ones((16, 24), np.float32)
    elif case == "rank5":
        m = np.ones((1, 3, 2, 16, 24), np.float32)
    elif case == "float64":
        m = m.astype(np.float64)
    elif case == "uint8":
        m = m.astype(np.uint8)
    elif case == "list":
        m = m.tolist()
    elif case == "too_many_styles":
        m = np.ones((3, 3, 16, 24), np.float32)
    elif case == "above_max_styles":
        m, sn = np.ones((3, 9, 16, 24), np.float32), 16
    elif case == "no_styles":
        m = np.ones((3, 0, 16, 24), np.float32)
    elif case == "with_weights":
        w = [0.5, 0.5]
    elif case == "frame_mode":
        ug = False
    with pytest.raises(ValueError):
        F.style_mask_args(m, w, B, 16, 24, sn, 0, use_Global=ug)


def test_methods_refuse_masks_before_the_library_is_called():
    """a wrong shape, a wrong dtype and style_weights given as well never reach the library"""
    class Lib:
        def __getattr__(self, name):
            raise AssertionError("library entry %s called" % name)

    frames = np.zeros((2, 16, 16, 3), np.uint8)
    good = np.ones((2, 1, 16, 16), np.float32)
    for kw in (dict(style_masks=np.ones((2, 1, 16, 8), np.float32)), dict(style_masks=good.astype(np.float64)),
               dict(style_masks=good, style_weights=[[1.0]] * 2), dict(style_masks=np.ones((3, 1, 16, 16), np.float32))):
        s = F.Stylization.__new__(F.Stylization)
        s._lib, s._h, s.use_Global, s.style_num, s.device = Lib(), None, True, 1, 0
        for fn in (s.transfer_batch, s.transfer_frames):
            with pytest.raises(ValueError):
                fn(frames, out=np.zeros((2, 16, 16, 3), np.float32), **kw)


def test_block_means_of_an_aligned_mask_are_one_hot():
    H, W = 48, 72
    m = np.zeros((3, H, W), np.float32)
    m[0, :16, :] = 1
    m[1, 16:, :40] = 1
    m[2, 16:, 40:] = 1
    lv = mask_ref.level_masks(m)
    assert [l.shape for l in lv] == [(3, 48, 72), (3, 24, 36), (3, 12, 18), (3, 6, 9)]
    for l in lv:
        assert l.dtype == np.float32 and np.all((l == 0) | (l == 1)) and np.all(l.sum(axis=0) == 1)
    # an edge off the 8-pixel grid mixes at the coarse levels only
    m2 = np.zeros((2, 16, 16), np.float32)
    m2[0, :, :4] = 1
    m2[1, :, 4:] = 1
    lv2 = mask_ref.level_masks(m2)
    assert np.all((lv2[2] == 0) | (lv2[2] == 1)) and lv2[3][0, 0, 0] == np.float32(0.5) and lv2[3][1, 0, 0] == np.float32(0.5)
    # the level means are block means (exact here: small dyadic values)
    r = np.random.default_rng(0).integers(0, 8, size=(1, 16, 24)).astype(np.float32)
    np.testing.assert_array_equal(mask_ref.level_masks(r)[3][0], r[0].reshape(2, 8, 3, 8).mean(axis=(1, 3)))
    # rows and columns beyond the multiple of 8 are ignored; the reflect pad is the frame's
    np.testing.assert_array_equal(mask_ref.level_masks(np.pad(r, ((0, 0), (0, 5), (0, 3)), constant_values=9))[0], r)
    import rerevst_oracle as O
    pm = mask_ref.pad_mask(r, O.padded_size(16), O.padded_size(24))
    assert pm.shape == (1, 192, 192)
    np.testing.assert_array_equal(pm[0], O.reflect_pad(r[0][..., None], 192, 192)[..., 0])


def test_constant_mask_is_the_oracles_multistyle_interpolation(pkg, oracle, weights):
    """mask_ref with M[s] == w_s against oracle.MultiStylization.transfer with style_weight = w.  The blended parameters are
    the same float32 sums in the same order; apply_filter is a per-pixel einsum here and one matrix product there, so the
    outputs differ by float32 summation order: compared within assert_pre_close (the project's pre-clamp bound) and IMG_ATOL."""
    S, H, W = 2, 32, 40
    styles = [pkg.synth_style(32, 32, kind="smooth", seed=7 + k) for k in range(S)]
    frames = [pkg.synth_frame(i, H, W, kind="smooth") for i in range(3)]
    ms = oracle.MultiStylization(weights, style_num=S)
    ms.prepare_style(styles)
    feats = [ms.generate_content_features(f) for f in frames]
    ms.add_patch(feats[0])
    ms.add_patch(feats[2])
    ms.compute_norm()
    states = [ms.get_state(k) for k in range(S)]
    w = np.array([0.3, 0.7], np.float32)
    mask = np.broadcast_to(w[:, None, None], (S, H, W)).astype(np.float32)
    want = ms.transfer(feats[1], style_weight=w, return_preclamp=True)
    got = mask_ref.transfer(ms.net, states, frames[1], mask, return_preclamp=True)
    assert got.shape == want.shape == (1, H, W, 3)
    assert_pre_close(got[0], want[0])
    assert np.abs(oracle.tensor_to_image(got) - oracle.tensor_to_image(want)).max() <= IMG_ATOL
    # a one-hot constant mask is single-style transfer
    one = np.zeros((S, H, W), np.float32)
    one[1] = 1
    assert_pre_close(mask_ref.transfer(ms.net, states, frames[1], one, return_preclamp=True)[0],
                     ms.per_style[1].dec.run(feats[1], ms.per_style[1].F_style, compute=False)[0])
    # and a mask that varies changes the picture
    half = np.zeros((S, H, W), np.float32)
    half[0, :, :16] = 1
    half[1, :, 16:] = 1
    assert np.abs(mask_ref.transfer(ms.net, states, frames[1], half) - oracle.tensor_to_image(want)).max() > 1.0

"""The delivery stage without a GPU: its ledger (every deliver_k symbol of librerevst_stages.so's gfx950 code object is named here
and held by one test of tests/test_gpu_deliver.py; the rule of tests/kernel_ledger.py, only symbol names are read), the out_size= and
--out-size argument handling, and tests/deliver_ref.py: its tolerances against the header's operation count and its float64 values
against torch's bilinear interpolation on an upscale."""
import importlib

import numpy as np
import pytest

import deliver_ref as DR
import kernel_ledger as KL
import resample_ref as R

L = importlib.import_module("rerevst-code_amd._lib")
assert "rrv_deliver_view_device" in L.SYMBOLS      # this file is about the delivery stage the library offers: without its entries nothing here is collected
FW = importlib.import_module("rerevst-code_amd.framework")
D = importlib.import_module("rerevst-code_amd.driver")

# ---- the delivery stage's ledger: kernel symbol -> the test of tests/test_gpu_deliver.py that holds THAT instantiation to the
# reference (deliver_k<OUT>, OUT the output form: float32 HWC / CHW, uint8 HWC / CHW, 8-bit YUV, uint16 YUV; each its own compile)
GPU = "tests/test_gpu_deliver.py::"
DELIVER_LEDGER = {
    "deliver_k<0>": GPU + "test_deliver_f32_hwc_against_reference",
    "deliver_k<1>": GPU + "test_deliver_f32_chw_against_reference",
    "deliver_k<2>": GPU + "test_deliver_u8_hwc_bit_exact",
    "deliver_k<3>": GPU + "test_deliver_u8_chw_bit_exact",
    "deliver_k<4>": GPU + "test_deliver_yuv8_bit_exact",
    "deliver_k<5>": GPU + "test_deliver_yuv16_bit_exact",
}


def test_deliver_library_ledger():
    KL.check_stage_ledger(DELIVER_LEDGER, "deliver", one_test_each=True)


def test_out_size_argument():
    assert FW._out_size((37, 53), (16, 24)) == (37, 53)
    assert FW._out_size([2160, 3840], (1080, 1920)) == (2160, 3840)
    assert FW._out_size(np.array([50, 300]), (40, 200)) == (50, 300)
    assert FW._out_size("source", (70, 77)) == (70, 77)
    for bad in ("Source", "4k", (37,), (1, 2, 3), (0, 5), (5, -1), (2.5, 4), 7, None, ("a", "b")):
        with pytest.raises(ValueError):
            FW._out_size(bad, (16, 24))
    with pytest.raises(ValueError):      # refused with multi-style interpolation and masks, before the GPU is looked at
        FW._no_styles_with_out_size([1.0], None)
    with pytest.raises(ValueError):
        FW._no_styles_with_out_size(None, np.ones((1, 8, 8), np.float32))
    FW._no_styles_with_out_size(None, None)


def test_driver_out_size_argument(tmp_path):
    assert D.parse_out_size("3840x2160") == (2160, 3840)
    assert D.parse_out_size("128X96") == (96, 128)
    assert D.parse_out_size("source") == "source" and D.parse_out_size("SOURCE") == "source"
    for bad in ("3840", "3840x", "ax4", "0x8", "8x-1", "1x2x3", ""):
        with pytest.raises(ValueError):
            D.parse_out_size(bad)
    base = ["--frames", str(tmp_path / "*.png"), "--checkpoint", "synthetic", "--out", str(tmp_path / "out")]

    def no_model(args, device):
        raise AssertionError("refused before a model is built")
    with pytest.raises(SystemExit):      # refused together with multi-style interpolation, as --work-size is
        D.main(["--style", "a.png", "b.png", "--out-size", "source"] + base, model_factory=no_model)
    with pytest.raises(SystemExit):
        D.main(["--style", "a.png", "--out-size", "12by8"] + base, model_factory=no_model)


def test_tolerances_are_the_headers_operation_count():
    for (H, W), (DH, DW) in DR.SHAPES:
        t = R.tolerance(H, W, DH, DW)
        # the resampler's bound: one rounding per tap and axis, the weights' and the value's own, at the scale of a pixel value
        assert t == (R.taps(H, DH)[1].max() + R.taps(W, DW)[1].max() + 6) * 2.0 ** -24 * 255.0
        assert DR.tolerance("pixel", H, W, DH, DW) == t
        assert DR.tolerance("unit", H, W, DH, DW) == t / 255.0 + 2.0 ** -24
        assert DR.tolerance("norm", H, W, DH, DW) == (t / 255.0 + 2.0 ** -23) / 0.224 + 2.0 ** -23
    assert min(DR.STD) == 0.224 and (1.0 - min(DR.MEAN)) / 0.224 < 4.0      # what the NORM bound assumes: the result is below 4
    with pytest.raises(ValueError):
        DR.tolerance("srgb", 8, 8, 8, 8)


UP_SHAPES = (((16, 24), (37, 53)), ((16, 24), (128, 192)), ((40, 200), (50, 300)), ((7, 13), (7, 40)))


@pytest.mark.parametrize("src,dst", UP_SHAPES, ids=["%dx%d_to_%dx%d" % (s + d) for s, d in UP_SHAPES])
def test_reference_agrees_with_torch_bilinear_on_an_upscale(src, dst):
    import torch
    x = np.random.default_rng(src[1] * 100 + dst[0]).uniform(0, 255, (2, src[0], src[1], 3)).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), size=dst, mode="bilinear", align_corners=False)
    got = DR.float_ref(x, dst[0], dst[1])
    err = np.abs(got - want.permute(0, 2, 3, 1).numpy()).max()
    print("max |reference - torch float64| = %.3g" % err)
    assert err <= 1e-9
    # and the other forms are that value's: planar RGB, UNIT, NORM
    np.testing.assert_array_equal(DR.float_ref(x, dst[0], dst[1], chw=True), got[..., ::-1].transpose(0, 3, 1, 2))
    np.testing.assert_allclose(DR.float_ref(x, dst[0], dst[1], "unit") * 255.0, got, rtol=0, atol=1e-10)
    np.testing.assert_allclose((DR.float_ref(x, dst[0], dst[1], "norm")[..., ::-1] * DR.STD + DR.MEAN) * 255.0, got[..., ::-1], rtol=0, atol=1e-10)


def test_integer_references():
    v = np.array([[[[-3.0, 0.5, 1.5], [2.5, 254.5, 255.5], [300.0, 127.49, 127.51]]]], np.float32)
    np.testing.assert_array_equal(DR.to_uint8(v)[0, 0], [[0, 0, 2], [2, 254, 255], [255, 127, 128]])      # half to even, clamped
    np.testing.assert_array_equal(DR.u8_ref(v, chw=True)[0, :, 0, 0], [2, 0, 0])                         # RGB planes of a BGR pixel
    img = np.random.default_rng(3).uniform(0, 255, (2, 5, 7, 3)).astype(np.float32)
    assert DR.yuv_ref(img, "nv12").shape == (2, 5 * 7 + 2 * 3 * 4) and DR.yuv_ref(img, "p010").dtype == np.uint16

"""The item boundary of the persistent transform-domain kernels (conv_f43_k, the upsample-fused conv_wino_k): set-up of the next item
inside the peeled last two chunks, the epilogue's fields and lane coordinates read where it starts.  A handle created under RRV_CUS=8
runs every launch on eight workgroups, so each workgroup chains many items (image changes included); one created without it runs one
item or fewer per workgroup at these sizes.  Fixed mode 2: all ten packed layers on conv_f43_k.  Three frames per call.
  72 x 104: no level is a multiple of 32 wide or high — every item takes the edge path;
  64 x 96 : level 0 is whole 32 x 32 items, the half-resolution level (32 x 48) mixes interior and edge items.
Checked on the pre-clamp image and every layer tap: bit for bit between the two handles, and against the float64 references of
tests/layer_ref.py with the families' K.  RRV_P8 (read when the handle is created, as in test_channel_chunk_major_tensors_change_no_bit):
the default and 0."""
import importlib

import numpy as np
import pytest

import layer_ref as LR
import test_gpu_layers as TL
from conftest import fixed_kernels, forced_family
from state_bounds import load_golden

pytestmark = pytest.mark.gpu

SIZES = [(72, 104), (64, 96)]
B = 3
CUS = 8


def _launch(pkg, weights, frames, blob, p8, cus):
    with fixed_kernels(mode=2), TL.env(**({"RRV_CUS": cus} if cus else {})):
        return TL.launch(pkg, weights, frames, blob, 2, p8=p8)


def _all_taps(s, H, W, b, frame, names):
    t = TL.Taps(s, H, W, b, frame)
    return {n: t.get(n) for n in names}, t.layout


@pytest.mark.parametrize("p8", [3, 0], ids=["p8", "nhwc"])
@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_chained_items_change_no_bit(pkg, weights, hw, p8):
    H, W = hw
    blob = load_golden("global_a")["state"]
    st = LR.parse_state(blob)
    frames = TL.frames_for(pkg, B, H, W, seed=900)
    names = [n for n in LR.STAGES] + list(LR.FOLDED)
    few, seq_few, out_few = _launch(pkg, weights, frames, blob, p8, CUS)
    try:
        many, seq_many, out_many = _launch(pkg, weights, frames, blob, p8, None)
        try:
            assert [n for n, _ in seq_few] == [n for n, _ in seq_many]            # the same kernels either way
            np.testing.assert_array_equal(out_few.cpu().numpy(), out_many.cpu().numpy())
            for b in range(B):
                a, la = _all_taps(few, H, W, b, frames[b], names)
                c, lc = _all_taps(many, H, W, b, frames[b], names)
                assert la == lc
                for n in names:
                    np.testing.assert_array_equal(a[n], c[n], err_msg="%s image %d" % (n, b))
        finally:
            many.close()
        for b in range(B):
            fam, lay = TL.check_image(few, weights, st, seq_few, H, W, b, frames[b])
            if not forced_family():
                assert all(fam[n] == "f43" for n in TL.ENC_F43 + TL.DEC_F43), fam
                assert fam["a4"] == fam["a3"] == fam["a2"] == "ups"
                assert all(lay[n] == (1 if p8 else 0) for n in ("c11",) + TL.ENC_F43[:-1] + ("a4", "a3", "a2")), lay
    finally:
        few.close()


def _grouped(pkg, weights, oracle, styles, frames, wts, p8, cus):
    """One grouped multi-style launch (rrv_transfer_features_batch, per-image blended state) on a fresh handle:
    (handle, launch sequence from ResidualBlock on, output, the styles' blobs)."""
    with fixed_kernels(mode=2), TL.env(RRV_P8=p8, **({"RRV_CUS": cus} if cus else {})):
        s = pkg.MultiStyleStylization(weights, cuda=True, style_num=len(styles))
        s.set_f43(2)
        s.prepare_style(styles)
        feats = [s.generate_content_features(f) for f in frames]
        s.clean()
        for i in (0, 2):
            s.add_patch(feats[i])
        s.compute_norm()
        blobs = [s.get_state(k) for k in range(len(styles))]
        s.set_multistyle_group(16)
        s.profile_begin()
        out = np.array(s.transfer_many(feats, wts))
        rows = [r[0] for r in s.profile_end()]
        s.sync()
    assert [n.split("@")[0] for n in rows[:len(frames)]] == ["pointwise"] * len(frames), rows
    rows = rows[len(frames):]
    seq = [("", False)] * 9              # the encoder's nine launches did not run (cached features)
    for i, n in enumerate(rows):
        if not n.startswith("sum_parts"):
            seq.append((n, i + 1 < len(rows) and rows[i + 1].startswith("sum_parts")))
    assert len(seq) == LR.N_LAUNCHES, rows
    return s, seq, out, blobs


@pytest.mark.parametrize("p8", [3, 0], ids=["p8", "nhwc"])
@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_chained_items_with_per_image_state(pkg, weights, oracle, hw, p8):
    """The same pair through the grouped multi-style entry: two styles, per-image weights, so every image of the launch has a state
    set of its own (ConvP::par_bstride) and an image change inside a workgroup's chain restages the epilogue parameters."""
    V = importlib.import_module("rerevst-code_amd.video")
    H, W = hw
    styles = [pkg.synth_style(64, 64, kind="smooth", seed=17 + k) for k in range(2)]
    frames = [pkg.synth_frame(910 + i, H, W, kind="smooth") for i in range(B)]
    wts = [V.ramp_weights(i, B, 2, blend="all") for i in range(B)]
    names = tuple(n for n in LR.STAGES if LR.STAGES[n][0] >= 13) + LR.FOLDED
    few, seq_few, out_few, blobs = _grouped(pkg, weights, oracle, styles, frames, wts, p8, CUS)
    try:
        many, seq_many, out_many, _ = _grouped(pkg, weights, oracle, styles, frames, wts, p8, None)
        try:
            assert [n for n, _ in seq_few] == [n for n, _ in seq_many]
            np.testing.assert_array_equal(out_few, out_many)
            for b in range(B):
                np.testing.assert_array_equal(few.debug_state_set(0, b), many.debug_state_set(0, b))
                a, la = _all_taps(few, H, W, b, None, names)
                c, lc = _all_taps(many, H, W, b, None, names)
                assert la == lc
                for n in names:
                    np.testing.assert_array_equal(a[n], c[n], err_msg="%s image %d" % (n, b))
        finally:
            many.close()
        for b in range(B):
            fam, _ = TL.check_image(few, weights, LR.parse_state(few.debug_state_set(0, b)), seq_few, H, W, b, None, names=names)
            if not forced_family():
                assert all(fam[n] == "f43" for n in TL.DEC_F43), fam          # per-image PARAMETERS are conv_f43_k's too
                assert fam["a4"] == fam["a3"] == fam["a2"] == "ups"
    finally:
        few.close()

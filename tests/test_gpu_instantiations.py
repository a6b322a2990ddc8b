"""The kernel instantiations that the public API can launch and that no other layer suite holds to a reference (tests/kernel_ledger.py
names, for every kernel of the library, the test that does): each against the float64 stage references of tests/layer_ref.py on its
own GPU input, one profiled call per case on a fresh handle, the profile's row names asserted.
  a  conv_wino_split_k<5,1>: conv4_1 + per-image Decoder.norm[0] of blended frames, on states that DIFFER in norm[0]
  b  pointwise_k's per-image Decoder.norm[0] of cached features in a grouped launch
  c  conv_wino_split_k<2,1> (unsplit) and <0,1> at split 4: filter_down with per-image folded weights
  d  conv_mfma_k<64,9,65> / <128,9,1> / <128,9,65> / <128,9,5>: the direct-form encoder behind RRV_DIRECT_LAYERS
Every case that claims per-image state carries a negative control: an image evaluated with its neighbour's state set must fail."""
import os

import numpy as np
import pytest
import torch

import layer_ref as LR
import mask_ref
import test_gpu_layers as TL
import test_gpu_frame_mode_layers as FL
from conftest import fixed_kernels
from state_bounds import load_golden
from test_gpu_mask_blend import _golden_setup, _mixed

pytestmark = pytest.mark.gpu

RATIOS = {}      # (case, family) -> the largest measured ratio


def _note(case, f, ratio):
    if f is not None and ratio > RATIOS.get((case, f), 0.0):
        RATIOS[case, f] = ratio


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (case, f), r in sorted(RATIOS.items()):
        print("\n[instantiation ratios] %s %s=%.3g" % (case, f, r), end="")
    print()


@pytest.fixture(scope="module")
def states(pkg, oracle, weights):
    """Three computed states, every pair different in Decoder.norm[0] (mask_ref.distinct_states asserts it)."""
    return mask_ref.distinct_states(*_golden_setup(pkg, oracle, weights, "multistyle_s4")[:2])[:3]


# distinct per frame, every style with a non-zero weight
WTS = np.array([[0.6, 0.3, 0.1], [0.2, 0.5, 0.3], [0.1, 0.25, 0.65]], np.float32)
FIVE = ("c41", "d", "f1", "f2", "f3")


def seq_of(rows):
    """[(row name, followed by sum_parts)] of the one launch sequence in `rows`, from its conv_first on."""
    first = [i for i, n in enumerate(rows) if n.startswith("conv_first")]
    assert len(first) == 1, rows
    rows = rows[first[0]:]
    seq = [(n, i + 1 < len(rows) and rows[i + 1].startswith("sum_parts")) for i, n in enumerate(rows) if not n.startswith("sum_parts")]
    assert len(seq) == LR.N_LAUNCHES, rows
    return seq


def blend_launch(pkg, weights, blobs, frames, wts, mode=None):
    """One profiled transfer_batch(style_weights=) on a fresh handle holding `blobs` as its styles' states: one group, one launch
    sequence with a blended state set per image.  mode: None = the default kernel choice, else fixed_kernels(mode)."""
    with TL.env(RRV_P8=3, RRV_F43_LAYERS=hex(0x3ff)):
        s = pkg.MultiStyleStylization(weights, cuda=True, style_num=len(blobs))
    try:
        for k, b in enumerate(blobs):
            s.set_state(b, k)
        torch.cuda.synchronize()

        def run():
            s.profile_begin()
            s.transfer_batch(frames, style_weights=wts)
            rows = [r[0] for r in s.profile_end()]
            s.sync()
            return rows

        if mode is None:
            rows = run()
        else:
            with fixed_kernels(s, mode=mode):
                rows = run()
        return s, seq_of(rows)
    except BaseException:
        s.close()
        raise


def checked(case, *a, **kw):
    """TL.check_image with the ratios it measures recorded under `case`."""
    saved = dict(TL.RATIOS)
    for f in TL.RATIOS:
        TL.RATIOS[f] = 0.0
    try:
        return TL.check_image(*a, **kw)
    finally:
        for f, r in TL.RATIOS.items():
            _note(case, f, r)
            TL.RATIOS[f] = max(saved[f], r)


def stage_passes(t, name, weights, st, seq):
    """Stage `name` of the taps t against its reference on state st: (inside its bound everywhere, worst fraction of the bound)."""
    li, inputs, op, _ = LR.STAGES[name]
    f = LR.family_of(*seq[li])
    got, inp = t.get(name), [t.get(i) for i in inputs]
    ok_all, worst_all = True, 0.0
    for y0, y1 in LR.strips(got.shape[0]):
        ok, worst, _ = LR.check(got[y0:y1], *op(inp, weights, st, y0, y1), LR.K[f])
        ok_all, worst_all = ok_all and ok, max(worst_all, worst)
    return ok_all, worst_all


def check_blended_set(case, s, blobs, wts, b):
    """Image b's state set of the last grouped launch against the float64 blend of the styles' blobs (blend_sets_k)."""
    blob = s.debug_state_set(0, b)
    ref, mag = LR.blend_ref(blobs, wts)
    err = np.abs(blob.astype(np.float64) - ref)
    ratio = float((err / np.maximum(LR.U * mag, 1e-300)).max())
    print("[ratio] %s image %d blend stat %.3g" % (case, b, ratio))
    assert np.all(err <= LR.K["stat"] * LR.U * mag), "image %d: blended set at ratio %.3g" % (b, ratio)
    _note(case, "stat", ratio)
    return LR.parse_state(blob)


def down_rows(seq):
    """the three KernelFilter down convolutions of a launch sequence: (kernel of the row, followed by sum_parts)"""
    rows = [(n.split("@")[0], sp) for n, sp in seq if "@512x32@" in n]
    assert len(rows) == 3, seq
    return rows


def assert_split(pkg, s, seq, H, W, split):
    """The slices of filter_down from the dpart tap's channel count (refused at split 1) and from the rows' kernel names."""
    if split > 1:
        _, lay, ch = s.debug_tensor_ex(0, LR.TAP["dpart"], H, W, 0)
        assert lay == 0 and ch == 32 * split, ch
        assert down_rows(seq) == [("conv_wino<0>", True)] * 3, down_rows(seq)
    else:
        with pytest.raises(pkg.RRVError, match="did not write|no such tensor"):
            s.debug_tensor_ex(0, LR.TAP["dpart"], H, W, 0)
        assert down_rows(seq) == [("conv_wino<E_LRELU>", False)] * 3, down_rows(seq)


# ---- a. blended from frames: conv4_1 with per-image Decoder.norm[0] ---------------------------------------------------------------

@pytest.mark.parametrize("kind", ["default", "fixed2"])
def test_blended_frames_per_image_conv4_1(pkg, weights, states, kind):
    """Three frames of 72 x 104 (no level a multiple of 32) blended from three states that differ in Decoder.norm[0], through
    transfer_batch(style_weights=): every encoder and decoder stage of images 0 and 2 on that image's own blended set, the sets
    against the float64 blend; image 2's c41 on image 0's set fails."""
    B, H, W = 3, 72, 104
    case = "a/" + kind
    frames = _mixed(pkg, 80, B, H, W)
    s, seq = blend_launch(pkg, weights, states, frames, WTS, mode=None if kind == "default" else 2)
    try:
        assert seq[8][0].startswith("conv_wino<") and "@256x512@" in seq[8][0], seq[8]       # conv4_1: the row-split kernel
        s.debug_state_set(0, 1)                                 # the launch had per-image state: conv() took the per-image row
        with pytest.raises(pkg.RRVError, match="did not write this image"):
            s.debug_state_set(0, B)
        sets = {}
        for b in (0, 2):
            sets[b] = check_blended_set(case, s, states, WTS[b], b)
            fam, lay = checked(case, s, weights, sets[b], seq, H, W, b, frames[b])
            assert fam["c41"] == fam["f3"] == "f23" and fam["d"] == "splitk"
            assert fam["xs4"] == fam["a4"] == fam["a3"] == fam["a2"] == "ups"
            if kind == "default" and os.environ.get("RRV_F43") != "2":        # under 256 items per layer: F(2x2,3x3) throughout
                assert all(fam[n] == "f23" for n in TL.ENC_F43 + TL.DEC_F43), fam
            if kind == "fixed2" and os.environ.get("RRV_F43") != "0":       # the P8 chain inside a grouped launch
                assert all(fam[n] == "f43" for n in TL.ENC_F43 + TL.DEC_F43), fam
                assert all(lay[n] == 1 for n in ("c11",) + TL.ENC_F43[:-1]) and lay["p3"] == 0, lay
        t2 = TL.Taps(s, H, W, 2, frames[2])
        ok, worst = stage_passes(t2, "c41", weights, sets[0], seq)
        print("[control] %s image 2 c41 on set 0: %.3g of the bound" % (case, worst))
        assert not ok, "image 2's c41 passes on image 0's state set (%.3g of the bound)" % worst
    finally:
        s.close()


# ---- b. cached features: pointwise_k with per-image Decoder.norm[0] ------------------------------------------------------------------

def test_cached_features_per_image_pointwise(pkg, weights, states):
    """Three cached features in one grouped transfer_many launch: c41 of each image against float64 conv4_1 + ReLU of the caching
    call's p3, normalised and clamped with the image's own blended set.  The caching call keeps its encoder taps in a plan of its
    own that no tap reads, so p3 comes from a plain F(2x2,3x3) launch of the same frames on a second handle: the same kernels on
    the same input, the same bits.  (Were they not, the reference would only be further from c41: nothing can pass by it.)"""
    B, H, W = 3, 72, 104
    case = "b"
    frames = _mixed(pkg, 90, B, H, W)
    donor, dseq, _ = TL.launch(pkg, weights, frames, states[0], 0)
    s = pkg.MultiStyleStylization(weights, cuda=True, style_num=len(states))
    try:
        assert all(LR.family_of(*dseq[i]) == "f23" for i in range(1, 8)), dseq
        p3 = [TL.Taps(donor, H, W, b, frames[b]).get("p3") for b in range(B)]
        for k, blob in enumerate(states):
            s.set_state(blob, k)
        feats = [s.generate_content_features(f) for f in frames]
        s.set_multistyle_group(16)
        s.profile_begin()
        s.transfer_many(feats, WTS.tolist())
        rows = [r[0] for r in s.profile_end()]
        s.sync()
        assert [n.split("@")[0] for n in rows[:B + 1]] == ["pointwise"] * B + ["conv_wino<0>"], rows
        sets, got = {}, {}
        for b in range(B):
            sets[b] = check_blended_set(case, s, states, WTS[b], b)
            got[b] = TL.Taps(s, H, W, b, None).get("c41")
            ok, worst, ratio = LR.check2(got[b], *LR.cached_c41(p3[b], weights, sets[b]), LR.K["f23"], LR.K["point"])
            print("[ratio] %s c41 %dx%d image %d point %.3g (%.3g of the bound)" % (case, H, W, b, ratio, worst))
            assert ok, "c41 image %d: %.3g of the bound, ratio %.3g" % (b, worst, ratio)
            _note(case, "point", ratio)
        ok, worst, _ = LR.check2(got[2], *LR.cached_c41(p3[2], weights, sets[0]), LR.K["f23"], LR.K["point"])
        print("[control] %s image 2 c41 on set 0: %.3g of the bound" % (case, worst))
        assert not ok, "image 2's c41 passes on image 0's state set (%.3g of the bound)" % worst
    finally:
        s.close()
        donor.close()


# ---- c. filter_down unsplit and at split 4 with per-image folded weights -----------------------------------------------------------
# The smallest frames that leave split 8 (more than 40 relu4_1 tiles) and split 4 (more than 128), with a partial last tile:
# 64 x 5136 -> 8 x 642, 41 tiles; 64 x 16400 -> 8 x 2050, 129 tiles.
C_SHAPES = [(64, 5136, 4), (64, 16400, 1)]


@pytest.mark.parametrize("H,W,split", C_SHAPES, ids=["%dx%d" % s[:2] for s in C_SHAPES])
def test_filter_down_per_image_weights_frame_mode(pkg, weights, H, W, split):
    """Two frames through the batched frame-mode device entry: c41, d, f1, f2, f3 of image 1 over the whole tensors on image 1's
    set; its d on image 0's set fails."""
    case = "c/frame/split%d" % split
    frames = FL._mixed(pkg, 2, H, W)
    s, seq, smean = FL.launch(pkg, weights, frames)
    try:
        fam = LR.frame_families(seq)
        assert_split(pkg, s, seq, H, W, split)
        assert fam["d0"] == fam["d1"] == fam["d2"] == ("splitk" if split > 1 else "f23"), fam
        t = TL.Taps(s, H, W, 1, frames[1])
        st = {b: LR.parse_state(s.debug_state_set(0, b)) for b in (0, 1)}
        bad = []
        for name, f, ok, worst, ratio in LR.frame_checks(t.get, weights, st[1], smean, fam, names=FIVE):
            print("[ratio] %s image 1 %s %s %.3g (%.3g of the bound)" % (case, name, f, ratio, worst))
            _note(case, f, ratio)
            if not ok:
                bad.append((name, worst))
        assert not bad, bad
        res = {name: (ok, worst) for name, f, ok, worst, ratio in LR.frame_checks(t.get, weights, st[0], smean, fam, names=("d",))}
        print("[control] %s image 1 d on set 0: %.3g of the bound" % (case, res["d"][1]))
        assert not res["d"][0], "image 1's d passes on image 0's state set"
    finally:
        s.close()


@pytest.mark.parametrize("H,W,split", C_SHAPES, ids=["%dx%d" % s[:2] for s in C_SHAPES])
def test_filter_down_per_image_weights_blended(pkg, weights, states, H, W, split):
    """The same two shapes through the grouped blend of case a (two frames, the blended sets' folded weights)."""
    case = "c/blend/split%d" % split
    frames = _mixed(pkg, 100, 2, H, W)
    s, seq = blend_launch(pkg, weights, states, frames, WTS[:2])
    try:
        assert_split(pkg, s, seq, H, W, split)
        assert seq[8][0].startswith("conv_wino<") and "@256x512@" in seq[8][0], seq[8]
        st = {b: check_blended_set(case, s, states, WTS[b], b) for b in (0, 1)}
        fam, _ = checked(case, s, weights, st[1], seq, H, W, 1, frames[1], names=FIVE)
        assert fam["d"] == ("splitk" if split > 1 else "f23"), fam
        ok, worst = stage_passes(TL.Taps(s, H, W, 1, frames[1]), "d", weights, st[0], seq)
        print("[control] %s image 1 d on set 0: %.3g of the bound" % (case, worst))
        assert not ok, "image 1's d passes on image 0's state set (%.3g of the bound)" % worst
    finally:
        s.close()


# ---- d. the direct-form encoder ------------------------------------------------------------------------------------------------------

D_SHAPES = [(1, 33, 31), (1, 77, 90), (5, 40, 56)]
ENC = ("p1", "c21", "p2", "c31", "c32", "c33", "p3", "c41")


@pytest.mark.parametrize("shape", D_SHAPES, ids=["%dx%dx%d" % s for s in D_SHAPES])
def test_direct_form_encoder(pkg, weights, shape):
    """RRV_DIRECT_LAYERS=0x1fe at handle creation: conv1_2 .. conv4_1 on conv_mfma_k (nine multiplies per output, no transform), all
    four instantiations; every stage checked, the encoder's in the gemm family."""
    B, H, W = shape
    case = "d/%dx%dx%d" % shape
    blob = load_golden("global_a")["state"]
    st = LR.parse_state(blob)
    frames = TL.frames_for(pkg, B, H, W)
    with TL.env(RRV_DIRECT_LAYERS="0x1fe"):
        s, seq, _ = TL.launch(pkg, weights, frames, blob, int(os.environ.get("RRV_F43", "1")))
    try:
        names = [seq[i][0].split("@")[0] for i in range(1, 9)]
        assert names[0].startswith("conv_mfma<64,9,") and all(n.startswith("conv_mfma<128,9,") for n in names[1:]), names
        assert len(set(names)) == 4, names          # ReLU + pool at 64 couts; ReLU, ReLU + pool and ReLU + norm at 128 per workgroup
        for b in sorted({0, B - 1}):
            fam, lay = checked(case, s, weights, st, seq, H, W, b, frames[b])
            assert fam["c11"] == fam["pre"] == "direct" and all(fam[n] == "gemm" for n in ENC), fam
            assert not any(lay[n] for n in ("c11",) + ENC), lay          # the direct form reads and writes NHWC: no P8 twin
    finally:
        s.close()

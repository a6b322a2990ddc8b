"""Every kernel of the frame-mode path (Stylization(use_Global=False): frame_mode_device, one-frame and batched) against the
float64 stage references of tests/layer_ref.py (FRAME_STAGES): each image's statistics, predicted filters and identity
entry from its state set (rrv_debug_copy_state), each tap teacher-forced on the GPU's own input taps and statistics.  One
profiled launch per case on a fresh handle; the profile's kernel names must be the launch sequence the stage table describes
(LR.frame_families), and every tap read has its zero ring checked.  Nothing is skipped or masked: every element of every
checked tensor is inside its bound.  The grouped multi-style launches (per-image BLENDED state sets on the fused path) are
checked with test_gpu_layers.check_image on each image's own set."""
import importlib

import numpy as np
import pytest
import torch

import layer_ref as LR
import test_gpu_layers as TL
from test_gpu_frame_mode_batch import _mixed, STYLE

pytestmark = pytest.mark.gpu

RATIOS = {f: (0.0, "-") for f in LR.FAMILIES}      # the largest measured figure per family over the module, and where


def _note(f, ratio, where):
    if f is not None and ratio > RATIOS[f][0]:
        RATIOS[f] = (ratio, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[layer ratios] " + " ".join("%s=%.3g" % (f, RATIOS[f][0]) for f in LR.FAMILIES))
    print("[layer ratios at] " + " ".join("%s=%s" % (f, RATIOS[f][1]) for f in LR.FAMILIES))


def launch(pkg, weights, frames, host=False):
    """One profiled frame-mode call on a fresh handle: the device entry (one launch sequence, B <= 16), or the host batch entry
    (sequences of up to sixteen).  Returns (handle, [(kernel name, followed by sum_parts)] of the LAST sequence, style half of
    the filter predictions)."""
    B, H, W, _ = frames.shape
    s = pkg.Stylization(weights, cuda=True, use_Global=False)
    s.prepare_style(pkg.synth_style(**STYLE))
    smean = s.debug_style_pred(0).astype(np.float64)
    with pytest.raises(pkg.RRVError, match="no per-image state"):
        s.debug_state_set(0, 0)
    torch.cuda.synchronize()
    s.profile_begin()
    if host:
        s.transfer_batch(frames)
    else:
        d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        d_out = torch.empty((B, H // 8 * 8, W // 8 * 8, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.transfer_batch_device(d_in.data_ptr(), B, H, W, d_out.data_ptr())
    rows = [r[0] for r in s.profile_end()]
    s.sync()
    starts = [i for i, n in enumerate(rows) if n.startswith("frame_sets_init")]
    assert len(starts) == (B + 15) // 16, rows
    rows = rows[starts[-1]:]
    seq = []
    for i, n in enumerate(rows):
        if n.startswith("sum_parts"):
            continue
        seq.append((n, i + 1 < len(rows) and rows[i + 1].startswith("sum_parts")))
    return s, seq, smean


def run_checks(tag, t, weights, st, smean, fam, names=None):
    """LR.frame_checks on one image's taps: prints every figure, returns [(stage, fraction of its bound)] of the failures."""
    bad = []
    for name, f, ok, worst, ratio in LR.frame_checks(t.get, weights, st, smean, fam, names=names):
        print("[ratio] %s %s %s %.3g (%.3g of the bound)%s" % (tag, name, f, ratio, worst, "" if ok else " FAILS"))
        if ok:
            _note(f, ratio, "%s:%s" % (tag, name))
        else:
            bad.append((name, worst))
    return bad


def check_image(s, weights, smean, fam, H, W, b, frame):
    t = TL.Taps(s, H, W, b, frame)
    st = LR.parse_state(s.debug_state_set(0, b))
    bad = run_checks("%dx%d image %d" % (H, W, b), t, weights, st, smean, fam)
    assert not bad, "%dx%d image %d: %s" % (H, W, b, bad)
    assert not any(t.layout.values()), t.layout        # frame mode is F(2x2,3x3) on NHWC tensors throughout
    return t, st


def frames_for(pkg, B, H, W):
    return _mixed(pkg, B, H, W) if B > 1 else pkg.synth_frame(0, H, W, kind="smooth")[None]


# (B, H, W, images checked).  The KernelFilter down convolution runs split K = 8 in every case (filter_down splits by the
# relu4_1 tile count: 8 slices up to 40 tiles of 16 x 16), with the shared folded weights at B = 1 and per-image ones above.
CASES = [(1, 8, 8, (0,)),             # 1 x 1 relu4_1: every off-centre rectangle is empty, variance exactly 0, rstd = 1e4
         (1, 16, 8, (0,)),            # one-column feature
         (1, 8, 24, (0,)),            # one-row feature
         (1, 33, 31, (0,)),           # floors, partial tiles
         (1, 77, 90, (0,)),
         (3, 40, 56, (0, 2)),         # small batch
         (16, 136, 200, (0, 7, 15)),  # a full launch sequence
         (2, 640, 640, (0, 1)),       # 25 tiles per image, per-image folded weights under split K; both images, whole tensors
         (1, 1032, 8, (0,))]          # more rows than chan_stat1's 512 blocks


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d" % c[:3] for c in CASES])
def test_every_frame_mode_stage(pkg, weights, case):
    B, H, W, images = case
    frames = frames_for(pkg, B, H, W)
    s, seq, smean = launch(pkg, weights, frames)
    try:
        fam = LR.frame_families(seq)
        assert fam["c11"] == fam["pre"] == "direct" and fam["a4"] == fam["a3"] == fam["a2"] == "ups"
        assert all(fam[n] == "f23" for n in LR.FRAME_ENC[1:] + ("c41", "u0", "u1", "u2", "o4", "o3", "o2")), fam
        assert ((H // 8 + 15) // 16) * ((W // 8 + 15) // 16) <= 40 and fam["d0"] == fam["d1"] == fam["d2"] == "splitk", fam
        _, lay, ch = s.debug_tensor_ex(0, LR.TAP["dpart"], H, W, 0)
        assert lay == 0 and ch == 32 * 8
        if B < 16:
            with pytest.raises(pkg.RRVError, match="did not write this image"):
                s.debug_state_set(0, B)
        with pytest.raises(pkg.RRVError) as e:
            s.debug_state_set(0, 16)           # a slot has sixteen sets
        assert e.value.code == -1
        with pytest.raises(pkg.RRVError, match="no per-image state"):
            s.debug_state_set(1, 0)
        sets = {}
        for b in images:
            t, sets[b] = check_image(s, weights, smean, fam, H, W, b, frames[b])
            if H == W == 8:
                assert np.allclose(sets[b]["norm"][0][1], 1e4, rtol=1e-6, atol=0)      # one pixel: variance exactly 0, rstd = 1 / sqrt(1e-8)
        for b in images[1:]:        # the style statistics frame_sets_init_k copies are the style's, the same in every set
            for x, y in zip(sets[b]["sty"], sets[images[0]]["sty"]):
                np.testing.assert_array_equal(x[0], y[0])
                np.testing.assert_array_equal(x[1], y[1])
        if B == 16:
            # wrong neighbour on real data: image 7's taps evaluated with image 8's state set must fail (the bounds are not vacuous)
            t7 = TL.Taps(s, H, W, 7, frames[7])
            st8 = LR.parse_state(s.debug_state_set(0, 8))
            names = ("stat0", "c41", "pred0", "f1", "d", "f3", "stat:a4", "a4")
            failed = {n for n, _ in run_checks("%dx%d image 7 on set 8" % (H, W), t7, weights, st8, smean, fam, names=names)}
            assert failed >= {"stat0", "c41", "pred0.F1", "pred0.F2", "f1", "d", "f3", "stat:a4", "a4"}, failed
    finally:
        s.close()


def test_second_launch_sequence_of_the_host_entry(pkg, weights):
    """17 frames of 72 x 88 through the host batch entry: sixteen in the first launch sequence, one in the second; the taps and
    the state set are the last sequence's."""
    H, W = 72, 88
    frames = _mixed(pkg, 17, H, W)
    s, seq, smean = launch(pkg, weights, frames, host=True)
    try:
        fam = LR.frame_families(seq)
        check_image(s, weights, smean, fam, H, W, 0, frames[16])
        with pytest.raises(pkg.RRVError, match="did not write this image"):
            s.debug_state_set(0, 1)
        with pytest.raises(pkg.RRVError, match="did not write this image"):
            s.debug_tensor_ex(0, LR.TAP["c41"], H, W, 1)
    finally:
        s.close()


def test_grouped_multistyle_launch_state_sets_and_layers(pkg, weights, oracle):
    """rrv_transfer_features_batch with per-frame style weights, one group of seven frames: the fused path with one BLENDED state
    set per image.  Each checked image's set against the float64 sum of the styles' blobs (blend_sets_k), and the stages d ..
    pre against their float64 references on that set."""
    V = importlib.import_module("rerevst-code_amd.video")
    styles = [pkg.synth_style(64, 64, kind="smooth", seed=7 + k) for k in range(4)]
    frames = [oracle.reflect_pad(pkg.synth_frame(i, 64, 48, kind="smooth"), 192, 192) for i in range(7)]
    s = pkg.MultiStyleStylization(weights, cuda=True, style_num=4)
    try:
        s.prepare_style(styles)
        feats = [s.generate_content_features(p) for p in frames]
        s.clean()
        for i in (0, 2):
            s.add_patch(feats[i])
        s.compute_norm()
        blobs = [s.get_state(k) for k in range(4)]
        wts = [V.ramp_weights(i, 7, 4, blend="all") for i in range(7)]       # every style active in every frame
        s.set_multistyle_group(16)
        s.profile_begin()
        s.transfer_many(feats, wts)
        rows = [r[0] for r in s.profile_end()]
        s.sync()
        assert [n.split("@")[0] for n in rows[:7]] == ["pointwise"] * 7, rows      # Decoder.norm[0] of each cached feature with ITS set
        rows = rows[7:]
        seq = [("", False)] * 9         # the encoder's nine launches did not run: the stage table's positions start behind them
        for i, n in enumerate(rows):
            if not n.startswith("sum_parts"):
                seq.append((n, i + 1 < len(rows) and rows[i + 1].startswith("sum_parts")))
        assert len(seq) == LR.N_LAUNCHES, rows
        names = tuple(n for n in LR.STAGES if LR.STAGES[n][0] >= 13) + LR.FOLDED
        for b in (0, 6):
            blob = s.debug_state_set(0, b)
            ref, mag = LR.blend_ref(blobs, wts[b])
            err = np.abs(blob.astype(np.float64) - ref)
            ratio = float((err / np.maximum(LR.U * mag, 1e-300)).max())
            print("[ratio] multistyle image %d blend stat %.3g" % (b, ratio))
            assert np.all(err <= LR.K["stat"] * LR.U * mag), "image %d: blended set at ratio %.3g" % (b, ratio)
            _note("stat", ratio, "multistyle image %d:blend" % b)
            TL.check_image(s, weights, LR.parse_state(blob), seq, 192, 192, b, None, names=names)
        with pytest.raises(pkg.RRVError, match="did not write this image"):
            s.debug_state_set(0, 7)
        pkg.Stylization.transfer(s, frames[1])          # a plain transfer re-activates style 0 in set 0: no per-image state left
        with pytest.raises(pkg.RRVError, match="no per-image state"):
            s.debug_state_set(0, 0)
    finally:
        s.close()

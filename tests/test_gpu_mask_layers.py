"""Every kernel of the masked multi-style walk (mask_mode_device: mask_pyramid_k, mask_norm_k, mask_filter_k and the convolutions
between them) against the float64 stage references of tests/mask_layer_ref.py: the four level masks bit for bit against
mask_ref.level_masks of the mask the caller passed, every other tap teacher-forced on the GPU's own input taps and on the GPU's
own level-mask tap.  One profiled masked call per case on a fresh handle through the device entry; the profile's rows must be
the 37-launch sequence DESIGN §5 lists (MR.mask_families), every tap NHWC with its zero ring checked.  Nothing is skipped or
masked: every element of every checked tensor is inside its bound."""
import importlib

import numpy as np
import pytest
import torch

import layer_ref as LR
import mask_layer_ref as MR
import mask_ref
import test_gpu_layers as TL
from test_gpu_mask_blend import _golden_setup, _mixed

pytestmark = pytest.mark.gpu

V = importlib.import_module("rerevst-code_amd.video")
RATIOS = {f: (0.0, "-") for f in LR.FAMILIES}      # the largest measured figure per family over the module, and where


def _note(f, ratio, where):
    if f is not None and ratio > RATIOS[f][0]:
        RATIOS[f] = (ratio, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[layer ratios] " + " ".join("%s=%.3g" % (f, RATIOS[f][0]) for f in LR.FAMILIES))
    print("[layer ratios at] " + " ".join("%s=%s" % (f, RATIOS[f][1]) for f in LR.FAMILIES))


@pytest.fixture(scope="module")
def base(pkg, oracle, weights):
    """Four computed states that differ pairwise in Decoder.norm[0] (mask_ref.distinct_states: with masks that sum to one
    mask_norm_k at c41 would otherwise compute the same value under any mask and any style order)."""
    return mask_ref.distinct_states(*_golden_setup(pkg, oracle, weights, "multistyle_s4")[:2])


def launch(pkg, weights, base, frames, M, S, pad_crop=False, host=False):
    """One profiled masked call on a fresh handle with S distinct states: the device entry (transfer_tensor, slot 0), or the host
    batch entry.  Returns (handle, the S state blobs, the profile rows of the LAST launch sequence)."""
    blobs = MR.mask_states(base, S)
    s = pkg.MultiStyleStylization(weights, cuda=True, style_num=S)
    for k, b in enumerate(blobs):
        s.set_state(b, k)
    with pytest.raises(pkg.RRVError, match="no such tensor"):
        s.debug_tensor_ex(0, LR.TAP["lm0"], frames.shape[1], frames.shape[2], 0)
    x = None if host else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    s.profile_begin()
    if host:
        s.transfer_batch(frames, style_masks=M)
    else:
        s.transfer_tensor(x, layout="nhwc", style_masks=M, pad_crop=pad_crop)
    rows = [r[0] for r in s.profile_end()]
    s.sync()
    starts = [i for i, n in enumerate(rows) if n.startswith("mask_pyramid")]
    assert len(starts) == (frames.shape[0] + 15) // 16, rows
    rows = rows[starts[-1]:]
    assert not any(n.startswith(("sum_parts", "conv_f43")) for n in rows), rows
    return s, blobs, rows


class MaskTaps(TL.Taps):
    """TL.Taps with the level masks (decoded to [S][h][w], taken from image `lm_image`: 0 for a launch with one mask) and the
    split-K slices."""

    def __init__(self, s, H, W, b, frame, S, lm_image=None):
        super().__init__(s, H, W, b, frame)
        self.S, self.lm_image = S, b if lm_image is None else lm_image

    def get(self, name):
        if name in self.cache or not (name.startswith("lm") or name == "dpart"):
            return super().get(name)
        if name == "dpart":
            flat, lay, ch = self.s.debug_tensor_ex(0, LR.TAP[name], self.H, self.W, self.b)
            v = LR.ring_to_hwc(flat, self.H // 8, self.W // 8, ch)
        else:
            l = int(name[2:])
            flat, lay, ch = self.s.debug_tensor_ex(0, LR.TAP[name], self.H, self.W, self.lm_image)
            assert ch == MR.MASK_CH, ch
            v = MR.decode_level_mask(flat, (self.H // 8 * 8) >> l, (self.W // 8 * 8) >> l, self.S)
        self.cache[name], self.layout[name] = v, lay
        return v


def split_of(pkg, s, H, W):
    """the slices of the KernelFilter down convolution, read from the dpart tap's channel count (refused at split 1)"""
    try:
        _, lay, ch = s.debug_tensor_ex(0, LR.TAP["dpart"], H, W, 0)
    except pkg.RRVError as e:
        assert "did not write" in str(e) or "no such tensor" in str(e), e
        return 1
    assert lay == 0 and ch % 32 == 0 and ch > 32, ch
    return ch // 32


def run_checks(tag, t, weights, sts, fam, split, lv=None, names=None, levels=(0, 1, 2, 3)):
    """The level masks against lv (when given) and MR.mask_checks on one image's taps: prints every figure, returns the failures."""
    out = [] if lv is None else MR.check_level_masks(t.get, lv, t.S, levels=levels)
    out += MR.mask_checks(t.get, weights, sts, fam, split, names=names)
    bad = []
    for name, f, ok, worst, ratio in out:
        print("[ratio] %s %s %s %.3g (%.3g of the bound)%s" % (tag, name, f, ratio, worst, "" if ok else " FAILS"))
        if ok:
            _note(f, ratio, "%s:%s" % (tag, name))
        else:
            bad.append((name, worst))
    return bad


def masks_for(kind, seed, B, S, H, W):
    if kind == "edge":
        return MR.odd_edge_mask(S, H, W, row=27, col=13)
    if kind == "one":
        return MR.softmax_mask(seed, S, H, W)
    return MR.softmax_mask(seed, S, H, W, B=B)


# (B, H, W, S, mask kind, images checked, split expected, stages): the smallest shapes that reach each path
ALL = None
CASES = [(1, 8, 8, 1, "soft", (0,), 8, ALL),             # one relu4_1 pixel; segs capped at 1; pyramid<1>
         (1, 33, 31, 3, "soft", (0,), 8, ALL),           # floors; odd S; partial 16-pixel segments
         (1, 77, 90, 2, "edge", (0,), 8, ALL),           # a hard mask with its edges at an odd row and column
         (3, 40, 56, 5, "soft", (0, 2), 8, ALL),         # a mask per image; relu4_1 of 35 pixels: mask_filter_k blocks straddle images
         (2, 72, 104, 7, "one", (0, 1), 8, ALL),         # ONE mask for both images (bstride 0)
         (1, 8, 264, 6, "soft", (0,), 8, ALL),           # one-row features
         (1, 1032, 8, 8, "soft", (0,), 8, ALL),          # one-column features; the maximum LDS of mask_filter_k
         (16, 136, 200, 4, "soft", (0, 7, 15), 8, ALL),  # a full launch sequence
         (1, 1152, 1152, 2, "soft", (0,), 4, MR.EIGHTH),  # the split-4 sum
         (1, 1536, 2048, 2, "soft", (0,), 1, MR.EIGHTH)]  # split 1: mask_filter_k in place on d


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d-S%d" % c[:4] for c in CASES])
def test_every_masked_stage(pkg, weights, base, case):
    B, H, W, S, kind, images, split, names = case
    frames = _mixed(pkg, 40, B, H, W) if B > 1 else pkg.synth_frame(0, H, W, kind="smooth")[None]
    M = masks_for(kind, 1000 + H, B, S, H, W)
    s, blobs, rows = launch(pkg, weights, base, frames, M, S)
    try:
        fam = MR.mask_families(rows)
        assert fam["c11"] == fam["pre"] == "direct"
        assert all(fam[n] == "f23" for n in LR.FRAME_ENC[1:] + ("c41", "d0", "u0", "d1", "u1", "d2", "u2", "o4", "o3", "o2")), fam
        assert split_of(pkg, s, H, W) == split
        sts = [LR.parse_state(b) for b in blobs]
        one = kind in ("edge", "one")
        if one:
            with pytest.raises(pkg.RRVError, match="did not write this image"):
                s.debug_tensor_ex(0, LR.TAP["lm3"], H, W, 1)
        elif B < 16:
            with pytest.raises(pkg.RRVError, match="did not write this image"):
                s.debug_tensor_ex(0, LR.TAP["lm0"], H, W, B)
        for b in images:
            t = MaskTaps(s, H, W, b, frames[b], S, lm_image=0 if one else b)
            lv = mask_ref.level_masks(M if one else M[b])
            tag = "%dx%d S%d image %d" % (H, W, S, b)
            bad = run_checks(tag, t, weights, sts, fam, split, lv=lv, names=names, levels=(3,) if names else (0, 1, 2, 3))
            assert not bad, "%s: %s" % (tag, bad)
            assert not any(t.layout.values()), t.layout
        if B == 16:
            # not vacuous on real data: image 7's taps with image 8's level masks, and with the states in reversed order
            five = ("c41", "d", "f3", "a4", "o4")
            t7 = MaskTaps(s, H, W, 7, frames[7], S, lm_image=8)
            failed = {n for n, _ in run_checks("%dx%d image 7 on the masks of image 8" % (H, W), t7, weights, sts, fam, split, names=five)}
            assert failed == set(five), failed
            t7 = MaskTaps(s, H, W, 7, frames[7], S)
            failed = {n for n, _ in run_checks("%dx%d image 7 on reversed states" % (H, W), t7, weights, sts[::-1], fam, split, names=five)}
            assert failed == set(five), failed
    finally:
        s.close()


@pytest.mark.parametrize("H,W", [(36, 45), (100, 141)])
def test_level_masks_of_the_pad_crop_geometry(pkg, weights, base, H, W):
    """transfer_frames' geometry: the pyramid reads the caller's unpadded mask through the frame's reflect pad."""
    S, B = 3, 2
    PH, PW = V.padded_size(H), V.padded_size(W)
    frames = _mixed(pkg, 50, B, H, W)
    M = MR.softmax_mask(2000 + H, S, H, W, B=B)
    s, _, rows = launch(pkg, weights, base, frames, M, S, pad_crop=True)
    try:
        MR.mask_families(rows)
        for b in range(B):
            t = MaskTaps(s, PH, PW, b, None, S)
            bad = run_checks("pad/crop %dx%d image %d" % (H, W, b), t, weights, None, None, 0, lv=mask_ref.level_masks(mask_ref.pad_mask(M[b], PH, PW)), names=())
            assert not bad, bad
    finally:
        s.close()


def test_second_launch_sequence_of_the_host_entry(pkg, weights, base):
    """17 frames of 72 x 88 through transfer_batch(style_masks=): sixteen in the first launch sequence, one in the second; the
    taps are the last sequence's."""
    H, W, S = 72, 88, 4
    frames = _mixed(pkg, 60, 17, H, W)
    M = MR.softmax_mask(3000, S, H, W, B=17)
    s, blobs, rows = launch(pkg, weights, base, frames, M, S, host=True)
    try:
        fam = MR.mask_families(rows)
        split = split_of(pkg, s, H, W)
        assert split == 8
        t = MaskTaps(s, H, W, 0, frames[16], S)
        bad = run_checks("host entry image 16", t, weights, [LR.parse_state(b) for b in blobs], fam, split, lv=mask_ref.level_masks(M[16]))
        assert not bad, bad
        for name in ("lm0", "lm3", "c41"):
            with pytest.raises(pkg.RRVError, match="did not write this image"):
                s.debug_tensor_ex(0, LR.TAP[name], H, W, 1)
    finally:
        s.close()


def test_level_mask_taps_are_refused_after_an_unmasked_launch(pkg, weights, base):
    """The level masks of a plan are those of its last masked launch: a plain launch on the same plan makes them stale."""
    H, W, S = 40, 56, 2
    frames = _mixed(pkg, 70, 2, H, W)
    s, _, _ = launch(pkg, weights, base, frames, MR.softmax_mask(4000, S, H, W, B=2), S)
    try:
        s.debug_tensor_ex(0, LR.TAP["lm2"], H, W, 1)
        s.set_pipeline(1)                   # the next call reuses slot 0's plan
        s.transfer_tensor(torch.from_numpy(frames).cuda(), layout="nhwc")
        s.sync()
        with pytest.raises(pkg.RRVError, match="did not write this tensor"):
            s.debug_tensor_ex(0, LR.TAP["lm2"], H, W, 0)
        with pytest.raises(pkg.RRVError):
            s.debug_tensor_ex(0, LR.TAP["lm3"] + 1, H, W, 0)
    finally:
        s.close()

"""The windowed launches of the pad / crop entries (rrv_transfer_frames*, RRV_TF_PAD_CROP) against their layer references, on a workspace
that holds another picture.  With a crop the full-resolution block computes windows only (transfer_device: wl, wo, wa; conv_params rounds
the shortcut-fused conv1 out to its 32 x 32 items), restated in LR.crop_windows and proven sufficient on the CPU (tests/test_layer_ref.py).
Each case is one handle on one stream and one workspace slot:
  1  a plain launch of B white-noise frames of the padded size fills every tensor of slot 0's plan; a2 (or its P8 twin), xs2, o2 and the
     pre-clamp tap are read back as stored
  2  the pad / crop device entry runs on B smooth source frames, profiled; the same taps are read back
  3  outside the windows of LR.crop_windows every element of every tap still holds the bits of 1: nothing outside a window is written,
     the launch really was windowed, and the library's windows are no larger than the restatement
  4  inside a window every element is finite and differs from 1's, unless the stale value itself is within the stage's bound of the
     reference (a clamp end both pictures sit on): the library's windows are no smaller than the restatement
  5  xs2 and a2 (from the whole o3 tap), o2 (from a2 and xs2) and pre (from o2) against the float64 stages of LR.STAGES on their windows,
     within the K of the family the profile row names; before each, every element the reference reads is asserted to lie in its producer's
     window or outside the frame (LR.window_faults and the conditions spelt out here), which a reference fed the GPU's own input cannot see
  6  the delivered crop equals, bit for bit, the crop of a fresh handle that made only the windowed call (zeros outside the windows) and
     the crop of a full compute of the reflect-padded frames in the same kernel choice on a third handle: a launch that read outside its
     producer's window would have seen noise in one run and zeros in the other.
The pre-clamp tap has a reference on LR.pre_checkable(w) only: with (64 + n) = 15 (mod 16) the last row of wl lies behind the crop and its
taps reach one row past wo (nothing delivers that row)."""
import importlib

import numpy as np
import pytest
import torch

import layer_ref as LR
import mask_ref
import test_gpu_layers as TL
import yuv_ref as Y
from state_bounds import load_golden
from test_gpu_instantiations import seq_of, check_blended_set, WTS
from test_gpu_mask_blend import _golden_setup

pytestmark = pytest.mark.gpu

D = importlib.import_module("rerevst-code_amd.driver")

# crop ends 64 + n of residue 0, 1, 15, 16, 17 and 31 (mod 32) on each axis; every one pads to 192 x 192
SHAPES = [(32, 63), (33, 48), (47, 49), (48, 33), (49, 32), (63, 47)]
B = 2
P = 192
TAPS = ("xs2", "a2", "o2", "pre")
WIN_OF = {"xs2": "xs", "a2": "wa", "o2": "wo", "pre": "wl"}
RATIOS = {}          # family -> the largest ratio of a windowed launch


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[window ratios] " + " ".join("%s=%.3g" % kv for kv in sorted(RATIOS.items())))


def test_the_shapes_reach_every_residue():
    for axis in (0, 1):
        assert sorted((LR.CROP0 + s[axis]) % 32 for s in SHAPES) == [0, 1, 15, 16, 17, 31]
    assert {LR.padded_size(n) for s in SHAPES for n in s} == {P}


def noise_frames(pkg, n, seed=500):
    return np.stack([pkg.synth_frame(seed + i, P, P, kind="noise") for i in range(n)])


def make(pkg, weights, mode, p8, blob=None, cus=None):
    """A handle of one kernel choice on one stream and one workspace slot."""
    kv = {"RRV_P8": p8, "RRV_F43_LAYERS": hex(0x3ff)}
    if cus:
        kv["RRV_CUS"] = cus
    with TL.env(**kv):
        s = pkg.Stylization(weights, cuda=True)
    s.set_f43(mode)
    s.set_pipeline(1)
    s.set_state(load_golden("global_a")["state"] if blob is None else blob)
    return s


def plain_call(s, frames):
    """rrv_transfer_batch_device on frames of the padded size; the float32 frames on the host."""
    n, H, W, _ = frames.shape
    d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    d_out = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s.transfer_batch_device(d_in.data_ptr(), n, H, W, d_out.data_ptr())
    s.sync()
    return d_out.cpu().numpy()


def windowed_call(s, frames, dtype=np.float32, profile=True):
    """The pad / crop device entry on unpadded frames: (crop on the host, launch sequence of the profile or None)."""
    n, H, W, _ = frames.shape
    d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    d_out = torch.full((n, H, W, 3), 77, dtype=torch.float32 if dtype == np.float32 else torch.uint8, device="cuda")
    torch.cuda.synchronize()
    seq = None
    if profile:
        s.profile_begin()
    s.transfer_frames_device(d_in.data_ptr(), n, H, W, d_out.data_ptr(), dtype=dtype)
    if profile:
        seq = seq_of([r[0] for r in s.profile_end()])
    s.sync()
    return d_out.cpu().numpy(), seq


def raw_taps(s, b):
    """The four taps of image b of slot 0's last launch AS STORED: {name: (flat float32, layout 0 ring / 1 P8 / None plain, channels)}."""
    out = {}
    for name in ("xs2", "o2"):
        out[name] = s.debug_tensor_ex(0, LR.TAP[name], P, P, b)
    got = []
    for n in ("a2", "qa2"):
        try:
            got.append(s.debug_tensor_ex(0, LR.TAP[n], P, P, b))
        except Exception as e:          # refused: this launch wrote the other layout
            assert "did not write" in str(e) or "no such tensor" in str(e), e
    assert len(got) == 1, "a2: %d layouts written" % len(got)
    out["a2"] = got[0]
    out["pre"] = (np.array(s.preclamp(P, P, image=b), np.float32).reshape(-1), None, 3)
    return out


def geo(name):
    return (P // 2, P // 2) if name == "xs2" else (P, P)


def hwc(name, tap):
    flat, lay, ch = tap
    h, w = geo(name)
    return flat.reshape(h, w, ch) if lay is None else LR.to_hwc(flat, lay, h, w, ch)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bbox(mask2d):
    ys, xs = np.nonzero(mask2d)
    return (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1) if ys.size else (0, 0, 0, 0)


def families(seq, conv2):
    """The kernel families of the launch sequence, asserted as TL.assert_kind does for the stages a window touches and the ones before them."""
    fam = {name: LR.family_of(*seq[li]) for name, (li, _, _, _) in LR.STAGES.items()}
    assert fam["c11"] == fam["pre"] == "direct"
    assert fam["xs4"] == fam["a4"] == fam["a3"] == fam["a2"] == fam["xs2"] == "ups"
    assert fam["d"] in ("splitk", "f23") and fam["f3"] == fam["c41"] == "f23"
    assert all(fam[n] == conv2 for n in TL.DEC_F43), fam
    return fam


def check_windows(case, s, weights, st, seq, w, b, stale, new, fam, k=None):
    """Steps 3, 4 and 5 for image b: `stale` and `new` are raw_taps() before and after the windowed call.  Returns {tap: passes its bound}
    when k (a K table to judge by) is given, else asserts."""
    assert LR.window_faults(w) == [], w
    k_tab = LR.K if k is None else k
    new_hwc = {n: hwc(n, new[n]) for n in TAPS}
    o3 = TL.Taps(s, P, P, b, None).get("o3")
    inputs = {"xs2": [o3], "a2": [o3], "o2": [new_hwc["a2"], new_hwc["xs2"]], "pre": [new_hwc["o2"]]}
    verdict = {}
    for name in TAPS:
        flat, lay, ch = new[name]
        h, wd = geo(name)
        win = LR.clip(w[WIN_OF[name]], h, wd)
        y0, x0, y1, x1 = win
        assert stale[name][1:] == (lay, ch), (name, stale[name][1:], lay, ch)
        # 3: nothing outside the window is written, in the tap's own layout (the P8 twin keeps pixel x at column x + 4)
        m = LR.window_mask(win, h, wd, lay, ch)
        nb, sb = bits(flat), bits(stale[name][0])
        assert m.size == nb.size and np.array_equal(nb[~m], sb[~m]), "%s %s image %d: %d elements outside %s were written" % (
            case, name, b, int((nb[~m] != sb[~m]).sum()), win)
        changed = (bits(new_hwc[name]) != bits(hwc(name, stale[name]))).any(axis=2)
        print("[window] %s image %d %s: written %s, stated %s" % (case, b, name, bbox(changed), win))
        # 5: the reference on the window; every element it reads is inside its producer's window or outside the frame
        ev = win
        if name == "o2":
            assert LR.inside(LR.reads3(win, P, P), w["wa"]) and LR.inside(LR.reads_half(win, P, P), w["xs"]), w
        if name == "pre":
            ev = LR.pre_checkable(w)
            assert LR.inside(LR.reads3(ev, P, P), w["wo"]) and LR.inside(w["crop"], ev) and LR.inside(ev, win), w
        v, mag = LR.window_stage(name, inputs[name], weights, st, ev)
        got = new_hwc[name][ev[0]:ev[2], ev[1]:ev[3]]
        f = fam[name]
        ok, worst, ratio = LR.check(got, v, mag, k_tab[f])
        print("[ratio] %s %s image %d window %s %s %.3g" % (case, name, b, ev, f, ratio))
        verdict[name] = ok
        if k is not None:
            continue
        RATIOS[f] = max(RATIOS.get(f, 0.0), ratio)
        assert ok, "%s %s image %d window %s (%s): %.3g of the bound, ratio %.3g" % (case, name, b, ev, f, worst, ratio)
        # 4: every element of the window is written: finite, and other than the stale one unless that one is the reference's value too
        inside_new = new_hwc[name][y0:y1, x0:x1]
        assert np.isfinite(inside_new).all(), (case, name, b)
        same = bits(inside_new) == bits(hwc(name, stale[name])[y0:y1, x0:x1])
        excused = np.zeros_like(same)
        old = hwc(name, stale[name])[ev[0]:ev[2], ev[1]:ev[3]].astype(np.float64)
        excused[ev[0] - y0:ev[2] - y0, ev[1] - x0:ev[3] - x0] = np.abs(old - v) <= k_tab[f] * LR.U * mag + LR.U * np.abs(v)
        left = same & ~excused
        assert not left.any(), "%s %s image %d: %d elements of %s kept the stale value (%d more are the reference's value)" % (
            case, name, b, int(left.sum()), win, int((same & excused).sum()))
        assert bbox(changed) == win, (case, name, b, bbox(changed), win)
    return verdict


@pytest.mark.parametrize("kind", ["f23", "f43_p8", "f43_nhwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_windowed_launch_on_a_stale_workspace(pkg, weights, oracle, kind, shape):
    H, W = shape
    case = "%s/%dx%d" % (kind, H, W)
    mode, p8 = TL.KINDS[kind]
    conv2 = "f23" if kind == "f23" else "f43"
    w = LR.crop_windows(H, W, conv2 == "f43")
    assert (w["PH"], w["PW"]) == (P, P)
    st = LR.parse_state(load_golden("global_a")["state"])
    frames = TL.frames_for(pkg, B, H, W, seed=40)
    s = make(pkg, weights, mode, p8)
    fresh = make(pkg, weights, mode, p8)
    full = make(pkg, weights, mode, p8)
    try:
        plain_call(s, noise_frames(pkg, B))
        stale = [raw_taps(s, b) for b in range(B)]
        crop, seq = windowed_call(s, frames)
        new = [raw_taps(s, b) for b in range(B)]
        fam = families(seq, conv2)
        assert new[0]["a2"][1] == (1 if kind == "f43_p8" else 0), new[0]["a2"][1]
        for b in sorted({0, B - 1}):
            check_windows(case, s, weights, st, seq, w, b, stale[b], new[b], fam)
        # 6: nothing outside a window is read
        crop_fresh, _ = windowed_call(fresh, frames, profile=False)
        np.testing.assert_array_equal(crop, crop_fresh)
        padded = np.stack([oracle.reflect_pad(f, P, P) for f in frames])
        whole = plain_call(full, padded)
        np.testing.assert_array_equal(crop, whole[:, LR.CROP0:LR.CROP0 + H, LR.CROP0:LR.CROP0 + W])
    finally:
        for h in (s, fresh, full):
            h.close()


# ---- further cases, at 47 x 49: crop ends 111 = 15 (mod 16), the tight end, and 113 = 17 (mod 32) -------------------------------------------
FH, FW = 47, 49


@pytest.fixture(scope="module")
def states(pkg, oracle, weights):
    """Three computed states, every pair different in Decoder.norm[0] (mask_ref.distinct_states asserts it)."""
    return mask_ref.distinct_states(*_golden_setup(pkg, oracle, weights, "multistyle_s4")[:2])[:3]


def _multi(pkg, weights, blobs):
    with TL.env(RRV_P8=3, RRV_F43_LAYERS=hex(0x3ff)):
        s = pkg.MultiStyleStylization(weights, cuda=True, style_num=len(blobs))
    for k, blob in enumerate(blobs):
        s.set_state(blob, k)
    s.set_f43(0)
    s.set_pipeline(1)
    return s


def _blend(s, frames, pad_crop, profile=False):
    """transfer_tensor(style_weights=WTS) on uint8 NHWC frames: (float32 frames on the host, launch sequence or None)."""
    x = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    seq = None
    if profile:
        s.profile_begin()
    out = s.transfer_tensor(x, layout="nhwc", pad_crop=pad_crop, style_weights=WTS, out_dtype=torch.float32)
    if profile:
        seq = seq_of([r[0] for r in s.profile_end()])
    s.sync()
    torch.cuda.synchronize()
    return out.cpu().numpy(), seq


def test_windowed_launch_with_per_image_state(pkg, weights, oracle, states):
    """A blended pad / crop call of three frames on states that differ: conv_wino_k<6,0,4,1,1,1> and conv_wino_split_k<54,1> windowed.  Steps 3
    to 6 with every image on its own blended set; an image judged on its neighbour's set fails a2 and o2."""
    n = len(WTS)
    case = "blend/%dx%d" % (FH, FW)
    w = LR.crop_windows(FH, FW, False)
    frames = TL.frames_for(pkg, n, FH, FW, seed=60)
    s, fresh, full = (_multi(pkg, weights, states) for _ in range(3))
    try:
        plain_call(s, noise_frames(pkg, n))
        stale = [raw_taps(s, b) for b in range(n)]
        crop, seq = _blend(s, frames, True, profile=True)
        new = [raw_taps(s, b) for b in range(n)]
        fam = families(seq, "f23")
        for i in (19, 20):          # the windowed rows are the per-image instantiations' (conv() takes the IMG row under per-image state)
            assert seq[i][0].startswith(("conv_upw", "conv_wino")), seq[i]
        s.debug_state_set(0, n - 1)
        sets = [check_blended_set(case, s, states, WTS[b], b) for b in range(n)]
        for b in range(n):
            check_windows(case, s, weights, sets[b], seq, w, b, stale[b], new[b], fam)
        verdict = check_windows(case + "/control", s, weights, sets[0], seq, w, 1, stale[1], new[1], fam, k=LR.K)
        assert not verdict["a2"] and not verdict["o2"], "image 1 passes on image 0's state set: %s" % verdict
        crop_fresh, _ = _blend(fresh, frames, True)
        np.testing.assert_array_equal(crop, crop_fresh)
        whole, _ = _blend(full, np.stack([oracle.reflect_pad(f, P, P) for f in frames]), False)
        np.testing.assert_array_equal(crop, whole[:, LR.CROP0:LR.CROP0 + FH, LR.CROP0:LR.CROP0 + FW])
    finally:
        for h in (s, fresh, full):
            h.close()


def test_windowed_item_walk_on_a_small_grid(pkg, weights):
    """RRV_CUS=5: fewer persistent workgroups than work items in each of the three windowed launches (the fused conv1, conv2, conv_last), so
    every workgroup walks several items of the window: the taps as stored and the crop hold the bits of the default grid, in both conv2 forms."""
    frames = TL.frames_for(pkg, B, FH, FW, seed=70)
    for kind in ("f23", "f43_p8"):
        mode, p8 = TL.KINDS[kind]
        w = LR.crop_windows(FH, FW, kind != "f23")
        tiles = lambda win, t: ((win[2] - win[0]) // t) * ((win[3] - win[1]) // t)
        # work items: 32 x 32 pixels x 2 slabs of 32 couts (conv1, and conv2 on conv_f43_k), 16 x 16 x 2 slabs (conv2 on F(2x2,3x3)), 16 x 16 (conv_last)
        items = [tiles(w["wa"], 32) * B * 2, tiles(w["wo"], 16 if kind == "f23" else 32) * B * 2, tiles(w["wl"], 16) * B]
        got = []
        for cus in (None, 5):
            s = make(pkg, weights, mode, p8, cus=cus)
            try:
                crop, seq = windowed_call(s, frames)
                grids = [g for g, _ in s.profile_grids()][-3:]
                got.append((crop, [raw_taps(s, b) for b in range(B)], grids))
            finally:
                s.close()
        (crop_a, taps_a, grids_a), (crop_b, taps_b, grids_b) = got
        print("[grid] %s items %s, grids %s at the default, %s at RRV_CUS=5" % (kind, items, grids_a, grids_b))
        assert all(0 < g < n for g, n in zip(grids_b, items)) and all(a > b for a, b in zip(grids_a, grids_b)), (items, grids_a, grids_b)
        np.testing.assert_array_equal(crop_a, crop_b)
        for b in range(B):
            for name in TAPS:
                assert taps_a[b][name][1:] == taps_b[b][name][1:]
                assert np.array_equal(bits(taps_a[b][name][0]), bits(taps_b[b][name][0])), (kind, b, name)


def test_windowed_launch_in_the_quantising_output_forms(pkg, weights):
    """uint8 and NV12 output of the windowed call (conv_last_k's window and crop in the quantising instantiations) equal D.to_uint8 / yuv_ref
    of its float32 crop."""
    frames = TL.frames_for(pkg, B, FH, FW, seed=80)
    s = make(pkg, weights, 2, 3)
    try:
        f, _ = windowed_call(s, frames)
        u8, _ = windowed_call(s, frames, dtype=np.uint8, profile=False)
        np.testing.assert_array_equal(u8, D.to_uint8(f))
        x = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        nv12 = s.transfer_tensor(x, layout="nhwc", out_layout="nv12", pad_crop=True)
        torch.cuda.synchronize()
        m = Y.matrix64("bt601", False).astype(np.float32)
        assert tuple(nv12.shape) == (B, Y.frame_bytes(FH, FW))
        np.testing.assert_array_equal(nv12.cpu().numpy(), Y.yuv_ref(f, m, "nv12"))
    finally:
        s.close()


def test_host_entry_delivers_the_windowed_last_kernel_in_pieces(pkg, weights):
    """transfer_frames on 56 frames of 47 x 49 equals the device entry's crop of the same frames bit for bit (kernel mode 2).  The host
    pipeline cuts sub-batches of 32 frames at 192 x 192 and drains the call's last one, here 24 frames, in pieces of 2 x 640 x 640 pixels =
    22 frames: run_last gets a FrameRange (22, then 2) together with the window."""
    n = 56
    frames = np.stack([pkg.synth_frame(900 + i, FH, FW, kind="noise" if i % 2 else "smooth") for i in range(n)])
    s = make(pkg, weights, 2, 3)
    try:
        ref, _ = windowed_call(s, frames, profile=False)
        s.set_pipeline(2)
        out = np.full((n, FH, FW, 3), -7.0, np.float32)
        assert s.transfer_frames(frames, out=out) is out
        assert (out >= 0).all(), "a sentinel value is left in the output"
        np.testing.assert_array_equal(out, ref)
    finally:
        s.close()

"""Every layer of the per-frame path against a float64 reference of its own GPU input (tests/layer_ref.py): each activation
tap is compared with the stage evaluated from the GPU's input tap(s), element-wise within K_family 2^-24 m + 2^-24 |ref|.
Each case creates its handle fresh, asserts from the profile's kernel names and the taps' layouts that the kernel family
and layout it claims to cover ran, and checks the zero ring / P8 padding of every tap it reads."""
import contextlib
import os

import numpy as np
import pytest
import torch

import layer_ref as LR
from state_bounds import load_golden

pytestmark = pytest.mark.gpu

RATIOS = {f: 0.0 for f in LR.FAMILIES}      # the largest measured ratio per family over the module (printed at the end)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[layer ratios] " + " ".join("%s=%.3g" % (f, RATIOS[f]) for f in LR.FAMILIES))


def launch(pkg, weights, frames, blob, mode, p8=3, layers=0x3ff):
    """One profiled launch of B frames ([B][H][W][3] uint8) through rrv_transfer_batch_device on a fresh handle; returns
    (handle, [(kernel name, followed by sum_parts)] without sum_parts, output on the device)."""
    B, H, W, _ = frames.shape
    with env(RRV_P8=p8, RRV_F43_LAYERS=hex(layers)):
        s = pkg.Stylization(weights, cuda=True)
    s.set_f43(mode)
    s.set_state(blob)
    d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    d_out = torch.empty((B, H // 8 * 8, W // 8 * 8, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s.profile_begin()
    s.transfer_batch_device(d_in.data_ptr(), B, H, W, d_out.data_ptr())
    rows = [r[0] for r in s.profile_end()]
    s.sync()
    seq = []
    for i, n in enumerate(rows):
        if n.startswith("sum_parts"):
            continue
        seq.append((n, i + 1 < len(rows) and rows[i + 1].startswith("sum_parts")))
    assert len(seq) == LR.N_LAUNCHES, rows
    return s, seq, d_out


class Taps:
    """The taps of one image of the last launch, each read once, in [H][W][C] (padding checked on the way)."""

    def __init__(self, s, H, W, b, frame):
        self.s, self.H, self.W, self.b, self.frame = s, H, W, b, frame
        self.cache, self.layout = {}, {}

    def get(self, name):
        if name in self.cache:
            return self.cache[name]
        if name == "frame":
            v = LR.grey_input(self.frame)
        elif name == "pre":
            v = self.s.preclamp(self.H // 8 * 8, self.W // 8 * 8, image=self.b)
        else:
            h, w, c = (LR.STAGES[name][3] if name in LR.STAGES else {"f1": LR.STAGES["f3"][3], "f2": LR.STAGES["f3"][3]}[name])(self.H, self.W)
            got = []
            for n in (name, LR.TWIN.get(name)):
                if n is None:
                    continue
                try:
                    got.append(self.s.debug_tensor_ex(0, LR.TAP[n], self.H, self.W, self.b))
                except Exception as e:          # refused: not written by this launch (the other layout)
                    assert "did not write" in str(e) or "no such tensor" in str(e), e
            assert len(got) == 1, "%s: %d layouts written" % (name, len(got))
            flat, lay, ch = got[0]
            assert ch == c, (name, ch, c)
            v = LR.to_hwc(flat, lay, h, w, c)
            self.layout[name] = lay
        self.cache[name] = v
        return v


def check_image(s, weights, st, seq, H, W, b, frame, names=None, taps=None):
    """Every stage (or `names`) of image b: returns {stage: family}; asserts each bound.  taps: the image's Taps, to share what is read."""
    t = Taps(s, H, W, b, frame) if taps is None else taps
    fam = {}
    for name, (li, inputs, op, geo) in LR.STAGES.items():
        if names and name not in names:
            continue
        f = LR.family_of(*seq[li])
        fam[name] = f
        got, inp = t.get(name), [t.get(i) for i in inputs]
        for y0, y1 in LR.strips(got.shape[0]):
            v, m = op(inp, weights, st, y0, y1)
            ok, worst, ratio = LR.check(got[y0:y1], v, m, LR.K[f])
            RATIOS[f] = max(RATIOS[f], ratio)
            print("[ratio] %s %dx%d image %d rows %d..%d %s %.3g" % (name, H, W, b, y0, y1, f, ratio))
            assert ok, "%s image %d rows %d..%d (%s): %.3g of the bound, ratio %.3g" % (name, b, y0, y1, f, worst, ratio)
    for name, (ld, lu, inputs, op) in LR.COMPOSITE.items():
        if names and name not in names:
            continue
        fd, fu = LR.family_of(*seq[ld]), LR.family_of(*seq[lu])
        got, inp = t.get(name), [t.get(i) for i in inputs]
        for y0, y1 in LR.strips(got.shape[0]):
            v, mu, md = op(inp, weights, st, y0, y1)
            err = np.abs(got[y0:y1].astype(np.float64) - v)
            bound = LR.U * (LR.K[fd] * md + LR.K[fu] * mu + np.abs(v))
            assert np.all(err <= bound), "%s image %d rows %d..%d: %.3g of the bound" % (name, b, y0, y1, float((err / bound).max()))
    return fam, t.layout


def frames_for(pkg, B, H, W, seed=0):
    return np.stack([pkg.synth_frame(seed + i, H, W, kind="smooth") for i in range(B)])


SHAPES = [(1, 8, 8), (1, 33, 31), (1, 77, 90), (1, 200, 136), (1, 264, 40), (1, 1032, 8), (5, 40, 56),
          (1, 8, 1032),      # wide and thin: one tile row, 65 tile columns at full resolution
          (1, 41, 37)]       # a level-0 width = 1 (mod 4): the P8 rows and their 16-byte pieces run along x
ENC_F43 = ("p1", "c21", "p2", "c31", "c32", "c33", "p3")       # conv1_2 .. conv3_4
DEC_F43 = ("o4", "o3", "o2")                                   # ResidualBlock.conv2


def assert_kind(kind, fam, lay):
    """The kernel families and layouts a case of `kind` claims to cover ran."""
    assert fam["c11"] == fam["pre"] == "direct"
    assert fam["xs4"] == fam["a4"] == fam["a3"] == fam["a2"] == "ups"
    assert fam["d"] in ("splitk", "f23") and fam["f3"] == fam["c41"] == "f23"
    if kind == "f23":
        assert all(fam[n] == "f23" for n in ENC_F43 + DEC_F43)
        assert not any(lay.values()), lay
    else:
        assert all(fam[n] == "f43" for n in ENC_F43 + DEC_F43), fam
        p8_names = ("c11",) + ENC_F43[:-1] + ("a4", "a3", "a2")
        assert all(lay[n] == (1 if kind == "f43_p8" else 0) for n in p8_names), lay
        assert lay["p3"] == 0


KINDS = {"f23": (0, 3), "f43_p8": (2, 3), "f43_nhwc": (2, 0)}      # kind -> (rrv_set_f43 mode, RRV_P8)


@pytest.mark.parametrize("kind", ["f23", "f43_p8", "f43_nhwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_every_layer_against_its_own_input(pkg, weights, kind, shape):
    B, H, W = shape
    blob = load_golden("global_a")["state"]
    st = LR.parse_state(blob)
    frames = frames_for(pkg, B, H, W)
    mode, p8 = KINDS[kind]
    s, seq, _ = launch(pkg, weights, frames, blob, mode, p8=p8)
    try:
        for b in sorted({0, B - 1}):
            fam, lay = check_image(s, weights, st, seq, H, W, b, frames[b])
            assert_kind(kind, fam, lay)
    finally:
        s.close()


CLAMP_SHAPE = (5, 40, 56)
_CLAMP = {}


def clamp_setup(pkg, weights):
    """(frames, blob, construction shares) of the clamp-end state for CLAMP_SHAPE, built once for the module."""
    if not _CLAMP:
        frames = frames_for(pkg, *CLAMP_SHAPE)
        blob, shares = LR.clamp_state(weights, load_golden("global_a")["state"], list(frames))
        _CLAMP["v"] = (frames, blob, shares)
    return _CLAMP["v"]


@pytest.mark.parametrize("kind", ["f23", "f43_p8", "f43_nhwc"])
def test_clamp_ends_on_every_channel(pkg, weights, kind):
    """global_a with lo / hi of every channel at every norm point moved to the 30th / 70th percentile of its pre-clamp value over the five
    frames (LR.clamp_state; means, rstds, filters and style statistics untouched, so the kernel choice is what it was): every stage of all
    five images within its bound.  Conditions, not measurements: on the float64 forward the state was built from, every channel that is
    not constant has at least 0.2 of its values at lo, 0.2 at hi and 0.2 strictly inside; on the teacher-forced reference of the GPU's own
    taps (they differ from that forward by rounding only) at least 0.1 each.  The share inside is not asked of a channel with more than
    half of its values on one value: 237 of Decoder.norm[0]'s 498 live channels, where conv4_1's ReLU leaves 50 .. 99 % zeros at these
    frames and both percentiles fall on the zero (their shares at lo and at hi are still asked; no channel of the other ten norm points)."""
    B, H, W = CLAMP_SHAPE
    frames, blob, built = clamp_setup(pkg, weights)
    assert LR.clamp_conditions(built, 0.2) == []
    st = LR.parse_state(blob)
    mode, p8 = KINDS[kind]
    s, seq, _ = launch(pkg, weights, frames, blob, mode, p8=p8)
    try:
        pre = {n: [] for n in built}
        for b in range(B):
            t = Taps(s, H, W, b, frames[b])
            fam, lay = check_image(s, weights, st, seq, H, W, b, frames[b], taps=t)
            assert_kind(kind, fam, lay)
            for n in built:
                pre[n].append(LR.norm_pre(n, t.get, weights, st))
        forced = {n: LR.clamp_shares(pre[n], st["norm"][n][2], st["norm"][n][3]) for n in built}
        for n, (at_lo, at_hi, inside, live, atom) in sorted(forced.items()):
            live = built[n][3]
            print("[clamp shares] %s norm %d: at lo >= %.3f, at hi >= %.3f, inside >= %.3f (channels asked: %d, %d of them not for the inside)"
                  % (kind, n, at_lo[live].min(), at_hi[live].min(), inside[live & (built[n][4] <= LR.ATOM)].min(), live.sum(),
                     (live & (built[n][4] > LR.ATOM)).sum()))
        assert LR.clamp_conditions(forced, 0.1, masks={n: (built[n][3], built[n][4]) for n in built}) == []
    finally:
        s.close()


def test_headline_launch_default_choice(pkg, weights):
    """What bench.py times: 16 frames of 640 x 640 in the default kernel choice; images 0, 7 and 15 on row strips."""
    g = load_golden("global_a")
    st = LR.parse_state(g["state"])
    frames = frames_for(pkg, 16, 640, 640)
    s, seq, _ = launch(pkg, weights, frames, g["state"], 1)
    try:
        for b in (0, 7, 15):
            fam, lay = check_image(s, weights, st, seq, 640, 640, b, frames[b])
        assert fam["d"] == "splitk"
        assert all(fam[n] == "f43" for n in ENC_F43 + DEC_F43), fam        # the default picks F(4x4,3x3) for this launch ...
        assert all(lay[n] == 1 for n in ("c11",) + ENC_F43[:-1] + ("a4", "a3", "a2")), lay      # ... with P8 between
    finally:
        s.close()


@pytest.mark.parametrize("H,W,split", [(640, 640, 8), (1152, 1152, 4), (1536, 2048, 1)])
def test_split_k_kernel_filter(pkg, weights, H, W, split):
    """filter_down's split K (8 / 4 / 1 slices by the relu4_1 tile count) and the folded up conv behind it."""
    blob = load_golden("global_a")["state"]
    st = LR.parse_state(blob)
    frames = frames_for(pkg, 1, H, W)
    s, seq, _ = launch(pkg, weights, frames, blob, 0)
    try:
        assert [sp for _, sp in seq[9:15:2]] == [split > 1] * 3
        if split > 1:
            _, lay, ch = s.debug_tensor_ex(0, LR.TAP["dpart"], H, W, 0)
            assert lay == 0 and ch == 32 * split
        else:
            with pytest.raises(pkg.RRVError):
                s.debug_tensor_ex(0, LR.TAP["dpart"], H, W, 0)
        check_image(s, weights, st, seq, H, W, 0, frames[0], names=("c41", "d", "f1", "f2", "f3"))
    finally:
        s.close()


def test_old_and_new_taps_agree(pkg, weights):
    """rrv_debug_copy_tensor and rrv_debug_copy_tensor_ex return the same bytes for indices 0..22, image 0."""
    blob = load_golden("global_a")["state"]
    frames = frames_for(pkg, 2, 77, 90)
    s, _, _ = launch(pkg, weights, frames, blob, 0)
    try:
        for i in range(23):
            a, lay, _ = s.debug_tensor_ex(0, i, 77, 90, 0)
            assert lay == 0
            np.testing.assert_array_equal(a, s.debug_tensor(0, i, 77, 90))
        with pytest.raises(pkg.RRVError, match="did not write this image"):
            s.debug_tensor_ex(0, 0, 77, 90, 2)
        with pytest.raises(pkg.RRVError, match="did not write|no such tensor"):
            s.debug_tensor_ex(0, LR.TAP["q11"], 77, 90, 0)       # the mode-0 launch wrote the NHWC c11, not its twin
    finally:
        s.close()


def test_p8_twins_are_built_with_the_plan(pkg, weights):
    """The P8 twins come with the per-frame plan: a launch that takes the P8 chain on the plan an NHWC launch built allocates
    nothing, and gives the bits of a fresh P8 launch."""
    blob = load_golden("global_a")["state"]
    frames = frames_for(pkg, 3, 48, 64)
    s, _, d_out = launch(pkg, weights, frames, blob, 0)
    ref, _, d_ref = launch(pkg, weights, frames, blob, 2)
    try:
        s.set_pipeline(1)            # the profiled launch ran on slot 0 and moved next_slot on: the next call reuses slot 0's plan
        s.set_f43(2)
        d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        torch.cuda.synchronize()
        s.debug_fail_alloc(1)        # any device allocation from here on fails
        try:
            s.transfer_batch_device(d_in.data_ptr(), 3, 48, 64, d_out.data_ptr())
            s.sync()
        finally:
            s.debug_fail_alloc(0)
        _, lay, _ = s.debug_tensor_ex(0, LR.TAP["q11"], 48, 64, 0)      # the mode-0 launch wrote c11, this one its twin
        assert lay == 1
        assert torch.equal(d_out, d_ref)
    finally:
        s.close()
        ref.close()


def test_p8_offset_band_frame(pkg, weights):
    """A frame the size guard admits ((H+2)(W+2)64 < 2^31) whose full-resolution P8 images would not fit 32-bit offsets
    ((H+2)(W+8)64 >= 2^31): the full-resolution tensors keep NHWC, rows beyond the mark repeat the periodic interior bit for
    bit, and the output equals an all-NHWC handle's bit for bit."""
    H, W = 900032, 32
    assert (H + 2) * (W + 2) * 64 < 2 ** 31 <= (H + 2) * (W + 8) * 64
    mark = 2 ** 31 // ((W + 8) * 64)
    blob = load_golden("global_a")["state"]
    strip = pkg.synth_frame(900, 64, W, kind="smooth")
    frame = np.tile(strip, (H // 64, 1, 1))[None]
    outs = []
    for p8 in (3, 0):
        s, _, d_out = launch(pkg, weights, frame, blob, 2, p8=p8)
        try:
            out = d_out[0].cpu().numpy()
            del d_out
            if p8 == 3:
                _, lay, _ = s.debug_tensor_ex(0, LR.TAP["c11"], H, W, 0)         # P8 refused at full resolution ...
                assert lay == 0
                _, lay, _ = s.debug_tensor_ex(0, LR.TAP["qa3"], H, W, 0)        # ... kept where it fits
                assert lay == 1
            outs.append(out)
        finally:
            s.close()
    out = outs[0]
    assert out.shape == (H, W, 3) and np.isfinite(out).all()
    top = out[512:576]
    assert float(top.std()) > 1.0
    for y0 in (H // 2 // 64 * 64, (mark + 64) // 64 * 64, H - 1024):
        np.testing.assert_array_equal(out[y0:y0 + 64], top)
    np.testing.assert_array_equal(outs[0], outs[1])

"""The per-layer checker of tests/test_gpu_layers.py checked on the CPU: the oracle's float32 numpy arithmetic stands in for
a kernel.  It must pass within the direct family's K, and fail on each defect a GPU layer test is there to catch."""
import numpy as np
import pytest

import layer_ref as LR
from state_bounds import load_golden

H, W = 64, 80       # the frame: p1 is 32 x 40 (two 16-pixel tiles and a partial one per row), p3 is 8 x 10


@pytest.fixture(scope="module")
def setup(pkg, weights, oracle):
    prev = oracle.CONV_BACKEND
    oracle.set_conv_backend("numpy")
    try:
        frames = [pkg.synth_frame(i, H, W, kind="smooth") for i in range(2)]
        acts = []
        for f in frames:
            x = oracle.rgb2gray(oracle.image_to_tensor(f))
            x = oracle.maxpool2(oracle.relu(oracle.conv3x3(oracle.relu(oracle.conv3x3(x, weights["Encoder.slice.0.weight"], weights["Encoder.slice.0.bias"])),
                                                           weights["Encoder.slice.2.weight"], weights["Encoder.slice.2.bias"])))
            p1 = x[0]
            for i in (5, 7):
                x = oracle.relu(oracle.conv3x3(x, weights["Encoder.slice.%d.weight" % i], weights["Encoder.slice.%d.bias" % i]))
            x = oracle.maxpool2(x)
            for i in (10, 12, 14, 16):
                x = oracle.relu(oracle.conv3x3(x, weights["Encoder.slice.%d.weight" % i], weights["Encoder.slice.%d.bias" % i]))
            acts.append((p1, oracle.maxpool2(x)[0]))
        states = [LR.parse_state(load_golden(n)["state"]) for n in ("global_a", "global_b")]
        yield oracle, acts, states
    finally:
        oracle.set_conv_backend(prev)


def _c21(oracle, weights, p1, w=None, b=None):
    """The stand-in kernel for Encoder conv2_1 (64 -> 128, ReLU): float32 numpy."""
    w = weights["Encoder.slice.5.weight"] if w is None else w
    b = weights["Encoder.slice.5.bias"] if b is None else b
    return oracle.relu(oracle.conv3x3(p1[None], w, b))[0]


def _c41(oracle, weights, p3, st):
    """The stand-in for conv4_1 with Decoder.norm[0] in the epilogue (float32), state st (parsed)."""
    y = oracle.relu(oracle.conv3x3(p3[None], weights["Encoder.slice.19.weight"], weights["Encoder.slice.19.bias"]))[0]
    mean, rstd, lo, hi = (np.asarray(a, np.float32) for a in st["norm"][0])
    return np.minimum(hi, np.maximum(lo, (y - mean) * rstd)).astype(np.float32)


def _verdict(got, name, inp, weights, st):
    _, _, op, _ = LR.STAGES[name]
    v, m = op(inp, weights, st, 0, got.shape[0])
    return LR.check(got, v, m, LR.K["direct"])


def test_float32_stand_in_passes(setup, weights):
    oracle, acts, states = setup
    for (p1, p3), st in zip(acts, states):
        ok, worst, ratio = _verdict(_c21(oracle, weights, p1), "c21", [p1], weights, st)
        assert ok, "conv2_1 stand-in at %.2f of its bound (ratio %.2f)" % (worst, ratio)
        ok, worst, ratio = _verdict(_c41(oracle, weights, p3, st), "c41", [p3], weights, st)
        assert ok, "conv4_1 + norm0 stand-in at %.2f of its bound (ratio %.2f)" % (worst, ratio)


def _defects(oracle, weights, p1):
    w5, b5 = weights["Encoder.slice.5.weight"], weights["Encoder.slice.5.bias"]
    good = _c21(oracle, weights, p1)
    out = {}
    q = p1.copy()
    q[..., 8:16] = 0                                   # one 8-channel chunk of the 64 input channels dropped
    out["chunk dropped"] = _c21(oracle, weights, q)
    g = good.copy()
    g[:, 15::16] = g[:, 14::16]                        # the last column of every 16-pixel tile = its neighbour's value
    out["tile column"] = g
    c = int(np.argmax((good > 0).mean(axis=(0, 1)) * np.abs(b5)))
    b = b5.copy()
    b[c] = 0                                           # one channel's bias missing
    out["bias dropped"] = _c21(oracle, weights, p1, b=b)
    w = w5.copy()
    w.flat[int(np.argmax(np.abs(w5)))] *= np.float32(1 + 2.0 ** -8)     # one weight off by one part in 256
    out["weight scaled"] = _c21(oracle, weights, p1, w=w)
    return out


DEFECTS = ("chunk dropped", "tile column", "bias dropped", "weight scaled")


@pytest.mark.parametrize("defect", DEFECTS)
def test_injected_defect_fails(setup, weights, defect):
    oracle, acts, states = setup
    p1 = acts[0][0]
    ok, worst, _ = _verdict(_defects(oracle, weights, p1)[defect], "c21", [p1], weights, states[0])
    assert not ok, "%s passes the bound (worst %.2f)" % (defect, worst)


def test_image_given_another_images_state_fails(setup, weights):
    """A grouped launch whose image 1 reads image 0's state (a per-image stride of 0)."""
    oracle, acts, states = setup
    p3 = acts[1][1]
    wrong = _c41(oracle, weights, p3, states[0])
    ok, worst, _ = _verdict(wrong, "c41", [p3], weights, states[1])
    assert not ok, "image 1 on image 0's state passes the bound (worst %.2f)" % worst


# ---- per-image Decoder.norm[0]: the references of tests/test_gpu_instantiations.py, cases a and b ---------------------------------

PI_STATES = ("global_a", "global_b", "global_a_seed1")
PI_WTS = np.array([[0.6, 0.3, 0.1], [0.1, 0.25, 0.65]], np.float32)      # image 0, image 1: every style active in both


def _blend32(blobs, w):
    """blend_sets_k's stand-in: float32 products summed in style order."""
    out = np.zeros_like(blobs[0])
    for s, b in enumerate(blobs):
        out = (out + w[s] * b).astype(np.float32)
    return out


def _c41_per_image(oracle, weights, p3, st, defect=None):
    """conv4_1 + ReLU, then Decoder.norm[0] of state st in float32: the fused epilogue (case a) and pointwise_k on a cached feature
    (case b) are this arithmetic.  defect: 'raw' = the un-normalised feature, 'lo / hi exchanged'."""
    y = oracle.relu(oracle.conv3x3(p3[None], weights["Encoder.slice.19.weight"], weights["Encoder.slice.19.bias"]))[0]
    if defect == "raw":
        return y
    mean, rstd, lo, hi = (np.asarray(a, np.float32) for a in st["norm"][0])
    if defect == "lo / hi exchanged":
        lo, hi = hi, lo
    return np.minimum(hi, np.maximum(lo, (y - mean) * rstd)).astype(np.float32)


def _per_image_verdict(case, got, p3, weights, st):
    if case == "a":         # the fused epilogue: the c41 stage on the image's blended set
        return _verdict(got, "c41", [p3], weights, st)[:2]
    return LR.check2(got, *LR.cached_c41(p3, weights, st), LR.K["direct"], LR.K["point"])[:2]      # (float32 numpy stands in at the direct family's K)


@pytest.fixture(scope="module")
def per_image(setup):
    blobs = [np.asarray(load_golden(n)["state"], np.float32).reshape(-1) for n in PI_STATES]
    sets = []
    for w in PI_WTS:
        blob = _blend32(blobs, w)
        ref, mag = LR.blend_ref(blobs, w)
        assert np.all(np.abs(blob - ref) <= LR.K["stat"] * LR.U * mag)
        sets.append(LR.parse_state(blob))
    m0, m1 = sets[0]["norm"][0][0], sets[1]["norm"][0][0]
    assert np.abs(m0 - m1).max() > 1e-4 * np.abs(m0).max()        # the two images' sets differ where conv4_1 reads them
    return sets


@pytest.mark.parametrize("case", ["a", "b"])
def test_per_image_norm0_stand_in_passes(setup, per_image, weights, case):
    oracle, acts, _ = setup
    for b, st in enumerate(per_image):
        p3 = acts[b][1]
        ok, worst = _per_image_verdict(case, _c41_per_image(oracle, weights, p3, st), p3, weights, st)
        assert ok, "case %s image %d: stand-in at %.2f of its bound" % (case, b, worst)


@pytest.mark.parametrize("defect", ["neighbour's norm[0]", "lo / hi exchanged", "raw"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_per_image_norm0_defect_fails(setup, per_image, weights, case, defect):
    """Image 1 normalised with image 0's blended entry (a per-image stride of 0), clamped with lo and hi exchanged, or left raw."""
    oracle, acts, _ = setup
    p3 = acts[1][1]
    wrong = _c41_per_image(oracle, weights, p3, per_image[0 if defect.startswith("neighbour") else 1],
                           defect=None if defect.startswith("neighbour") else defect)
    ok, worst = _per_image_verdict(case, wrong, p3, weights, per_image[1])
    assert not ok, "case %s: %s passes the bound (worst %.2f)" % (case, defect, worst)


# ---- clamp ends on every channel: the state of tests/test_gpu_layers.py::test_clamp_ends_on_every_channel ------------------------------------------

CLAMP_SHAPE = (5, 40, 56)


@pytest.fixture(scope="module")
def clamp(pkg, weights):
    frames = [pkg.synth_frame(i, *CLAMP_SHAPE[1:], kind="smooth") for i in range(CLAMP_SHAPE[0])]
    blob0 = np.asarray(load_golden("global_a")["state"], np.float32).reshape(-1)
    blob, shares = LR.clamp_state(weights, blob0, frames)
    return blob0, blob, shares


def test_clamp_state_cuts_into_every_channel(clamp):
    """The construction-time conditions: at every norm point every channel that is not constant has 0.2 of its values at lo, 0.2 at hi and
    0.2 strictly inside (the inside share is not asked where more than half of a channel sits on one value: ReLU's zeros at
    Decoder.norm[0], and nowhere else); nothing but lo and hi differs from the blob it was built from."""
    blob0, blob, shares = clamp
    assert LR.clamp_conditions(shares, 0.2) == []
    st0, st = LR.parse_state(blob0), LR.parse_state(blob)
    for n, (at_lo, at_hi, inside, live, atom) in shares.items():
        assert live.sum() >= 0.95 * live.size, (n, int(live.sum()))
        assert not np.any(live & (atom > LR.ATOM)) or n == 0, n
        assert np.all(inside[live & (atom <= LR.ATOM)] >= 0.2) and np.all(at_lo[live] >= 0.2) and np.all(at_hi[live] >= 0.2), n
        for k in (0, 1):
            assert np.array_equal(st["norm"][n][k], st0["norm"][n][k])
        for k in (2, 3):      # a constant channel keeps the blob's ends
            assert np.array_equal(st["norm"][n][k][~live], st0["norm"][n][k][~live])
        assert np.all(st["norm"][n][2] <= st["norm"][n][3])
    assert all(np.array_equal(st["filt"][k], st0["filt"][k]) for k in st["filt"])
    assert all(np.array_equal(a, b) for x, y in zip(st["sty"], st0["sty"]) for a, b in zip(x, y))
    # the check itself can fail: with the golden state's own ends almost nothing clamps
    assert LR.clamp_conditions({0: LR.clamp_shares([np.zeros((2, 2, 4)), np.ones((2, 2, 4))], np.full(4, -9.0), np.full(4, 9.0))}, 0.2)


def _c41_clamp(oracle, weights, p3, st, defect=None):
    """conv4_1 + ReLU + Decoder.norm[0] in float32 on state st; defect: the ends of channel c + 4, the ends exchanged, no clamp."""
    y = oracle.relu(oracle.conv3x3(p3[None], weights["Encoder.slice.19.weight"], weights["Encoder.slice.19.bias"]))[0]
    mean, rstd, lo, hi = (np.asarray(a, np.float32) for a in st["norm"][0])
    v = ((y - mean) * rstd).astype(np.float32)
    if defect == "clamp omitted":
        return v
    if defect == "lo / hi of channel c + 4":
        lo, hi = np.roll(lo, -4), np.roll(hi, -4)
    if defect == "lo and hi exchanged":
        lo, hi = hi, lo
    return np.minimum(hi, np.maximum(lo, v)).astype(np.float32)


def test_clamp_state_stand_in_passes(setup, clamp, weights):
    oracle, acts, _ = setup
    st = LR.parse_state(clamp[1])
    for _, p3 in acts:
        ok, worst, ratio = _verdict(_c41_clamp(oracle, weights, p3, st), "c41", [p3], weights, st)
        assert ok, "conv4_1 + clamped norm0 stand-in at %.2f of its bound (ratio %.2f)" % (worst, ratio)


@pytest.mark.parametrize("defect", ["lo / hi of channel c + 4", "lo and hi exchanged", "clamp omitted"])
def test_clamp_defect_fails(setup, clamp, weights, defect):
    oracle, acts, _ = setup
    st = LR.parse_state(clamp[1])
    p3 = acts[0][1]
    ok, worst, _ = _verdict(_c41_clamp(oracle, weights, p3, st, defect), "c41", [p3], weights, st)
    assert not ok, "%s passes the bound (worst %.2f)" % (defect, worst)


def test_nine_tap_conv_mfma_rows_are_the_gemm_family():
    assert LR.family_of("conv_mfma<64,9,E_RELU | E_POOL>@64x64@40x56", False) == "gemm"
    assert LR.family_of("conv_mfma<128,9,E_RELU | E_NORM1>@256x512@5x7", False) == "gemm"
    assert LR.family_of("conv_mfma<128,1,0>@512x256@5x7", False) == "direct"
    assert LR.family_of("conv_wino<E_RELU | E_NORM1>@256x512@5x7", False) == "f23"


def test_k_within_four_times_the_measured_maximum():
    assert set(LR.MEASURED) == set(LR.K) == set(LR.FAMILIES) and {"stat", "point", "pred", "pstat", "gemm", "ppred"} <= set(LR.FAMILIES)
    for f in LR.FAMILIES:
        assert 0 < LR.MEASURED[f] <= LR.K[f] <= 4 * LR.MEASURED[f], f


# ---- frame mode: the references of tests/test_gpu_frame_mode_layers.py ---------------------------------------------------

STYLE = dict(H=64, W=64, kind="smooth", seed=7)
FM_NAMES = tuple(n for n in LR.FRAME_STAGES[:LR.FRAME_STAGES.index("o4") + 1] if n not in LR.FRAME_ENC)      # c41 .. block slice4
CPU_FAM = {n: "direct" for n in LR.FRAME_ENC + ("c41", "d0", "u0", "d1", "u1", "d2", "u2", "a4", "o4", "a3", "o3", "a2", "o2", "pre")}


def _style(oracle, pkg, weights):
    """(F_style of the oracle, style statistics in blob order, float64 style half of the six filter predictions)."""
    F = oracle.Net(weights).encoder_style(oracle.image_to_tensor(pkg.synth_style(**STYLE)))
    m4, s4 = F["relu4_1"]
    sn = ((F["map"] - m4) / s4).astype(np.float32)[0]
    smean = np.stack([LR.conv3(sn, weights["Decoder.%s.down_sample.0.weight" % n], weights["Decoder.%s.down_sample.0.bias" % n],
                               0, sn.shape[0])[0].reshape(-1, 32).mean(axis=0) for n in LR.FILTER_NAMES])
    sty = [tuple(np.asarray(a, np.float64) for a in F[n]) for n in ("relu1_1", "relu2_1", "relu3_1", "relu4_1")]
    return F, sty, smean


def _empty_state(sty):
    return {"norm": [(np.zeros(C), np.ones(C), np.full(C, LR.NO_LO), np.full(C, LR.NO_HI)) for C in LR.NORM_CH], "filt": {}, "sty": sty}


def _stats32(oracle, x, nminus1=False):
    """chan_stat1_k + chan_stat1_final_k on [H,W,C] float32: the state-set entry (float64 views of float32 values)."""
    C = x.shape[-1]
    flat = x.reshape(-1, C)
    mean = oracle._mean32(flat, axis=0)
    xc = flat - mean
    var = np.sum(xc.astype(np.float64) ** 2, axis=0) / (flat.shape[0] - (1 if nminus1 else 0))
    rstd = (np.float32(1) / np.sqrt(var.astype(np.float32) + np.float32(1e-8))).astype(np.float32)
    return mean.astype(np.float64), rstd.astype(np.float64), np.full(C, LR.NO_LO), np.full(C, LR.NO_HI)


def _pred32(x, w, name, smean, tall=False):
    """rect_sums_k + pred_mean_k + fc_filter_k on [H,W,512] float32.  tall: the rectangles of the taps that look up (dy < 0) keep
    the last row (y < H instead of y < H - 1)."""
    H, W, _ = x.shape
    p = "Decoder.%s." % name
    wd = np.asarray(w[p + "down_sample.0.weight"], np.float64)
    x64, acc = x.astype(np.float64), np.zeros(32)
    for t in range(9):
        dy, dx = t // 3 - 1, t % 3 - 1
        ys = slice(0, H if tall else H - 1) if dy < 0 else slice(1, H) if dy > 0 else slice(0, H)
        xs = slice(0, W - 1) if dx < 0 else slice(1, W) if dx > 0 else slice(0, W)
        S = x64[ys, xs].sum(axis=(0, 1)).astype(np.float32).astype(np.float64)
        acc += wd[:, :, t // 3, t % 3] @ S
    c = (acc / (H * W) + np.asarray(w[p + "down_sample.0.bias"], np.float64)).astype(np.float32)
    v = np.concatenate([c, np.asarray(smean, np.float32)])
    return (w[p + "FC.weight"] @ v + w[p + "FC.bias"]).astype(np.float32).reshape(32, 32)


def _standin(oracle, weights, frame, sty, smean, defect=None, other=None):
    """The frame-mode chain up to block slice4 in the oracle's float32 arithmetic, stage by stage as the kernels run it:
    (taps, state set).  `defect` plants one of the wrong values the GPU suite is there to catch; `other`: image 0's state set
    for the defects that read a neighbour's."""
    O, w = oracle, weights
    x = O.rgb2gray(O.image_to_tensor(frame))
    for idx in O.VGG_IDX[:-1]:
        x = O.relu(O.conv3x3(x, w["Encoder.slice.%d.weight" % idx], w["Encoder.slice.%d.bias" % idx]))
        if idx in O.POOL_AFTER:
            x = O.maxpool2(x)
    taps, st = {"p3": x[0]}, _empty_state(sty)

    def normed(t, e):
        return ((t - e[0].astype(np.float32)) * e[1].astype(np.float32)).astype(np.float32)

    raw = O.relu(O.conv3x3(x, w["Encoder.slice.19.weight"], w["Encoder.slice.19.bias"]))
    st["norm"][0] = _stats32(O, raw[0], nminus1=defect == "variance over N - 1")
    cur = normed(raw, other["norm"][0] if defect == "statistics of image 0" else st["norm"][0])
    taps["c41"] = cur[0]
    for f in range(3):
        fn = "Filter%d" % (f + 1)
        for g in (1, 2):
            st["filt"]["%s.F%d" % (fn, g)] = _pred32(cur[0], w, "%s.F%d" % (fn, g), smean[2 * f + g - 1],
                                                     tall=defect == "rectangle one row too tall").astype(np.float64)
        use = other if (defect == "filter of image 0 in Filter 2" and f == 1) else st
        F1, F2 = (use["filt"]["%s.F%d" % (fn, g)].astype(np.float32) for g in (1, 2))
        p = "Decoder.%s." % fn
        d = O.lrelu(O.apply_filter(O.conv3x3(cur, w[p + "down_sample.0.weight"], w[p + "down_sample.0.bias"]), F1))
        cur = cur + O.conv3x3(O.apply_filter(d, F2), w[p + "upsample.0.weight"], w[p + "upsample.0.bias"])
        taps["f%d" % (f + 1)] = cur[0]
    taps["d"] = d[0]
    m4, s4 = (a.astype(np.float32) for a in sty[3])
    cur = (cur * s4 + m4).astype(np.float32)
    taps["f3"] = cur[0]
    n1, n2, na, si = LR.RES["slice4"]
    taps["xs4"] = O.conv1x1(cur, w["Decoder.slice4.conv_shortcut.weight"])[0]
    a = O.lrelu(O.conv3x3(O.upsample2(cur), w["Decoder.slice4.conv1.weight"], w["Decoder.slice4.conv1.bias"]))
    st["norm"][n1] = _stats32(O, a[0])
    a = normed(a, st["norm"][n1])
    taps["a4"] = a[0]
    c2 = O.lrelu(O.conv3x3(a, w["Decoder.slice4.conv2.weight"], w["Decoder.slice4.conv2.bias"]))
    st["norm"][n2] = _stats32(O, c2[0])
    xsu = O.upsample2(taps["xs4"][None])
    h = normed(c2 + xsu, st["norm"][n2]) if defect == "shortcut before the normalisation" else normed(c2, st["norm"][n2]) + xsu
    st["norm"][na] = _stats32(O, h[0])
    ms, ss = (v.astype(np.float32) for v in sty[si])
    taps["o4"] = (normed(h, st["norm"][na]) * ss + ms).astype(np.float32)[0]
    return taps, st


@pytest.fixture(scope="module")
def fm(pkg, weights, oracle):
    prev = oracle.CONV_BACKEND
    oracle.set_conv_backend("numpy")
    try:
        _, sty, smean = _style(oracle, pkg, weights)
        frames = [pkg.synth_frame(0, 64, 80, kind="smooth"), pkg.synth_frame(1, 64, 80, kind="noise")]
        good = [_standin(oracle, weights, f, sty, smean) for f in frames]
        yield oracle, frames, sty, smean, good
    finally:
        oracle.set_conv_backend(prev)


def _failed(taps, st, weights, smean, names=FM_NAMES):
    return {n: worst for n, _, ok, worst, _ in LR.frame_checks(taps.__getitem__, weights, st, smean, CPU_FAM, names=names) if not ok}


def test_frame_mode_float32_stand_in_passes(fm, weights):
    _, _, _, smean, good = fm
    for b, (taps, st) in enumerate(good):
        bad = _failed(taps, st, weights, smean)
        assert not bad, "image %d: %s" % (b, bad)


FM_DEFECTS = {"variance over N - 1": {"stat0"}, "rectangle one row too tall": {"pred0.F1", "pred0.F2"}, "statistics of image 0": {"c41"},
              "filter of image 0 in Filter 2": {"f2"}, "shortcut before the normalisation": {"o4"}}


@pytest.mark.parametrize("defect", sorted(FM_DEFECTS))
def test_frame_mode_injected_defect_fails(fm, weights, defect):
    """Image 1 with one wrong value planted; the stages that see it must fail at the committed K."""
    oracle, frames, sty, smean, good = fm
    taps, st = _standin(oracle, weights, frames[1], sty, smean, defect=defect, other=good[0][1])
    bad = _failed(taps, st, weights, smean)
    assert set(bad) >= FM_DEFECTS[defect], "%s: only %s fail" % (defect, bad)


def test_float64_frame_stages_reproduce_the_reference_golden(pkg, weights, oracle):
    """All float64 stages composed from the golden's frame give tests/golden/frame_mode.npz's pre-clamp output within the
    stated PRE_ATOL / PRE_RTOL (the stage table follows the unmodified reference), and LR.frame_checks accepts the composed
    taps with the composed statistics (its arithmetic is that composition)."""
    from state_bounds import assert_pre_close
    frame = oracle.reflect_pad(pkg.synth_frame(2, 64, 48, kind="smooth"), 192, 192)
    _, sty, smean = _style(oracle, pkg, weights)
    w, st = weights, _empty_state(sty)
    taps = {"frame": LR.grey_input(frame)}

    def full(op, inputs, rows):
        return op([taps[i] for i in inputs], w, st, 0, rows)[0]

    def stats(v):
        f = v.reshape(-1, v.shape[-1])
        return f.mean(axis=0), 1.0 / np.sqrt(f.var(axis=0) + LR.EPS32), np.full(v.shape[-1], LR.NO_LO), np.full(v.shape[-1], LR.NO_HI)

    for name in LR.FRAME_ENC:
        _, inputs, op, geo = LR.STAGES[name]
        taps[name] = full(op, inputs, geo(192, 192)[0])
    raw = full(LR._enc_stage(19, ()), ["p3"], 24)
    st["norm"][0] = stats(raw)
    taps["c41"] = LR.norm(raw, raw, st["norm"][0])[0]
    cur = "c41"
    for f in range(3):
        for g in (1, 2):
            name = "Filter%d.F%d" % (f + 1, g)
            st["filt"][name] = LR.predict_filter(taps[cur], w, name, smean[2 * f + g - 1])[0]
        taps["d"] = full(LR._down(f), [cur], 24)
        taps["f%d" % (f + 1)] = full(LR._up(f), ["d", cur], 24)
        cur = "f%d" % (f + 1)
    for blk, xin, xs, a, o in LR.FRAME_BLOCKS:
        n1, n2, na, si = LR.RES[blk]
        p = "Decoder.%s." % blk
        x = taps[xin]
        taps[xs] = LR.conv1(x, w[p + "conv_shortcut.weight"], 0, x.shape[0])[0]
        v = LR.lrelu(*LR.conv3(x, w[p + "conv1.weight"], w[p + "conv1.bias"], 0, 2 * x.shape[0], ups=True))[0]
        st["norm"][n1] = stats(v)
        taps[a] = LR.norm(v, v, st["norm"][n1])[0]
        v = LR.lrelu(*LR.conv3(taps[a], w[p + "conv2.weight"], w[p + "conv2.bias"], 0, 2 * x.shape[0]))[0]
        st["norm"][n2] = stats(v)
        h = LR.norm(v, v, st["norm"][n2])[0] + LR._up2(taps[xs], *v.shape[:2])
        st["norm"][na] = stats(h)
        taps[o] = LR.adain(h, h, st["norm"][na], sty[si])[0]
    taps["pre"] = full(LR._last, ["o2"], 192)
    assert_pre_close(taps["pre"][64:128, 64:112].astype(np.float32), load_golden("frame_mode")["pre_crop"])
    bad = {n: worst for n, _, ok, worst, _ in LR.frame_checks(taps.__getitem__, w, st, smean, CPU_FAM) if not ok}
    assert not bad, bad


# ---- the masked multi-style walk: the references of tests/test_gpu_mask_layers.py -------------------------------------------

import mask_layer_ref as MR      # noqa: E402
import mask_ref                  # noqa: E402

MK_NAMES = ("c41", "f1", "f2", "dpart", "d", "f3", "xs4", "a4", "o4", "xs3", "a3", "o3")
MK_SPLIT = 8
MK_STATES = ("global_a", "global_b", "global_a_seed1")


def _mask_standin(oracle, weights, frame, blobs, M, defect=None):
    """The masked walk up to block slice3 in the oracle's float32 arithmetic, stage by stage as the kernels run it, the split-K
    slices included: the taps, level masks as the GPU's decoded taps.  `defect` plants one wrong step."""
    O, w = oracle, weights
    lv = mask_ref.level_masks(M)
    st = [mask_ref._unpack(b) for b in (blobs[::-1] if defect == "styles blended in swapped order" else blobs)]
    S = len(st)
    x = O.rgb2gray(O.image_to_tensor(frame))
    for idx in O.VGG_IDX[:-1]:
        x = O.relu(O.conv3x3(x, w["Encoder.slice.%d.weight" % idx], w["Encoder.slice.%d.bias" % idx]))
        if idx in O.POOL_AFTER:
            x = O.maxpool2(x)
    taps = {"p3": x[0]}
    taps.update({"lm%d" % l: lv[l] for l in range(4)})

    def norm(t, n, m, swap=False):
        q = [mask_ref.blend(m, [getattr(s["norm"][n], f) for s in st]) for f in ("mean", "rstd", "lo", "hi")]
        lo, hi = (q[3], q[2]) if swap else (q[2], q[3])
        return np.minimum(hi, np.maximum(lo, (t - q[0]) * q[1])).astype(np.float32)

    def affine(t, sty, m, swap=False):
        mean, std = (mask_ref.blend(m, [s["sty"][sty][i] for s in st]) for i in (0, 1))
        return (t * mean + std if swap else t * std + mean).astype(np.float32)

    def apply(t, k, m):
        F = np.zeros(m.shape[1:] + (32, 32), np.float32)
        for s in range(S):
            F = F + m[s][..., None, None] * st[s]["filt"][k][None, None]
        return np.einsum("hwij,hwj->hwi", F.astype(np.float32), t[0]).astype(np.float32)[None]

    m3 = np.roll(lv[3], 1, axis=2) if defect == "level mask shifted by one pixel in x" else lv[3]
    raw = O.relu(O.conv3x3(x, w["Encoder.slice.19.weight"], w["Encoder.slice.19.bias"]))
    cur = norm(raw, 0, m3, swap=defect == "lo / hi exchanged")
    taps["c41"] = cur[0]
    for f in range(3):
        p = "Decoder.Filter%d." % (f + 1)
        wd, bd = w[p + "down_sample.0.weight"], w[p + "down_sample.0.bias"]
        n = 512 // MK_SPLIT
        part = [O.conv3x3(np.ascontiguousarray(cur[..., k * n:(k + 1) * n]), np.ascontiguousarray(wd[:, k * n:(k + 1) * n]), np.zeros_like(bd))
                for k in range(MK_SPLIT)]
        taps["dpart"] = np.concatenate(part, axis=-1)[0]
        d = part[0]
        for k in range(1, MK_SPLIT - (1 if defect == "one split-K slice dropped" else 0)):
            d = d + part[k]
        if defect != "bias of down_sample omitted":
            d = (d + bd).astype(np.float32)
        k1, k2 = (2 * f + 1, 2 * f) if defect == "F1 and F2 exchanged" else (2 * f, 2 * f + 1)
        d = apply(O.lrelu(d), k1, lv[3]) if defect == "LeakyReLU before F1" else O.lrelu(apply(d, k1, lv[3]))
        d = apply(d, k2, lv[3])
        cur = cur + O.conv3x3(d, w[p + "upsample.0.weight"], w[p + "upsample.0.bias"])
        taps["f%d" % (f + 1)] = cur[0]
    taps["d"] = d[0]
    cur = affine(norm(cur, 1, lv[3]), 3, lv[3], swap=defect == "AdaIN mean / std exchanged")
    taps["f3"] = cur[0]
    for blk, xin, xs, a, o, l in MR.MASK_BLOCKS[:2]:
        n1, n2, na, si = LR.RES[blk]
        m = lv[l]
        if defect == "level-1 mask from the neighbouring row pair" and l == 1:
            m = np.ascontiguousarray(m[:, np.arange(m.shape[1]) ^ 1])
        pre = "Decoder.%s." % blk
        taps[xs] = O.conv1x1(cur, w[pre + "conv_shortcut.weight"])[0]
        h = norm(O.lrelu(O.conv3x3(O.upsample2(cur), w[pre + "conv1.weight"], w[pre + "conv1.bias"])), n1, m)
        taps[a] = h[0]
        h = norm(O.lrelu(O.conv3x3(h, w[pre + "conv2.weight"], w[pre + "conv2.bias"])), n2, m)
        xsu = O.upsample2(taps[xs][None])
        if defect == "shortcut read at x instead of x >> 1" and l == 2:
            W2 = xsu.shape[2]
            xsu = np.repeat(taps[xs], 2, axis=0)[None][:, :, np.minimum(np.arange(W2), W2 // 2 - 1)]
        if defect == "shortcut added after the AdaIN affine" and l == 2:
            cur = (affine(norm(h, na, m), si, m) + xsu).astype(np.float32)
        else:
            cur = affine(norm((h + xsu).astype(np.float32), na, m), si, m)
        taps[o] = cur[0]
    return taps


@pytest.fixture(scope="module")
def mk(pkg, weights, oracle):
    prev = oracle.CONV_BACKEND
    oracle.set_conv_backend("numpy")
    try:
        blobs = [np.asarray(load_golden(n)["state"], np.float32) for n in MK_STATES]
        frame = pkg.synth_frame(1, 64, 80, kind="smooth")
        M = MR.softmax_mask(11, len(blobs), 64, 80)
        yield oracle, frame, blobs, M, [LR.parse_state(b) for b in blobs]
    finally:
        oracle.set_conv_backend(prev)


def _mask_failed(taps, weights, sts):
    out = MR.mask_checks(taps.__getitem__, weights, sts, CPU_FAM, MK_SPLIT, names=MK_NAMES)
    assert tuple(n for n, *_ in out) == MK_NAMES
    return {n: worst for n, _, ok, worst, _ in out if not ok}


def test_masked_float32_stand_in_passes(mk, weights):
    oracle, frame, blobs, M, sts = mk
    taps = _mask_standin(oracle, weights, frame, blobs, M)
    bad = _mask_failed(taps, weights, sts)
    assert not bad, bad
    # ... and with the convolution filtered in place (split 1: d composite from f2)
    out = MR.mask_checks(taps.__getitem__, weights, sts, CPU_FAM, 1, names=("dpart", "d"))
    assert [(n, ok) for n, _, ok, _, _ in out] == [("d", True)], out


MK_DEFECTS = {"level-1 mask from the neighbouring row pair": {"a3", "o3"}, "level mask shifted by one pixel in x": {"c41"},
              "shortcut read at x instead of x >> 1": {"o4"}, "styles blended in swapped order": {"c41"}, "F1 and F2 exchanged": {"d"},
              "bias of down_sample omitted": {"d"}, "LeakyReLU before F1": {"d"}, "one split-K slice dropped": {"d"},
              "lo / hi exchanged": {"c41"}, "AdaIN mean / std exchanged": {"f3"}, "shortcut added after the AdaIN affine": {"o4"}}


@pytest.mark.parametrize("defect", sorted(MK_DEFECTS))
def test_masked_injected_defect_fails(mk, weights, defect):
    """One wrong step planted in the float32 walk; the stage that sees it must fail at the committed K."""
    oracle, frame, blobs, M, sts = mk
    bad = _mask_failed(_mask_standin(oracle, weights, frame, blobs, M, defect=defect), weights, sts)
    assert set(bad) >= MK_DEFECTS[defect], "%s: only %s fail" % (defect, bad)


def test_level_mask_decoder(mk):
    """A level-mask tap decodes to the mask it was laid out from, and a non-zero float outside the w * S run of a row is refused."""
    M = mk[3]
    S = M.shape[0]
    for lv in mask_ref.level_masks(M):
        _, h, w = lv.shape
        t = np.zeros((h + 2, w + 2, MR.MASK_CH), np.float32)
        t.reshape(h + 2, -1)[1:h + 1, MR.MASK_CH:MR.MASK_CH + w * S] = lv.transpose(1, 2, 0).reshape(h, w * S)
        np.testing.assert_array_equal(MR.decode_level_mask(t.ravel(), h, w, S), lv)
        for y, off in ((0, 9), (h + 1, 9), (1, 0), (1, MR.MASK_CH + w * S), (h, (w + 2) * MR.MASK_CH - 1)):
            bad = t.copy()
            bad.reshape(h + 2, -1)[y, off] = 1e-30
            with pytest.raises(AssertionError, match="outside the w \\* S run"):
                MR.decode_level_mask(bad.ravel(), h, w, S)
    lv = mask_ref.level_masks(M)
    assert all(ok for _, _, ok, _, _ in MR.check_level_masks({"lm%d" % l: lv[l] for l in range(4)}.__getitem__, lv, S))
    off = [a.copy() for a in lv]
    off[2][1, 3, 4] = np.nextafter(off[2][1, 3, 4], np.float32(2))
    assert [ok for _, _, ok, _, _ in MR.check_level_masks({"lm%d" % l: off[l] for l in range(4)}.__getitem__, lv, S)] == [True, True, False, True]


# ---- the preparation pass: the references of tests/test_gpu_prep_layers.py ----------------------------------------------------

import prep_ref as PR            # noqa: E402

F32 = np.float32


def _lrelu_like(rng, n, C, spread=1.0):
    """[n, C] float32 shaped like a LeakyReLU output: channel means and scales of their own."""
    x = rng.standard_normal((n, C)) * rng.uniform(0.2, 3.0, C) * spread + rng.uniform(-1.0, 2.0, C)
    return np.where(x >= 0, x, 0.2 * x).astype(F32)


def _partials32(x, mean=None, keep=None):
    """chan_stat_k's two passes over the pixels `keep` of x [n, C]: the fp64 sum, or (fp64 sum of fp32 squares about the fp32
    mean, min, max)."""
    x = x if keep is None else x[keep]
    if mean is None:
        return x.astype(np.float64).sum(axis=0)
    d = (x - mean).astype(F32)
    return (d * d).astype(F32).astype(np.float64).sum(axis=0), x.min(axis=0), x.max(axis=0)


def _two_pass32(x, mode=1, keep=None, n_for_style=None):
    """chan_stat_k + chan_final_k (modes 1 and 2) in float32 numpy.  keep: the pixels the passes read (a defect: N stays)."""
    N = x.shape[0]
    mean = (_partials32(x, keep=keep) / N).astype(F32)
    q, mn, mx = _partials32(x, mean, keep)
    if mode == 2:
        var = (q / ((N - 1.0) if n_for_style is None else n_for_style)).astype(F32) + F32(1e-5)
        return mean.astype(np.float64), np.sqrt(var).astype(F32).astype(np.float64)
    r = (F32(1) / np.sqrt((q / N).astype(F32) + F32(1e-8))).astype(F32)
    return tuple(a.astype(np.float64) for a in (mean, r, ((mn - mean) * r).astype(F32), ((mx - mean) * r).astype(F32)))


def _merged32(groups, frame_px, cross=True, short=False):
    """chan_stats_group + chan_merge_k + chan_finish_k over groups of pixels [n_b, C] (whole frames of frame_px pixels).
    cross=False: the merge without d^2 n_a n_b / n; short: n_a one frame short."""
    acc, n_a = None, 0.0
    for g in groups:
        n_b = float(g.shape[0])
        m32 = (_partials32(g) / n_b).astype(F32)
        q, mn, mx = _partials32(g, m32)
        mean_b = _partials32(g) / n_b
        e = mean_b - m32.astype(np.float64)
        M2_b = np.maximum(q - n_b * e * e, 0.0)
        if acc is None:
            acc = [mean_b, M2_b, mn.astype(np.float64), mx.astype(np.float64)]
        else:
            na = n_a - (frame_px if short else 0.0)
            n, d = na + n_b, mean_b - acc[0]
            acc[0] = acc[0] + d * (n_b / n)
            acc[1] = acc[1] + M2_b + (d * d * (na * n_b / n) if cross else 0.0)
            acc[2], acc[3] = np.minimum(acc[2], mn), np.maximum(acc[3], mx)
        n_a += n_b
    m = acc[0].astype(F32)
    r = (F32(1) / np.sqrt((acc[1] / n_a).astype(F32) + F32(1e-8))).astype(F32)
    return tuple(a.astype(np.float64) for a in (m, r, ((acc[2].astype(F32) - m) * r).astype(F32), ((acc[3].astype(F32) - m) * r).astype(F32)))


def _fc32(w, name, t, smean):
    """chan_stat_k's mean (mode 0) of t [n, 32] + fc_filter_k in float32."""
    p = "Decoder.%s.FC." % name
    vec = np.concatenate([(t.astype(np.float64).sum(axis=0) / t.shape[0]).astype(F32), np.asarray(smean, F32)])
    return (w[p + "weight"].astype(F32) @ vec + w[p + "bias"].astype(F32)).astype(F32).reshape(32, 32)


def test_prep_statistic_stand_ins_pass():
    rng = np.random.default_rng(5)
    for n in (1, 6, 254, 19008):
        x = _lrelu_like(rng, n, 16)
        ok, worst, ratio = PR.check_pstat(_two_pass32(x), PR.raw_stats(x), LR.K["pstat"])
        assert ok, "two-pass statistic over %d pixels at %.2f of its bound (ratio %.2f)" % (n, worst, ratio)
        if n > 1:
            ok, worst, ratio = PR.check_pstat_style(_two_pass32(x, mode=2), PR.raw_stats(x), LR.K["pstat"])
            assert ok, "style statistic over %d pixels at %.2f of its bound (ratio %.2f)" % (n, worst, ratio)
    frames = [_lrelu_like(rng, 35, 16) + F32(0.3 * i) for i in range(5)]      # real mean differences between the groups
    for sizes in ((1, 1, 1, 1, 1), (2, 2, 1), (3, 2), (5,)):
        groups, i = [], 0
        for k in sizes:
            groups.append(np.concatenate(frames[i:i + k]))
            i += k
        ok, worst, ratio = PR.check_pstat(_merged32(groups, 35), PR.raw_stats(np.concatenate(frames)), LR.K["pstat"])
        assert ok, "merged statistic over groups %s at %.2f of its bound (ratio %.2f)" % (sizes, worst, ratio)


def test_prep_mean_and_fc_stand_in_passes_and_a_foreign_style_half_fails(weights):
    rng = np.random.default_rng(6)
    t = (rng.standard_normal((425, 32)) * 2.0 + rng.uniform(-1, 1, 32)).astype(F32)
    smean = rng.standard_normal((6, 32)).astype(F32)
    t64 = t.astype(np.float64)
    for i, name in enumerate(LR.FILTER_NAMES):
        ok, worst, ratio = PR.check_pred(_fc32(weights, name, t, smean[i]), weights, name, t64.mean(axis=0), np.abs(t64).mean(axis=0), smean[i], LR.K["ppred"])
        assert ok, "%s stand-in at %.2f of its bound (ratio %.2f)" % (name, worst, ratio)
        ok, worst, _ = PR.check_pred(_fc32(weights, name, t, smean[(i + 2) % 6]), weights, name, t64.mean(axis=0), np.abs(t64).mean(axis=0), smean[i],
                                     LR.K["ppred"])
        assert not ok, "%s with another filter's style half passes (worst %.2f)" % (name, worst)


def test_prep_statistic_defects_fail():
    rng = np.random.default_rng(7)
    K = LR.K["pstat"]
    x = _lrelu_like(rng, 270400, 4)
    rs = PR.raw_stats(x)
    assert PR.check_pstat(_two_pass32(x), rs, K)[0]
    keep = np.ones(x.shape[0], bool)
    keep[int(np.argmax(x[:, 0]))] = False
    assert not PR.check_pstat(_two_pass32(x, keep=keep), rs, K)[0], "the maximum pixel left out passes"
    # ... and a pixel that holds no extremum: the mean and the variance alone must see it
    inner = int(np.argsort(x[:, 0])[x.shape[0] // 2])
    keep = np.ones(x.shape[0], bool)
    keep[inner] = False
    assert not PR.check_pstat(_two_pass32(x, keep=keep), rs, K)[0], "one median pixel left out passes"
    nblk = 1024
    tail = x.shape[0] - nblk * (x.shape[0] // nblk)
    assert tail == 64
    keep = np.ones(x.shape[0], bool)
    keep[-tail:] = False
    assert not PR.check_pstat(_two_pass32(x, keep=keep), rs, K)[0], "the last block's tail left out passes"
    for n in (6, 4096):
        y = _lrelu_like(rng, n, 16)
        assert PR.check_pstat_style(_two_pass32(y, mode=2), PR.raw_stats(y), K)[0]
        assert not PR.check_pstat_style(_two_pass32(y, mode=2, n_for_style=float(n)), PR.raw_stats(y), K)[0], "N instead of N - 1 at N = %d passes" % n
    frames = [_lrelu_like(rng, 35, 16) + F32(0.3 * i) for i in range(5)]
    groups = [np.concatenate(frames[0:2]), np.concatenate(frames[2:4]), frames[4]]
    rs = PR.raw_stats(np.concatenate(frames))
    assert PR.check_pstat(_merged32(groups, 35), rs, K)[0]
    assert not PR.check_pstat(_merged32(groups, 35, cross=False), rs, K)[0], "a merge without the cross term passes"
    assert not PR.check_pstat(_merged32(groups, 35, short=True), rs, K)[0], "n_a one frame short passes"


class _FakeRun:
    def __init__(self, taps, st, B):
        self.taps, self.st, self.B = taps, st, B

    def get(self, name, b=0):
        return self.taps[name][b]


def _filter_stage32(oracle, w, content, sty, smean, own_residual=False):
    """Stops 0 and 1 of the resident pass on content [B, h, w, 512] in the oracle's float32 arithmetic, as the kernels run it."""
    O = oracle
    B = content.shape[0]
    st = _empty_state(sty)
    st["norm"][0] = _two_pass32(content.reshape(-1, 512))
    mean, rstd = (a.astype(F32) for a in st["norm"][0][:2])
    cn = ((content - mean) * rstd).astype(F32)
    t32 = None
    for g in (1, 2):
        p = "Decoder.Filter1.F%d." % g
        t32 = O.conv3x3(cn, w[p + "down_sample.0.weight"], w[p + "down_sample.0.bias"])
        st["filt"]["Filter1.F%d" % g] = _fc32(w, "Filter1.F%d" % g, t32.reshape(-1, 32), smean[g - 1]).astype(np.float64)
    F1, F2 = (st["filt"]["Filter1.F%d" % g].astype(F32) for g in (1, 2))
    p = "Decoder.Filter1."
    d, u = [], []
    for b in range(B):
        d.append(O.lrelu(O.apply_filter(O.conv3x3(cn[b:b + 1], w[p + "down_sample.0.weight"], w[p + "down_sample.0.bias"]), F1)))
        u.append(O.conv3x3(O.apply_filter(d[b], F2), w[p + "upsample.0.weight"], w[p + "upsample.0.bias"])[0])
    nxt = np.stack([cn[b] + u[b if own_residual else 0] for b in range(B)]).astype(F32)
    taps = {"content": content, "cn": cn, "t32": t32, "d32": d[0], "u": u[0][None], "nxt": nxt}
    return _FakeRun(taps, st, B)


def test_prep_filter_stage_stand_in_passes_and_own_residuals_fail(pkg, weights, oracle):
    """The stage functions themselves on a float32 stand-in of stops 0 and 1 (two images, 4 x 5 features), and quirk Q1: every
    image given its own residual instead of frame 0's fails on image 1."""
    prev = oracle.CONV_BACKEND
    oracle.set_conv_backend("numpy")
    try:
        _, sty, smean = _style(oracle, pkg, weights)
        rng = np.random.default_rng(8)
        content = np.maximum(rng.standard_normal((2, 4, 5, 512)) + 0.3, 0).astype(F32) * rng.uniform(0.1, 2.0, 512).astype(F32)
        # (the oracle's float32 numpy convolutions stand in for every kernel family at the direct family's K, as above)
        k = dict(LR.K, f23=LR.K["direct"], gemm=LR.K["direct"])
        c = PR.Ctx(weights, smean, (0, 1), k=k)
        run = _filter_stage32(oracle, weights, content, sty, smean)
        res = PR.STAGES[0](run, None, c) + PR.STAGES[1](run, None, c)
        bad = {n: worst for n, _, ok, worst, _ in res if not ok}
        assert not bad, bad
        assert {n for n, *_ in res} >= {"norm0", "cn[1]", "t32[1]", "Filter1.F1", "Filter1.F2", "d32", "u", "nxt[0]", "nxt[1]"}
        run = _filter_stage32(oracle, weights, content, sty, smean, own_residual=True)
        bad = {n for n, _, ok, _, _ in PR.STAGES[1](run, None, c) if not ok}
        assert bad == {"nxt[1]"}, bad
    finally:
        oracle.set_conv_backend(prev)


def test_prep_blob_entries_and_bit_equality():
    seen = [e for s in range(PR.N_STOPS) for e in PR.stage_entries(s)]
    assert sorted(seen) == sorted([("norm", i) for i in range(11)] + [("filt", i) for i in range(6)]) and len(PR.STAGES) == 14
    assert sum(n for _, n in PR.OFFSETS.values()) == 17536
    a = np.arange(17536, dtype=F32)
    b = a.copy()
    o, _ = PR.OFFSETS["norm", 1]          # written at stop 4
    b[o + 3] = np.nextafter(b[o + 3], F32(0))
    assert PR.entries_bit_equal(a, b, 4) and not PR.entries_bit_equal(a, b, 5)


# ---- the windows of the pad / crop entries: LR.crop_windows against the window rule, and the rule's negative controls -----------------

def test_padded_size_is_the_oracles(oracle):
    assert [LR.padded_size(n) for n in range(1, 700)] == [oracle.padded_size(n) for n in range(1, 700)]


@pytest.mark.parametrize("conv2_f43", [False, True], ids=["f23", "f43"])
def test_crop_windows_suffice_for_every_source_size(conv2_f43):
    """H, W in 1..256: every o2 element conv_last reads for a crop pixel lies in wo or outside the frame, every a2 element conv2 reads for
    a wo pixel in the written a2 window or outside the frame, every xs2 element of the upsampled residual in the halved window
    (LR.window_faults: conditions on index arithmetic, no exception), and the windows have the alignment their kernels' items need."""
    for H in range(1, 257):
        for W in range(1, 257):
            w = LR.crop_windows(H, W, conv2_f43)
            assert LR.window_faults(w) == [], (H, W, w)
            assert not any(v & 15 for v in w["wl"] + w["wo"]) and not any(v & 31 for v in w["wa"]) and not any(v & 15 for v in w["xs"]), (H, W, w)
            assert not conv2_f43 or not any(v & 31 for v in w["wo"]), (H, W, w)
            for n in ("wl", "wo", "wa"):
                assert LR.inside(w[n], (0, 0, w["PH"], w["PW"])), (H, W, n, w)      # (a padded size is a multiple of 64: no round-out leaves it)
            assert LR.inside(w["crop"], LR.pre_checkable(w)), (H, W, w)


def test_tightest_window_is_one_row_behind_the_crop():
    """(64 + H) = 15 (mod 16): the crop's last row reads o2 row 64 + H, and wo (the 16-aligned form) ends exactly there, one row behind the
    crop, with wl; one row less and conv_last would read a stale row."""
    tight = [H for H in range(1, 257) if (LR.CROP0 + H) % 16 == 15]
    assert tight[:3] == [15, 31, 47] and len(tight) == 16
    for H in tight:
        w = LR.crop_windows(H, H, False)
        assert w["wo"][2] == w["wo"][3] == LR.CROP0 + H + 1 == w["wl"][2]
        assert LR.window_faults(w) == []
        for side in (2, 3):
            v = list(w["wo"])
            v[side] -= 1
            assert LR.window_faults(dict(w, wo=tuple(v))) == ["last: reads o2 outside wo"]
        # the rows of wl behind the crop have no reference: their taps reach past wo
        assert LR.pre_checkable(w)[2:] == (LR.CROP0 + H, LR.CROP0 + H)
    for H in range(1, 257):         # nowhere else is wo that tight on the far side
        if H not in tight:
            assert LR.crop_windows(H, H, False)["wo"][2] > LR.CROP0 + H + 1


# One source size per window form, both padded to 192 x 192.  16-aligned wo: crop ends 79 = 15 (mod 16) on both axes, the tight end, where wo ends
# at 80 = 16 (mod 32) and every strip of all three windows is read.  32-aligned wo: 79 on y and 127 = 31 (mod 32) on x, the one residue at which
# the far wa strip reaches the crop.
WIN_SRC = {False: (15, 15), True: (15, 63)}
SHRINKS = [(n, side) for n in ("wo", "wa", "xs") for side in range(4)]


def _cone(w):
    """What a crop pixel depends on, by index arithmetic: the o2, a2 and xs2 elements inside the frame."""
    PH, PW = w["PH"], w["PW"]
    o2 = LR.reads3(w["crop"], PH, PW)
    return {"wo": o2, "wa": LR.reads3(o2, PH, PW), "xs": LR.reads_half(o2, PH, PW)}


def _meet(a, b):
    return max(a[0], b[0]) < min(a[2], b[2]) and max(a[1], b[1]) < min(a[3], b[3])


def _strip(win, side, tile):
    """What shrink(win, side, tile) takes off."""
    v = list(win)
    if side < 2:
        v[side + 2] = win[side] + tile
    else:
        v[side - 2] = win[side] - tile
    return tuple(v)


@pytest.fixture(scope="module")
def window_decode(weights):
    """The float64 decoder stages behind o3 at 192 x 192 (slice2.conv1 + shortcut, slice2.conv2, conv_last) for the source sizes of WIN_SRC: frame A
    is what the call stylizes, every tensor holds frame B's values (an unrelated o3 through the same stages; noise on the rows no window
    reaches) wherever the windowed evaluation does not write.  Every evaluation runs the stage on the same rows at the full width and then
    keeps the window, so two evaluations whose inputs agree on what a value reads give that value bit for bit."""
    st = LR.parse_state(load_golden("global_a")["state"])
    rng = np.random.default_rng(77)
    P = 192
    assert {LR.padded_size(n) for hw in WIN_SRC.values() for n in hw} == {P}
    ROWS = 128          # a2 rows evaluated: no window of either form goes further down (asserted below)
    full, stale = {}, {}
    for who, seed in ((full, 1), (stale, 2)):
        o3 = np.random.default_rng(seed).standard_normal((P // 2, P // 2, 128))
        a2 = rng.standard_normal((P, P, 64))
        a2[:ROWS] = LR.STAGES["a2"][2]([o3], weights, st, 0, ROWS)[0]
        who["a2"], who["xs2"] = a2, LR.STAGES["xs2"][2]([o3], weights, st, 0, P // 2)[0]
    stale["o2"] = rng.standard_normal((P, P, 64))

    def paste(dst, src, win):
        y0, x0, y1, x1 = LR.clip(win, *dst.shape[:2])
        out = dst.copy()
        out[y0:y1, x0:x1] = src[y0:y1, x0:x1]
        return out

    def run(w, base):
        """(crop, o2 on the unshrunk wo) of frame A evaluated through the windows w; base: the unshrunk windows (they fix the rows evaluated)."""
        assert base["wa"][2] <= ROWS
        y0, _, y1, _ = base["wo"]
        a2 = paste(stale["a2"], full["a2"], w["wa"])
        xs = paste(stale["xs2"], full["xs2"], w["xs"])
        v = np.zeros((P, P, 64))
        v[y0:y1] = LR.STAGES["o2"][2]([a2, xs], weights, st, y0, y1)[0]
        o2 = paste(stale["o2"], v, w["wo"])
        cy0, cx0, cy1, cx1 = base["crop"]
        pre = LR.STAGES["pre"][2]([o2], weights, st, cy0, cy1)[0][:, cx0:cx1]
        by0, bx0, by1, bx1 = base["wo"]
        return pre, o2[by0:by1, bx0:bx1]

    return run


@pytest.mark.parametrize("conv2_f43", [False, True], ids=["f23", "f43"])
def test_windows_are_necessary_on_the_float64_decoder(window_decode, conv2_f43):
    """The crop evaluated through the windows of LR.crop_windows from tensors that hold another frame's values everywhere else equals the
    evaluation through windows that cover everything, exactly.  Then each of wo, wa and the shortcut window one tile short on one side (16;
    32 for the fused conv1's items and for wo where conv2 runs on conv_f43_k; 16 half-resolution pixels for xs2):
      - window_faults names the broken condition and o2 inside wo changes, exactly where index arithmetic says a wo pixel (for wo: a crop
        pixel) reads the strip taken off;
      - the CROP changes exactly where index arithmetic says a crop pixel depends on that strip (_cone).
    16-aligned wo, 15 x 15: all twelve strips break a condition and all twelve change the crop.
    32-aligned wo, 15 x 63: the wo and wa strips break their conditions, the xs2 strips do not, at this or ANY size.  wo starts at 32, so wa
    starts at 0 and xs2 at 0, and the near xs2 strip 0..15 ends where wo's first row reads (32 // 2); wo ends on a multiple of 32, so wa ends
    32 further, xs2 16 further, and the far xs2 strip starts at wo's end halved, one row behind the last one read.  The fused kernel writes
    its shortcut for whole 32 x 32 items, a tile more than conv2 reads on each side: larger than needed, not smaller, which is the side the
    GPU suite pins by comparing what was written.  Of the strips that break a condition, the crop sees both wo strips per axis and the far wa
    strip on x: the near wa strip 0..31 ends 30 rows before a2 row 62 = 64 - 2, the first a crop pixel depends on, at every size, and the far
    one starts at wo's end, which the crop's last a2 row 64 + n + 1 reaches only for 64 + n = 31 (mod 32), as on x here."""
    base = LR.crop_windows(*WIN_SRC[conv2_f43], conv2_f43)
    PH, PW = base["PH"], base["PW"]
    everything = dict(base, wo=(0, 0, PH, PW), wa=(0, 0, PH, PW), xs=(0, 0, PH // 2, PW // 2))
    ref_crop, ref_o2 = window_decode(everything, base)
    crop, o2 = window_decode(base, base)
    assert np.array_equal(crop, ref_crop) and np.array_equal(o2, ref_o2)
    assert LR.window_faults(base) == []
    cone = _cone(base)
    wo_in = LR.clip(base["wo"], PH, PW)
    needed = {"wo": cone["wo"], "wa": LR.reads3(wo_in, PH, PW), "xs": LR.reads_half(wo_in, PH, PW)}
    tiles = {"wo": 32 if conv2_f43 else 16, "wa": 32, "xs": 16}
    want = {"wo": "last: reads o2 outside wo", "wa": "conv2: reads a2 outside wa", "xs": "res: reads xs2 outside its window"}
    broke, seen = set(), set()
    for name, side in SHRINKS:
        w = dict(base)
        w[name] = LR.shrink(base[name], side, tiles[name])
        strip = _strip(base[name], side, tiles[name])
        breaks, visible = _meet(strip, needed[name]), _meet(strip, cone[name])
        assert (want[name] in LR.window_faults(w)) == breaks, (name, side, LR.window_faults(w))
        crop, o2 = window_decode(w, base)
        assert np.array_equal(o2, ref_o2) != breaks, (name, side, breaks)
        assert np.array_equal(crop, ref_crop) != visible, (name, side, visible)
        broke |= {(name, side)} if breaks else set()
        seen |= {(name, side)} if visible else set()
    if conv2_f43:
        assert broke == {s for s in SHRINKS if s[0] != "xs"}, broke
        assert seen == {("wo", 0), ("wo", 1), ("wo", 2), ("wo", 3), ("wa", 3)}, seen
    else:
        assert broke == seen == set(SHRINKS), (broke, seen)

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


def test_k_within_four_times_the_measured_maximum():
    for f in LR.FAMILIES:
        assert LR.MEASURED[f] <= LR.K[f] <= 4 * LR.MEASURED[f], f

"""The checkers of tests/test_gpu_packs.py checked on the CPU: numpy stand-ins built from tests/pack_ref.py in the arithmetic each pack
kernel promises (float32 where the kernel is float32, one rounding of an extended-precision value where it promises that) must pass, and
each defect a GPU pack test is there to catch must fail the same check_buffer / check_fold."""
import numpy as np
import pytest

import layer_ref as LR
import pack_ref as P
from state_bounds import load_golden

F43_KEY, WINO_KEY, UPS_KEY, SC_KEY = "Encoder.slice.2", "Encoder.slice.5", "Decoder.slice2.conv1", "Decoder.slice2.conv_shortcut"


def _raw(w, key):
    return w[key + ".weight"]


def _wino32(raw, G=P.G23, negate=True):
    """pack_wino_k's stand-in: both stages of U = G g G^T in float32."""
    return P.slab16(P.transform(raw, G, np.float32)[0], negate=negate)


def _f43(raw, dtype=np.longdouble):
    return P.slab_f43(P.transform(raw, P.g43(dtype), dtype)[0]).astype(np.float32)


def _ups_sc(raw, sc, scale=0.25):
    u = P.transform(raw, P.GUPS5, np.longdouble)[0]
    blk = (np.asarray(sc, np.float32).reshape(u.shape[0], u.shape[1], 1) * np.float32(scale)).astype(np.longdouble)
    return P.slab16(np.concatenate([u, blk], axis=2)).astype(np.float32)


def _grey32(raw, bias):
    """pack_first_grey_k's stand-in: float32 throughout, terms in the kernel's order."""
    mean, sd = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    w = np.asarray(raw, np.float32).reshape(64, 3, 9)
    w1, w0, b = np.zeros((9, 64), np.float32), np.zeros((9, 64), np.float32), np.asarray(bias, np.float32).copy()
    for c in range(3):
        w1 = w1 + w[:, c, :].T / sd[c]
        w0 = w0 - w[:, c, :].T * (mean[c] / sd[c])
    for tap in range(9):
        for c in range(3):
            b = b - w[:, c, tap] * (mean[c] / sd[c])
    return np.concatenate([w1.reshape(-1), w0.reshape(-1), b]).astype(np.float32)


def _fold32(F, w2, left):
    """fold_down_k (left: F . W) / fold_up_k (W . F over the middle axis)'s stand-in: a 32-term float32 sum in index order."""
    F = np.asarray(F, np.float32).reshape(32, 32)
    if left:
        w2 = np.asarray(w2, np.float32).reshape(32, -1)
        s = np.zeros((32, w2.shape[1]), np.float32)
        for m in range(32):
            s = s + F[:, m, None] * w2[None, m, :]
        return s.reshape(-1)
    w3 = np.asarray(w2, np.float32).reshape(-1, 32, 9)
    s = np.zeros((w3.shape[0], 32, 9), np.float32)
    for m in range(32):
        s = s + w3[:, m, None, :] * F[None, m, :, None]
    return s.reshape(-1)


def _filters(name, f):
    st = LR.parse_state(load_golden(name)["state"])
    return st["filt"]["Filter%d.F1" % (f + 1)], st["filt"]["Filter%d.F2" % (f + 1)]


def _fold_standins(w, F1, F2, f=0):
    p = "Decoder.Filter%d." % (f + 1)
    down = _fold32(F1, w[p + "down_sample.0.weight"], True)
    bias = np.zeros(256, np.float32)
    bias[:32] = _fold32(F1, np.asarray(w[p + "down_sample.0.bias"]).reshape(32, 1), True)
    up = _fold32(F2, w[p + "upsample.0.weight"], False)
    return down, bias, up


def test_stand_ins_pass(weights):
    w = weights
    cases = [("Encoder.slice.0", "first", P.first(_raw(w, "Encoder.slice.0"))),
             ("Encoder.slice.0", "first_grey", _grey32(_raw(w, "Encoder.slice.0"), w["Encoder.slice.0.bias"])),
             ("Decoder.slice1", "last", P.last(_raw(w, "Decoder.slice1"))),
             ("Decoder.slice1", "bias", np.concatenate([w["Decoder.slice1.bias"], np.zeros(1, np.float32)])),
             (SC_KEY, "bias", np.zeros(64, np.float32)),
             (SC_KEY, "pk", P.pk(_raw(w, SC_KEY), 64)),
             (WINO_KEY, "pk", P.pk(_raw(w, WINO_KEY), 128)),
             ("Decoder.Filter1.F1.down_sample.0", "pk", P.pk(_raw(w, "Decoder.Filter1.F1.down_sample.0"), 32)),
             (WINO_KEY, "raw", _raw(w, WINO_KEY)),
             (WINO_KEY, "pk_wino", _wino32(_raw(w, WINO_KEY))),
             (UPS_KEY, "pk_ups", _wino32(_raw(w, UPS_KEY), P.GUPS9)),
             (UPS_KEY, "pk_ups_sc", _ups_sc(_raw(w, UPS_KEY), _raw(w, SC_KEY))),
             (F43_KEY, "pk_f43", _f43(_raw(w, F43_KEY)))]
    for key, form, got in cases:
        ok, fig, fam = P.check_buffer(key, form, got, w, kgrey=LR.K["grey"])
        assert ok, "%s %s stand-in (%s): %.6g" % (key, form, fam, fig)
    # a float64 evaluation in another order (numpy's einsum) still rounds to the same float32 but for the 2^-20 ulp the bound allows
    g = np.asarray(_raw(w, F43_KEY), np.float64)
    G = P.g43(np.float64)
    u64 = np.einsum("pk,oikl,ql->oipq", G, g, G).reshape(g.shape[0], g.shape[1], 36)
    ok, fig, _ = P.check_buffer(F43_KEY, "pk_f43", P.slab_f43(u64).astype(np.float32), w)
    assert ok, fig


def test_fold_stand_ins_pass(weights):
    for name in ("global_a", "global_b"):
        F1, F2 = _filters(name, 0)
        down, bias, up = _fold_standins(weights, F1, F2)
        for kind, form, got, F in (("down", "raw", down, F1), ("down", "bias", bias, F1), ("up", "raw", up, F2)):
            ok, fig, _ = P.check_fold(kind, form, got, F, weights, 0)
            assert ok, "%s %s on %s: ratio %.3g" % (kind, form, name, fig)
        for kind, raw, shape in (("down", down, (32, 512, 3, 3)), ("up", up, (512, 32, 3, 3))):
            ok, fig, _ = P.check_fold(kind, "pk_wino", _wino32(raw.reshape(shape)), None, weights, 0, got_raw=raw)
            assert ok, "%s pk_wino on %s: ratio %.3g" % (kind, name, fig)


def _swap_channels(raw, a=5, b=6):
    r = np.array(raw, copy=True)
    r[:, [a, b]] = r[:, [b, a]]
    return r


def _pack_defects(w):
    """{defect: (key, form, the defective buffer)}"""
    f43, wino, ups, sc = (_raw(w, k) for k in (F43_KEY, WINO_KEY, UPS_KEY, SC_KEY))
    out = {"F(4x4) U in float32": (F43_KEY, "pk_f43", _f43(f43, np.float32)),
           "F(2x2) swizzle without the negation": (WINO_KEY, "pk_wino", _wino32(wino, negate=False)),
           "five-product swizzle without the negation": (UPS_KEY, "pk_ups_sc", P.slab16(
               np.concatenate([P.transform(ups, P.GUPS5)[0], np.asarray(sc, np.float64).reshape(64, 128, 1) / 4], axis=2), negate=False).astype(np.float32)),
           "direct-form swizzle negated": (WINO_KEY, "pk", P.slab16(np.asarray(wino).reshape(128, 64, 9), 128, negate=True)),
           "two channels of a chunk exchanged, pk": (WINO_KEY, "pk", P.pk(_swap_channels(wino), 128)),
           "two channels of a chunk exchanged, pk_wino": (WINO_KEY, "pk_wino", _wino32(_swap_channels(wino))),
           "two channels of a chunk exchanged, pk_f43": (F43_KEY, "pk_f43", _f43(_swap_channels(f43))),
           "shortcut block not scaled": (UPS_KEY, "pk_ups_sc", _ups_sc(ups, sc, scale=1.0)),
           "G row 2 of F(2x2) with the wrong sign": (WINO_KEY, "pk_wino", _wino32(wino, P.G23 * np.array([1, 1, -1, 1.0])[:, None])),
           "nine-product G on an F(2x2) buffer's rows": (UPS_KEY, "pk_ups", _wino32(ups, P.GUPS9[[1, 0, 2]])),
           "first: taps and colours transposed": ("Encoder.slice.0", "first", np.ascontiguousarray(
               np.asarray(_raw(w, "Encoder.slice.0")).reshape(64, 3, 9).transpose(1, 2, 0)).reshape(-1)),
           "last: row 27 not zero": ("Decoder.slice1", "last", None),
           "grey fold: bias without the sum of W0": ("Encoder.slice.0", "first_grey", None)}
    good = _f43(f43).reshape(2, 8, 36, 16, 4, 2, 2).copy()
    good[:, :, :, 3] = good[:, :, :, 3, :, ::-1].copy()
    out["the two cout blocks of an F(4x4) row exchanged"] = (F43_KEY, "pk_f43", good.reshape(-1))
    la = P.last(_raw(w, "Decoder.slice1")).copy().reshape(2, 4, 64, 4)
    la[1, 0, 11, 0] = la[0, 0, 11, 0]                                   # n = 16 + 11 = 27
    out["last: row 27 not zero"] = ("Decoder.slice1", "last", la.reshape(-1))
    gr = _grey32(_raw(w, "Encoder.slice.0"), w["Encoder.slice.0.bias"]).copy()
    gr[1152:] = w["Encoder.slice.0.bias"]
    out["grey fold: bias without the sum of W0"] = ("Encoder.slice.0", "first_grey", gr)
    return out


PACK_DEFECTS = ("F(4x4) U in float32", "F(2x2) swizzle without the negation", "five-product swizzle without the negation", "direct-form swizzle negated",
                "two channels of a chunk exchanged, pk", "two channels of a chunk exchanged, pk_wino", "two channels of a chunk exchanged, pk_f43",
                "the two cout blocks of an F(4x4) row exchanged", "shortcut block not scaled", "G row 2 of F(2x2) with the wrong sign",
                "nine-product G on an F(2x2) buffer's rows", "first: taps and colours transposed", "last: row 27 not zero",
                "grey fold: bias without the sum of W0")


@pytest.fixture(scope="module")
def pack_defects(weights):
    d = _pack_defects(weights)
    assert set(d) == set(PACK_DEFECTS)
    return d


@pytest.mark.parametrize("defect", PACK_DEFECTS)
def test_injected_pack_defect_fails(weights, pack_defects, defect):
    key, form, got = pack_defects[defect]
    ok, fig, fam = P.check_buffer(key, form, got, weights, kgrey=LR.K["grey"])
    assert not ok, "%s passes %s %s (%s: %.6g)" % (defect, key, form, fam, fig)


def test_float32_f43_misses_correct_rounding_on_half_the_values(weights):
    """The figure the rounded-once bound is there for: a float32 evaluation of the F(4x4) transform is correctly rounded on about half of the values only."""
    got = _f43(_raw(weights, F43_KEY), np.float32)
    u = P.pk_f43(_raw(weights, F43_KEY))
    miss = float(np.mean(np.abs(got.astype(np.longdouble) - u).astype(np.float64) > P.ONCE * P.ulp32(u)))
    assert 0.3 < miss < 0.7, miss


FOLD_DEFECTS = ("F transposed, down", "F transposed, down bias", "F transposed, up", "set 1 folded with set 0's F, down", "set 1 folded with set 0's F, up",
                "a non-zero float in bias slots 32..255", "pk_wino of another set's folded weights")


@pytest.mark.parametrize("defect", FOLD_DEFECTS)
def test_injected_fold_defect_fails(weights, defect):
    F1, F2 = _filters("global_a", 0)
    G1, G2 = _filters("global_b", 0)           # "set 1"
    if defect.startswith("F transposed"):
        down, bias, up = _fold_standins(weights, F1.T, F2.T)
        kind, form, got, F = {"down": ("down", "raw", down, F1), "down bias": ("down", "bias", bias, F1), "up": ("up", "raw", up, F2)}[defect.split(", ")[1]]
        ok, fig, _ = P.check_fold(kind, form, got, F, weights, 0)
    elif defect.startswith("set 1"):
        down, _, up = _fold_standins(weights, F1, F2)
        ok, fig, _ = P.check_fold("down", "raw", down, G1, weights, 0) if defect.endswith("down") else P.check_fold("up", "raw", up, G2, weights, 0)
    elif defect.startswith("a non-zero"):
        _, bias, _ = _fold_standins(weights, F1, F2)
        assert P.check_fold("down", "bias", bias, F1, weights, 0)[0]
        bias[200] = np.float32(1e-30)
        ok, fig, _ = P.check_fold("down", "bias", bias, F1, weights, 0)
    else:
        down, _, _ = _fold_standins(weights, F1, F2)
        other, _, _ = _fold_standins(weights, G1, G2)
        ok, fig, _ = P.check_fold("down", "pk_wino", _wino32(down.reshape(32, 512, 3, 3)), None, weights, 0, got_raw=other)
    assert not ok, "%s passes (figure %.4g)" % (defect, fig)


def test_expected_buffers_follow_the_weight_table(pkg):
    """Every convolution of the checkpoint has its raw weights among the expected buffers, conv1_1 and Decoder.slice1 (freed after packing) their packs."""
    keys = {k[:-len(".weight")] for k in pkg.weight_table() if k.endswith(".weight") and ".FC." not in k}
    raws = {k for k, f in P.expected_buffers() if f == "raw" and ".fold_" not in k}
    assert keys - raws == {"Encoder.slice.0", "EncoderStyle.slice1.0", "Decoder.slice1"}, sorted(keys ^ raws)
    assert raws <= keys
    assert len(P.expected_buffers()) == len(set(P.expected_buffers()))

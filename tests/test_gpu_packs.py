"""Every weight buffer the handle holds, read back (rrv_debug_copy_weights) and held to a reference of its own (tests/pack_ref.py): the
pack and fold kernels on dense Gaussian weights where every value is distinct, so a weight in the wrong place, a wrong swizzle or a
transform in the wrong precision shows whether or not an activation ever meets it.  One handle for the module; one case per buffer
the library enumerates, and the enumeration must be exactly the cases.

  bit for bit   raw, bias, pk (pack_conv_k at BN 32 / 64 / 128), first (pack_first_k), last (pack_last_k with its zero rows 27..31)
  rounded once  pk_f43 (pack_f43_k), pk_ups_sc (pack_ups5_k; the shortcut block is w / 4, exact): |got - U| <= (1/2 + 2^-20) ulp32(U), U
                in extended precision; the 2^-20 covers the order of the kernel's float64 evaluation
  float32       |got - ref64| <= n 2^-24 m with n the float32 roundings on an element's path and m the same arithmetic on absolute values:
    pk_wino, pk_ups (pack_wino_k)   U = G (g G^T) in two stages.  The widest row of either G sums three terms: two additions, two
                roundings (the factor 1/2 of F(2x2) is exact), each at most 2^-24 of a partial sum that m's row bounds; the second
                stage's two roundings act on values within (1 + 2^-23) of the first stage's magnitudes.  n = 4.
    first_grey (pack_first_grey_k)  against float64 arithmetic on the float32 constants widened:
                W1 = sum_c w_c / sd_c: one division per term and two additions (0 + x is exact): n = 3.
                W0 = -sum_c w_c (mean_c / sd_c): the float32 quotient and the product, one rounding each per term, and two
                subtractions: n = 4.
                bias - sum over the 27 (tap, c) terms: quotient and product per term (2) and 27 subtractions, each rounding a partial
                sum that m bounds: n = 29.
  folds         fold_down_k / fold_up_k teacher-forced on the state set's own filter and the checkpoint's weights: a 32-term float32 sum,
                |got - ref64| <= 32 2^-24 sum |F||W| + 2^-24 |ref|; the folded bias's floats 32..255 exactly 0; the folded pk_wino against
                the F(2x2) reference of the set's own folded raw.  Set 0 after set_state(global_a), again after set_state(global_b) (the
                second fold replaces the first), and the three sets of a grouped multi-style launch (blockIdx.y strides, the set-major
                pack), where image 1 on image 0's filter must fail.
Each n above is the cap of its family; layer_ref.K carries the family's K under that cap (pack32, grey, fold) and `once` in ulps."""
import numpy as np
import pytest

import layer_ref as LR
import pack_ref as P
import test_gpu_layers as TL
from state_bounds import load_golden

pytestmark = pytest.mark.gpu

CASES = P.expected_buffers()
RATIOS = {}      # (family, form) -> the largest figure
GROUP_STATES = ("global_a", "global_b", "global_a_seed1")
GROUP_WTS = np.array([[0.6, 0.3, 0.1], [0.2, 0.5, 0.3], [0.1, 0.25, 0.65]], np.float32)      # distinct rows, every style active


def _note(family, form, figure):
    RATIOS[family, form] = max(RATIOS.get((family, form), 0.0), figure)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (family, form), r in sorted(RATIOS.items()):
        print("\n[pack ratios] %s %s %.6g" % (family, form, r), end="")
    print()


@pytest.fixture(scope="module")
def handle(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    try:
        yield s, {(info["key"], info["form"]): (info, read) for info, read in s.debug_weights()}
    finally:
        s.close()


@pytest.fixture(scope="module")
def grouped(pkg, weights):
    """A grouped multi-style launch of three 8 x 8 frames with distinct weight rows: (handle, its buffers, each image's own state set)."""
    s = pkg.MultiStyleStylization(weights, cuda=True, style_num=len(GROUP_STATES))
    try:
        for k, name in enumerate(GROUP_STATES):
            s.set_state(load_golden(name)["state"], k)
        s.transfer_batch(TL.frames_for(pkg, 3, 8, 8), style_weights=GROUP_WTS)
        s.sync()
        sets = [LR.parse_state(s.debug_state_set(0, b)) for b in range(3)]
        yield s, {(info["key"], info["form"]): (info, read) for info, read in s.debug_weights()}, sets
    finally:
        s.close()


def test_the_enumeration_is_the_cases(handle):
    """A pack the library adds shows up here before anything else: the buffers it enumerates are exactly the parametrised cases."""
    s, buffers = handle
    listed = sorted((info["key"], info["form"]) for info, _ in s.debug_weights())
    assert len(listed) == len(set(listed)) == len(CASES), (len(listed), len(CASES))
    assert listed == CASES, sorted(set(listed) ^ set(CASES))
    for (key, form), (info, _) in buffers.items():
        assert info["sets"] == (P.N_SETS if ".fold_" in key else 1), (key, form, info)
        assert (info["BN"] > 0) == (form == "pk"), (key, form, info)


def test_read_back_refusals(pkg, handle):
    """Nothing is copied into a buffer that is too small; a bad index, a bad set and a set nothing folded are refused with a text."""
    import ctypes as C
    s, buffers = handle
    index = {(info["key"], info["form"]): i for i, (info, _) in enumerate(s.debug_weights())}
    i, n = index["Decoder.slice1", "last"], C.c_size_t(0)
    out = np.full(2048, 7.0, np.float32)
    assert s._lib.rrv_debug_copy_weights(s._h, i, 0, out.ctypes.data_as(C.c_void_p), 2047, C.byref(n)) == 0
    assert n.value == 2048 and np.all(out == 7.0)
    count = s._lib.rrv_debug_weight_count(s._h)
    for bad in (-1, count):
        assert s._lib.rrv_debug_copy_weights(s._h, bad, 0, None, 0, C.byref(n)) == -1
        assert s._lib.rrv_debug_weight_info(s._h, bad, None, 0, None, None, None, None, None, None, None) == -1
    assert s._lib.rrv_debug_copy_weights(s._h, i, 1, None, 0, C.byref(n)) == -1                       # a checkpoint weight has one buffer
    key = C.create_string_buffer(4)
    assert s._lib.rrv_debug_weight_info(s._h, i, key, 4, None, None, None, None, None, None, None) == -1      # the key does not fit
    _, read = buffers["Decoder.Filter2.fold_up", "raw"]
    with pytest.raises(pkg.RRVError, match="nothing has folded Decoder.Filter2.fold_up of state set 31"):
        read(31)
    with pytest.raises(pkg.RRVError, match="no state set 32"):
        read(32)


def _fold_case(label, read, kind, form, f, st, weights, raw_read, s_set, note=True):
    F = st["filt"]["Filter%d.F%d" % (f + 1, 1 if kind == "down" else 2)]
    got = read(s_set)
    ok, fig, fam = P.check_fold(kind, form, got, F, weights, f, got_raw=raw_read(s_set) if form == "pk_wino" else None,
                                kfold=min(P.FOLD_N, LR.K["fold"]), k32=min(P.PACK32_N, LR.K["pack32"]))
    print("[ratio] %s %s %s %s %.4g" % (label, kind, form, fam, fig))
    if note:
        _note(fam, "fold_%s.%s" % (kind, form), fig)
    return ok, fig, got


@pytest.mark.parametrize("key,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_buffer_against_its_reference(pkg, weights, handle, request, key, form):
    """One buffer against its reference (module docstring).  The controls of the fold cases measured ratios of 3.0e6 and more against K = 11."""
    s, buffers = handle
    info, read = buffers[key, form]
    if ".fold_" not in key:
        got = read()
        assert got.size == info["floats"]
        ok, fig, fam = P.check_buffer(key, form, got, weights, k32=min(P.PACK32_N, LR.K["pack32"]), kgrey=LR.K["grey"])
        print("[ratio] %s %s %s %.6g" % (key, form, fam, fig))
        _note(fam, form, fig)
        if form == "first_grey":      # the three parts, each against its own n
            v, m, n = P.first_grey(weights[key + ".weight"], weights[key + ".bias"])
            for part, sl in (("W1", slice(0, 576)), ("W0", slice(576, 1152)), ("bias", slice(1152, 1216))):
                _note(fam, "first_grey." + part, P.within(got[sl], v[sl], m[sl], n[sl])[1])
        assert ok, "%s %s (%s): %.6g" % (key, form, fam, fig)
        return
    f, kind = int(key[len("Decoder.Filter")]) - 1, key.rsplit("_", 1)[1]
    raw_read = buffers[key, "raw"][1]
    first = None
    for name in ("global_a", "global_b"):              # set 0: the second fold must replace the first
        blob = load_golden(name)["state"]
        s.set_state(blob)
        ok, fig, got = _fold_case(name, read, kind, form, f, LR.parse_state(blob), weights, raw_read, 0)
        assert ok, "%s %s on %s: ratio %.4g" % (key, form, name, fig)
        assert first is None or not np.array_equal(first, got)
        first = got
    g, gbuf, sets = request.getfixturevalue("grouped")
    gread, graw = gbuf[key, form][1], gbuf[key, "raw"][1]
    for b in range(3):                                  # the grouped launch: image b's weights on image b's own filter
        ok, fig, _ = _fold_case("image %d" % b, gread, kind, form, f, sets[b], weights, graw, b)
        assert ok, "%s %s image %d: ratio %.4g" % (key, form, b, fig)
    if form == "pk_wino":                               # control: image 1's pack is not the pack of image 0's folded weights
        ok, fig, _ = _fold_case("control", gread, kind, form, f, sets[1], weights, lambda _: graw(0), 1, note=False)
    else:                                               # control: image 1's folded weights are not image 0's filter times the checkpoint's
        ok, fig, _ = _fold_case("control", gread, kind, form, f, sets[0], weights, graw, 1, note=False)
    print("[control] %s %s image 1 on image 0's set: ratio %.4g" % (key, form, fig))
    assert not ok, "%s %s: image 1 passes on image 0's set (ratio %.4g)" % (key, form, fig)

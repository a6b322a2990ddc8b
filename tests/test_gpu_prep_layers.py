"""Every step of the once-per-video preparation pass (prepare_style, add, compute: resident and streaming) against the float64
stage references of tests/prep_ref.py.  Each case creates its handle fresh and runs compute() once per sync point with
rrv_debug_prep_stop set to it, profiled; the pass's kept workspace (rrv_debug_copy_prep_tensor) and the blob as it stands
(rrv_debug_copy_state) are then checked: each convolution on its own input tap, each statistic and its lo / hi on its own raw
tap, each predicted filter on the tensor it averaged, each in-place normalisation on the raw tensor the previous stop's run
left there and the blob's own statistics, after asserting that the two runs' blob entries of the earlier stages are bit-equal
(the pass has no atomics: that assertion is a determinism test of the pass).  The profile's row names must show the kernels
the module claims to cover, and every tap read has its zero ring checked.  Nothing is skipped, masked or sampled: every element
of every checked tensor is inside its bound (the two full-resolution cases evaluate the convolutions on LR.strips row bands and
the statistics, extrema and pointwise results on whole tensors).

Streaming: one group (a one-byte cap at one frame) gets every stop; the ragged multi-group cases get stops 0 .. 3 from the
stored features (the merged statistic with n_a > 0, the means-only merge, frame 0's chain).  The later multi-group stages keep
only the existing resident-versus-streaming comparison of tests/test_gpu_configs.py."""
import numpy as np
import pytest

import layer_ref as LR
import prep_ref as PR
from test_gpu_frame_mode_batch import _mixed, STYLE

pytestmark = pytest.mark.gpu

RATIOS = {f: (0.0, "-") for f in LR.FAMILIES}      # the largest figure per family over the module, and where


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[prep ratios] " + " ".join("%s=%.3g" % (f, RATIOS[f][0]) for f in LR.FAMILIES))
    print("[prep ratios at] " + " ".join("%s=%s" % (f, RATIOS[f][1]) for f in LR.FAMILIES))


def frames_for(pkg, B, H, W):
    return _mixed(pkg, B, H, W) if B > 1 else pkg.synth_frame(0, H, W, kind="smooth")[None]


class Run:
    """The workspace and the blob one stopped pass left: taps read once, in [H][W][C], zero ring checked on the way.  The next
    pass overwrites the workspace: what a later stop's checks need of this one (PR.KEEP) is read before, by keep()."""
    live = None

    def __init__(self, s, stop, B, sid=0):
        self.s, self.stop, self.B = s, stop, B
        self.blob = s.debug_style_blob(sid)
        self.st = LR.parse_state(self.blob)
        self.cache = {}
        Run.live = self

    def keep(self, images):
        for name in PR.KEEP.get(self.stop, ()):
            for b in images:
                self.get(name, b)
        return self

    def get(self, name, b=0):
        if (name, b) not in self.cache:
            assert Run.live is self, "%s[%d] of the pass stopped at %d was not read before the next pass ran" % (name, b, self.stop)
            t = self.s.debug_prep_tensor(name, b)
            H, W, C = t.shape[0] - 2, t.shape[1] - 2, t.shape[2]
            self.cache[name, b] = LR.ring_to_hwc(t, H, W, C)
        return self.cache[name, b]


def stopped(s, stop, B, sid=0):
    """compute() ended at `stop`, profiled: (Run, kernel names of the profile rows)."""
    s.debug_prep_stop(stop)
    s.profile_begin()
    s.compute()
    rows = [r[0].split("@")[0] for r in s.profile_end()]
    return Run(s, stop, B, sid), rows


def report(tag, results):
    """Prints every figure; returns the failures [(name, fraction of its bound)]."""
    bad = []
    for name, f, ok, worst, ratio in results:
        print("[ratio] %s %s %s %.3g (%.3g of the bound)%s" % (tag, name, f, ratio, worst, "" if ok else " FAILS"))
        if not ok:
            bad.append((name, worst))
        elif f is not None and ratio > RATIOS[f][0]:
            RATIOS[f] = (ratio, "%s:%s" % (tag, name))
    return bad


def walk(pkg, s, weights, tag, B, stops, images, strips=PR.whole, streaming=False, sid=0):
    """One stopped pass per stop of `stops`, each checked by its stage function.  Returns ({stop: Run}, rows of the last pass)."""
    c = PR.Ctx(weights, s.debug_style_pred(sid), images, strips=strips, streaming=streaming)
    runs, prev, bad, rows = {}, None, [], []
    for stop in stops:
        run, rows = stopped(s, stop, B, sid)
        if stop < PR.N_STOPS - 1:       # the style stays "not computed": no state to read, and the transfer entries refuse
            with pytest.raises(pkg.RRVError, match="not computed"):
                s.get_state()
            with pytest.raises(pkg.RRVError, match="state not computed"):
                s.transfer(np.zeros((8, 8, 3), np.uint8))
        if prev is not None and prev.stop != stop - 1:
            prev = None
        if prev is not None:
            assert PR.entries_bit_equal(prev.blob, run.blob, stop), "%s: stop %d rewrote an earlier stage's entry with other bits" % (tag, stop)
        bad += [(stop,) + x for x in report("%s stop %d" % (tag, stop), PR.STAGES[stop](run, prev, c))]
        runs[stop] = prev = run.keep(images)
        for old in list(runs):
            if old < stop:
                runs[old].cache.clear()
    assert not bad, "%s: %s" % (tag, bad)
    return runs, rows


def style_check(s, weights, tag, sid=0):
    st = LR.parse_state(s.debug_style_blob(sid))

    def get(name):
        t = s.debug_prep_tensor(name, sid if name == "map" else 0)
        return LR.ring_to_hwc(t, t.shape[0] - 2, t.shape[1] - 2, t.shape[2])

    bad = report(tag, PR.style_checks(get, st, s.debug_style_pred(sid), weights))
    assert not bad, "%s: %s" % (tag, bad)


def prepared(pkg, weights, frames, style=None):
    s = pkg.Stylization(weights, cuda=True)
    s.prepare_style(pkg.synth_style(**STYLE) if style is None else style)
    for f in frames:
        s.add(f)
    return s


# (B, H, W)
RESIDENT = [(1, 8, 8),            # one relu4_1 pixel: variance exactly 0, rstd = 1e4, lo == hi == 0
            (1, 16, 8),           # one-column feature
            (1, 8, 24),           # one-row feature
            (2, 33, 31),          # floors
            (3, 77, 90),          # level 0: 19008 pixels in 75 blocks of 254: a block's range is no multiple of nsub and ends inside a row
            (5, 136, 200)]        # 17 x 25 features: more than one tile each way at relu4_1; 532 blocks at level 0


@pytest.mark.parametrize("case", RESIDENT, ids=["%dx%dx%d" % c for c in RESIDENT])
def test_every_stop_of_the_resident_pass(pkg, weights, case):
    B, H, W = case
    frames = frames_for(pkg, B, H, W)
    s = prepared(pkg, weights, frames)
    try:
        with pytest.raises(pkg.RRVError, match="did not allocate"):
            s.debug_prep_tensor("cn")                          # no pass has run
        runs, rows = walk(pkg, s, weights, "%dx%dx%d" % case, B, range(PR.N_STOPS), sorted({0, B - 1}))
        # the kernels the figures belong to (stop 13 is a full pass)
        names = set(rows)
        assert {"chan_stat", "chan_final", "pointwise", "conv_mfma<32,9,0>", "conv_mfma<128,1,0>", "conv_mfma<64,1,0>", "conv_upw<E_LRELU>",
                "conv_wino<0>", "conv_wino<E_LRELU>"} <= names, sorted(names)
        assert not any(n.startswith("conv_upw_sc") or n.startswith("conv_f43") for n in names), sorted(names)
        assert rows.count("conv_upw<E_LRELU>") == 3 and rows.count("conv_mfma<32,9,0>") == 6 and rows.count("conv_wino<0>") == 3
        for b in range(B):      # the resident batch is the stored features, bit for bit
            np.testing.assert_array_equal(runs[13].get("content", b).view(np.uint32), runs[13].get("patch", b).view(np.uint32))
        with pytest.raises(pkg.RRVError, match="beyond the batch"):
            s.debug_prep_tensor("cn", B)
        with pytest.raises(pkg.RRVError, match="beyond the batch"):
            s.debug_prep_tensor("u", 1)
        with pytest.raises(pkg.RRVError, match="beyond the batch"):
            s.debug_prep_tensor("patch", B)
        with pytest.raises(pkg.RRVError, match="did not allocate"):
            s.debug_prep_tensor("grp")                         # a streaming pass's tensor
        if H == W == 8:
            mean, rstd, lo, hi = runs[13].st["norm"][0]
            assert np.allclose(rstd, 1e4, rtol=1e-6, atol=0) and not np.any(lo) and not np.any(hi)
        # stop 13 is a full pass: the state is computed and is the blob; with the knob off the same bits, and the plan is gone
        full = s.get_state()
        np.testing.assert_array_equal(full.view(np.uint32), runs[13].blob.view(np.uint32))
        if case == (2, 33, 31):
            s.debug_prep_stop(-1)
            with pytest.raises(pkg.RRVError, match="did not allocate"):
                s.debug_prep_tensor("cn")
            s.compute()
            np.testing.assert_array_equal(s.get_state().view(np.uint32), full.view(np.uint32))
            with pytest.raises(pkg.RRVError, match="did not allocate"):
                s.debug_prep_tensor("cn")
    finally:
        s.close()


FULL_RES = [(1, 520, 520),        # 270400 pixels > 1024 x 256: the block cap, ppb = 265, three trailing blocks empty
            (4, 4104, 8)]         # 16416 image rows at level 0: pointwise_k's strided row walk


@pytest.mark.parametrize("case", FULL_RES, ids=["%dx%dx%d" % c for c in FULL_RES])
def test_full_resolution_stops(pkg, weights, case):
    """Stops 0 and 11 .. 13: the statistics, extrema and pointwise results on whole tensors, the float64 convolutions on row bands."""
    B, H, W = case
    s = prepared(pkg, weights, frames_for(pkg, B, H, W))
    try:
        walk(pkg, s, weights, "%dx%dx%d" % case, B, (0, 11, 12, 13), sorted({0, B - 1}), strips=LR.strips)
    finally:
        s.close()


STYLES = [(16, 24),     # N = 6 at relu4_1: N - 1 matters
          (37, 53),     # floors
          (64, 64)]


@pytest.mark.parametrize("size", STYLES, ids=["%dx%d" % c for c in STYLES])
def test_style_side(pkg, weights, size):
    s = pkg.Stylization(weights, cuda=True)
    try:
        with pytest.raises(pkg.RRVError, match="prepare_style has not been called"):
            s.debug_style_blob(0)
        with pytest.raises(pkg.RRVError, match="did not allocate"):
            s.debug_prep_tensor("map", 0)
        s.prepare_style(pkg.synth_style(size[0], size[1], kind="smooth", seed=7))
        style_check(s, weights, "style %dx%d" % size)
    finally:
        s.close()


def test_two_styles(pkg, weights):
    """Two prepared styles, 2 x 33 x 31, a full pass: both blobs' norm[0] are the same bits (same content, same kernel), each
    style's own side holds, and the last style's stop-13 checks hold on the kept plan."""
    B, H, W = 2, 33, 31
    s = pkg.Stylization(weights, cuda=True, style_num=2)
    try:
        s.prepare_style([pkg.synth_style(64, 64, kind="smooth", seed=7), pkg.synth_style(37, 53, kind="smooth", seed=8)])
        style_check(s, weights, "style 1 of two", sid=1)            # (the style encoder's plan holds the last prepared style)
        assert s.debug_prep_tensor("map", 0).shape == (10, 10, 512) and s.debug_prep_tensor("map", 1).shape == (6, 8, 512)
        for f in frames_for(pkg, B, H, W):
            s.add(f)
        c = PR.Ctx(weights, s.debug_style_pred(1), (0, B - 1))
        prev = stopped(s, 12, B, sid=1)[0].keep(c.images)
        run, _ = stopped(s, 13, B, sid=1)
        assert PR.entries_bit_equal(prev.blob, run.blob, 13)
        bad = report("two styles stop 13", PR.STAGES[13](run, prev, c))
        assert not bad, bad
        b0, b1 = s.get_state(0), s.get_state(1)
        o, n = PR.OFFSETS["norm", 0]
        np.testing.assert_array_equal(b0[o:o + n].view(np.uint32), b1[o:o + n].view(np.uint32))
        assert not np.array_equal(b0, b1)
    finally:
        s.close()


def test_streaming_one_group_every_stop(pkg, weights):
    """1 x 33 x 31 under a one-byte cap: G = 1, one group; the same references on grp, f0, su[f] and image 0 of cn."""
    B, H, W = 1, 33, 31
    s = prepared(pkg, weights, frames_for(pkg, B, H, W))
    try:
        s.set_workspace_cap(1)
        runs, rows = walk(pkg, s, weights, "streaming 1x33x31", B, range(PR.N_STOPS), (0,), streaming=True)
        assert s.last_compute_info()[:2] == (1, 1)
        assert "chan_stat" not in rows and "conv_upw<E_LRELU>" in rows and "conv_mfma<32,9,0>" in rows      # the merged statistics are not profiled rows
        np.testing.assert_array_equal(runs[13].get("f0", 0).view(np.uint32), runs[13].get("patch", 0).view(np.uint32))
        with pytest.raises(pkg.RRVError, match="did not allocate"):
            s.debug_prep_tensor("content")
        streamed = s.get_state()
        np.testing.assert_array_equal(streamed.view(np.uint32), runs[13].blob.view(np.uint32))
    finally:
        s.close()


def _cap_for(s, G, hi):
    """The smallest cap (to 1 KB) at which the groups hold G frames, by bisection on last_compute_info over passes stopped at 0."""
    s.debug_prep_stop(0)
    lo = 1
    while hi - lo > 1024:
        mid = (lo + hi) // 2
        s.set_workspace_cap(mid)
        s.compute()
        if s.last_compute_info()[1] >= G:
            hi = mid
        else:
            lo = mid
    return hi


@pytest.fixture(scope="module")
def ragged(pkg, weights):
    """5 x 40 x 56 on one handle: the frames' stored features (read once), and the resident workspace size."""
    B, H, W = 5, 40, 56
    s = prepared(pkg, weights, frames_for(pkg, B, H, W))
    s.set_workspace_cap(1 << 40)
    run, _ = stopped(s, 0, B)
    info = s.last_compute_info()
    assert info[:2] == (1, B)
    patches = [run.get("patch", b) for b in range(B)]
    yield s, patches, info[2]
    s.close()


@pytest.mark.parametrize("G", (1, 2, 3))
def test_streaming_ragged_groups(pkg, weights, ragged, G):
    """5 x 40 x 56 in groups of G (1,1,1,1,1 / 2,2,1 / 3,2): the merged norm[0] (n_a > 0, real mean differences, C = 512) against the
    float64 statistic of all five stored features; the means-only merge at C = 32 through both predicted filters of each
    KernelFilter from feature-derived inputs; frame 0's chain cn[0] -> d32 -> su[f] from its taps."""
    s, patches, resident_bytes = ragged
    B = len(patches)
    cap = 1 if G == 1 else _cap_for(s, G, resident_bytes)
    s.set_workspace_cap(cap)
    c = PR.Ctx(weights, s.debug_style_pred(0), (0,), streaming=True)
    tag = "streaming 5x40x56 G=%d" % G
    run, _ = stopped(s, 0, G)
    assert s.last_compute_info()[:2] == ((B + G - 1) // G, G), s.last_compute_info()
    bad = report(tag + " stop 0", PR.multi_norm0(patches, run.st, c))
    prev = run
    for f in range(3):
        run, _ = stopped(s, 1 + f, G)
        assert PR.entries_bit_equal(prev.blob, run.blob, 1 + f)
        bad += report(tag + " stop %d" % (1 + f), PR.multi_filter(f, patches, run, c))
        prev = run
    assert not bad, bad


def test_bounds_reject_wrong_values_on_real_data(pkg, weights):
    """The bounds are not vacuous on the GPU's own numbers (3 x 77 x 90): a reference that leaves one median pixel, or the last
    block's tail, out of a statistic, a residual not added, and image 1's input taken for image 2's must all fail."""
    B, H, W = 3, 77, 90
    s = prepared(pkg, weights, frames_for(pkg, B, H, W))
    try:
        k = LR.K
        run, _ = stopped(s, 0, B)
        x = np.stack([run.get("content", b) for b in range(B)]).reshape(-1, 512)
        assert PR.check_pstat(run.st["norm"][0], PR.raw_stats(x), k["pstat"])[0]
        c = int(np.argmax(x.var(axis=0)))
        median = int(np.argsort(x[:, c])[x.shape[0] // 2])
        assert not PR.check_pstat(run.st["norm"][0], PR.raw_stats(np.delete(x, median, axis=0)), k["pstat"])[0]
        assert not PR.check_pstat(run.st["norm"][0], PR.raw_stats(x[:-(x.shape[0] % 16 or 1)]), k["pstat"])[0]
        run, _ = stopped(s, 1, B)
        cn, nxt, u = run.get("cn", 2), run.get("nxt", 2), run.get("u", 0)
        assert LR.check(nxt, *PR.added(cn, u), k["point"])[0]
        assert not LR.check(nxt, *PR.added(cn, 0.0 * u), k["point"])[0]
        assert not LR.check(nxt, *PR.added(run.get("cn", 1), u), k["point"])[0]
        p = "Decoder.Filter1.F2.down_sample.0."
        assert not LR.check(run.get("t32", 2), *LR.conv3(run.get("cn", 1), weights[p + "weight"], weights[p + "bias"], 0, cn.shape[0]), k["gemm"])[0]
    finally:
        s.close()

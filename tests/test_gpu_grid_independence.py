"""Results do not depend on the grid (include/rerevst_hip.h, rrv_set_grid_share; RRV_CUS): every path of the library on handles whose
persistent kernels chain many work items per workgroup, against a handle on which every workgroup runs one item or none.

  reference handle   RRV_CUS=1024, share 1.  Asserted from the grids the library reports (rrv_profile_entry_grid): every launch has one
                     workgroup per item, so no boundary code between two items runs.  This is the configuration the layer suites hold
                     to float64.
  grid handles       GRIDS below, set through RRV_CUS at creation and rrv_set_grid_share only (no CU mask: the grids are the same on
                     any device).  5 workgroups: the plain walk with a slab change inside every chain; 24: the plain walk with
                     grid % slabs == 0 for 2 / 4 / 8 slabs (a slab change for 16); 256 CUs at share 2 / 3 / 4 = 128 / 80 / 64 workgroups:
                     the XCD walk (64 where a level has fewer than 128 items) and grid % 16 == 0 on the plain walk (80).
Frames of 136 x 200, three per launch: the smallest with more than eight 16 x 16 tiles per launch at the 1/8 level.

Each case runs one path in a fixed kernel mode on both handles and asserts the same kernel names and bit-for-bit equality of the
delivered output, the pre-clamp image, every tensor rrv_debug_copy_tensor_ex hands out for every image (rings and padding included),
and the per-image state sets where the path has them; on the 5-workgroup handle the global and frame-mode paths are also held to the
float64 layer references (test_gpu_layers.check_image, test_gpu_frame_mode_layers.check_image, the families' K unchanged).

Which walk a launch took is read from the library's record (grid, xcd_slabs); tests/grid_ref.py turns it into the longest chain and
the slab / image changes inside chains.  At module end the classes seen per kernel symbol must equal test_grid_walk.WALKS (the rows
of the other family dropped under RRV_F43=0 / 2), and the table is printed (profiles/grid_walk.txt keeps one run's)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import grid_ref as GR
import layer_ref as LR
import mask_layer_ref as MR
import mask_ref
import test_grid_walk as GW
import test_gpu_frame_mode_layers as FL
import test_gpu_layers as TL
from conftest import fixed_kernels, forced_family
from state_bounds import load_golden
from test_gpu_frame_mode_batch import STYLE
from test_gpu_mask_blend import _golden_setup, _mixed

pytestmark = pytest.mark.gpu

L = importlib.import_module("rerevst-code_amd._lib")
V = importlib.import_module("rerevst-code_amd.video")

H, W, B = 136, 200, 3
REF = (1024, 1)
GRIDS = [(5, 1), (24, 1), (256, 2), (256, 3), (256, 4)]
IDS = ["cus%d-share%d" % g for g in GRIDS]
FEW = (5, 1)                        # the handle that is also held to float64
N_TAPS = len(LR.TAP_NAMES)
E = dict(E_RELU=1, E_LRELU=2, E_NORM1=4, E_RES=8, E_RES_UPS=16, E_NORM2=32, E_POOL=64)      # conv_mfma.h

SEEN = {}        # kernel symbol -> {class: {test names}}
_REFS = {}       # (path key) -> the reference handle's record


# ---- from a profile row to (kernel symbol, geometry, class) ---------------------------------------------------------------------------

def symbol_of(kernel, per_image):
    """The ledger's key (tests/kernel_ledger.py) of a transform-domain profile row name, e.g. 'conv_wino<E_RELU | E_POOL>'."""
    m = re.match(r"^(conv_wino|conv_upw_sc|conv_upw|conv_f43)<(.*)>$", kernel)
    if not m:
        return None
    fam, arg = m.groups()
    lay = 0
    if fam == "conv_f43" and "," in arg:
        arg, lay = arg.rsplit(",", 1)
    epi = eval(arg, {"__builtins__": {}}, E)
    if fam == "conv_f43":
        return "conv_f43_k<%d, %d>" % (epi, int(lay))
    if fam == "conv_wino":
        return "conv_wino_split_k<%d, %d>" % (epi, int(per_image))
    return "conv_wino_k<%d, 0, 4, 1, %d, %d>" % (epi, fam == "conv_upw_sc", int(per_image) if fam == "conv_upw_sc" else 0)


def geometry(row):
    """(tiles_x, tiles_y, slabs) of a transform-domain row '<kernel>@CinxCout@HxW': 32 x 32 pixel items for conv_f43_k and the
    shortcut-fused upsample kernel, 16 x 16 otherwise; one slab per 32 couts, split K's slices on the 512 -> 32 down convolution."""
    kernel, cc, hw = row.split("@")
    cin, cout = (int(v) for v in cc.split("x"))
    h, w = (int(v) for v in hw.split("x"))
    ts = 32 if kernel.startswith(("conv_f43", "conv_upw_sc")) else 16
    slabs = cout // 32
    if kernel == "conv_wino<0>" and (cin, cout) == (512, 32):
        slabs *= GR.kf_split(h, w)
    return (w + ts - 1) // ts, (h + ts - 1) // ts, slabs


class Rec:
    """What one handle's run of a path left, on the host."""

    def __init__(self, s, out, images_of=lambda i, row: B, per_image=lambda i, row: False, last=None, ntiles_last=None):
        self.names = [r[0] for r in s.profile_end()]
        self.grids = s.profile_grids()
        assert len(self.names) == len(self.grids)
        self.out = out
        self.images_of, self.per_image, self.last, self.ntiles_last = images_of, per_image, last, ntiles_last
        self.taps, self.sets, self.pre = {}, {}, {}

    def walks(self):
        """[(symbol, grid, items, classes)] of the persistent launches of the record."""
        out = []
        for i, (row, (grid, xcd)) in enumerate(zip(self.names, self.grids)):
            kernel = row.split("@")[0]
            if kernel == "conv_last":
                if self.last is not None:
                    out.append((self.last, grid, self.ntiles_last, GR.last_classes(grid, self.ntiles_last)))
                continue
            sym = symbol_of(kernel, self.per_image(i, row))
            if sym is None:
                assert xcd == -1, (row, grid, xcd)
                continue
            assert grid > 0 and xcd in (0, 1), (row, grid, xcd)
            tx, ty, slabs = geometry(row)
            n = self.images_of(i, row)
            out.append((sym, grid, tx * ty * n * slabs, GR.td_classes(grid, xcd, tx, ty, n, slabs, self.per_image(i, row))))
        return out


def note(rec, test, reference, only=None):
    """The reference handle: one workgroup per item in every persistent launch (which also proves the geometry read from the row
    names).  A grid handle: at most that, and the classes it ran are filed under the test's name.  only: the one symbol a case is
    about (its frames are too large for the other launches of the reference handle to be chain-free)."""
    for sym, grid, items, classes in rec.walks():
        if only is not None and sym != only:
            assert grid <= items, (sym, grid, items)
            continue
        if reference:
            assert grid == items and not classes, (sym, grid, items, classes)
        else:
            assert grid <= items, (sym, grid, items)
            for c in classes:
                SEEN.setdefault(sym, {}).setdefault(c, set()).add(test)


def read_taps(pkg, s, rec, h, w, n, pre=True, sets=False, only=None):
    for idx in (range(N_TAPS) if only is None else [LR.TAP[t] for t in only]):
        for b in range(n):
            try:
                rec.taps[idx, b] = s.debug_tensor_ex(0, idx, h, w, b)
            except pkg.RRVError as e:
                assert "did not write" in str(e) or "no such tensor" in str(e), e
                rec.taps[idx, b] = None
    for b in range(n):
        if pre:
            rec.pre[b] = s.preclamp(h // 8 * 8, w // 8 * 8, image=b)
        if sets:
            rec.sets[b] = s.debug_state_set(0, b)
    assert sum(v is not None for v in rec.taps.values()) >= (13 if only is None else len(only)) * n, "fewer taps than any path writes"
    return rec


def same(ref, got):
    assert got.names == ref.names                                  # the same kernels either way
    np.testing.assert_array_equal(got.out, ref.out)
    assert got.taps.keys() == ref.taps.keys() and got.pre.keys() == ref.pre.keys() and got.sets.keys() == ref.sets.keys()
    for b in ref.pre:
        np.testing.assert_array_equal(got.pre[b], ref.pre[b], err_msg="pre-clamp image %d" % b)
    for b in ref.sets:
        np.testing.assert_array_equal(got.sets[b], ref.sets[b], err_msg="state set of image %d" % b)
    for (idx, b), r in ref.taps.items():
        g = got.taps[idx, b]
        assert (g is None) == (r is None), (LR.TAP_NAMES[idx], b)
        if r is not None:
            assert g[1:] == r[1:], (LR.TAP_NAMES[idx], b)
            np.testing.assert_array_equal(g[0], r[0], err_msg="%s image %d" % (LR.TAP_NAMES[idx], b))


def pair(key, test, run, grid, only=None):
    """run(cus, share) -> Rec on the reference configuration (once per key) and on `grid`; notes both, compares them."""
    if key not in _REFS:
        while len(_REFS) >= 2:                  # the cases of a path follow each other: keep two paths' reference taps, not all
            del _REFS[next(iter(_REFS))]
        _REFS[key] = run(*REF)
        note(_REFS[key], test, True, only)
    got = run(*grid)
    note(got, test, False, only)
    same(_REFS[key], got)
    return got


@pytest.fixture(scope="module", autouse=True)
def _coverage():
    yield
    _REFS.clear()
    want = GW.expected(os.environ.get("RRV_F43"))
    lines = []
    for sym in sorted(set(want) | set(SEEN)):
        lines.append("%-34s %s" % (sym, "  ".join("%s: %s" % (c, ",".join(sorted(t))) for c, t in sorted(SEEN.get(sym, {}).items())) or "-"))
    print("\n[grid walks] classes seen per kernel symbol (A XCD walk, B plain walk grid % slabs == 0, C slab change inside a chain, "
          "I image change with per-image state; band / rr: conv_last_k)\n" + "\n".join(lines))
    if len(_RAN) < len(ALL_TESTS):
        return            # a partial run (-k): the table is printed, not asserted
    assert {s: set(c) for s, c in SEEN.items()} == {s: set(c) for s, c in want.items()}
    for sym, classes in want.items():
        for c, test in classes.items():
            assert test.split("::")[1] in SEEN[sym][c], (sym, c, test)


_RAN = set()
ALL_TESTS = ("test_global_mode0", "test_global_mode2", "test_grouped_per_image_state", "test_blended_frames_per_image_state", "test_frame_mode",
             "test_frame_mode_unsplit_filter_down",
             "test_preparation_pass", "test_masked_blend", "test_output_forms", "test_output_views_and_pad_crop", "test_tickets_and_grid_share")


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    _RAN.add(request.node.name.split("[")[0])


def plain_handle(pkg, weights, cus, share, p8=3, **kw):
    with TL.env(RRV_CUS=cus, RRV_P8=p8, RRV_F43_LAYERS=hex(0x3ff)):
        s = pkg.Stylization(weights, cuda=True, **kw)
    s.set_grid_share(share)
    return s


def multi_handle(pkg, weights, cus, share, style_num, p8=3):
    with TL.env(RRV_CUS=cus, RRV_P8=p8, RRV_F43_LAYERS=hex(0x3ff)):
        s = pkg.MultiStyleStylization(weights, cuda=True, style_num=style_num)
    s.set_grid_share(share)
    return s


def seq_of(rows):
    return [(n, i + 1 < len(rows) and rows[i + 1].startswith("sum_parts")) for i, n in enumerate(rows) if not n.startswith("sum_parts")]


# ---- a, b. the global path ---------------------------------------------------------------------------------------------------------------

def run_global(pkg, weights, frames, blob, mode, p8, cus, share, live=None):
    n, h, w, _ = frames.shape
    with fixed_kernels(mode=mode):
        s = plain_handle(pkg, weights, cus, share, p8=p8)
    try:
        with fixed_kernels(s, mode=mode):
            s.set_state(blob)
            d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
            d_out = torch.empty((n, h // 8 * 8, w // 8 * 8, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            s.profile_begin()
            s.transfer_batch_device(d_in.data_ptr(), n, h, w, d_out.data_ptr())
            s.profile_end()
            s.sync()
        rec = read_taps(pkg, s, Rec(s, d_out.cpu().numpy(), images_of=lambda i, row: n), h, w, n)
        assert len(seq_of(rec.names)) == LR.N_LAUNCHES, rec.names
        if live:
            live(s, seq_of(rec.names))
        return rec
    finally:
        s.close()


def _global(pkg, weights, test, mode, p8, grid):
    blob = load_golden("global_a")["state"]
    st = LR.parse_state(blob)
    frames = TL.frames_for(pkg, B, H, W, seed=900)

    def live(s, seq):      # the chained configuration against the float64 references themselves
        for b in sorted({0, B - 1}):
            fam, lay = TL.check_image(s, weights, st, seq, H, W, b, frames[b])
            if not forced_family():
                want = "f43" if mode == 2 else "f23"
                assert all(fam[n] == want for n in TL.ENC_F43 + TL.DEC_F43), fam
                assert fam["a4"] == fam["a3"] == fam["a2"] == "ups"

    def run(cus, share):
        return run_global(pkg, weights, frames, blob, mode, p8, cus, share, live=live if (cus, share) == FEW else None)

    return pair(("global", mode, p8), test, run, grid)


@pytest.mark.parametrize("grid", GRIDS, ids=IDS)
def test_global_mode0(pkg, weights, grid):
    """a. F(2x2,3x3) on every packed layer: conv_wino_split_k<1,0>, <65,0>, <54,0> chained (the item boundary suite runs mode 2 only)."""
    _global(pkg, weights, "test_global_mode0", 0, 3, grid)


@pytest.mark.parametrize("p8", [3, 0], ids=["p8", "nhwc"])
@pytest.mark.parametrize("grid", GRIDS, ids=IDS)
def test_global_mode2(pkg, weights, grid, p8):
    """b. conv_f43_k on every packed layer, channel-chunk-major tensors between them (RRV_P8=3) and NHWC (0)."""
    _global(pkg, weights, "test_global_mode2", 2, p8, grid)


# ---- c. per-image state on the fused path -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def states(pkg, oracle, weights):
    """Four computed states, every pair different in Decoder.norm[0] (mask_ref.distinct_states asserts it)."""
    return mask_ref.distinct_states(*_golden_setup(pkg, oracle, weights, "multistyle_s4")[:2])


@pytest.mark.parametrize("mode,p8", [(0, 3), (2, 3), (2, 0)], ids=["f23", "f43-p8", "f43-nhwc"])
@pytest.mark.parametrize("grid", GRIDS, ids=IDS)
def test_grouped_per_image_state(pkg, weights, states, grid, mode, p8):
    """The grouped multi-style launch on cached features (rrv_transfer_features_batch, as test_chained_items_with_per_image_state):
    every image has a blended state set of its own, so an image change inside a chain re-stages the epilogue parameters, and the
    KernelFilter convolutions read per-image folded weights (w_bstride).  In mode 2 ResidualBlock.conv2 runs conv_f43_k, which reads
    the per-image parameters itself (both layouts of its input)."""
    frames = [pkg.synth_frame(910 + i, H, W, kind="smooth") for i in range(B)]
    wts = [V.ramp_weights(i, B, 2, blend="all") for i in range(B)]

    def run(cus, share):
        with fixed_kernels(mode=mode):
            s = multi_handle(pkg, weights, cus, share, 2, p8=p8)
        try:
            with fixed_kernels(s, mode=mode):
                for k in range(2):
                    s.set_state(states[k], k)
                feats = [s.generate_content_features(f) for f in frames]
                s.set_multistyle_group(16)
                s.profile_begin()
                out = np.array(s.transfer_many(feats, wts))
                s.profile_end()
                s.sync()
            rec = Rec(s, out, per_image=lambda i, row: True)
            assert [n.split("@")[0] for n in rec.names[:B]] == ["pointwise"] * B, rec.names
            return read_taps(pkg, s, rec, H, W, B, sets=True)
        finally:
            s.close()

    pair(("grouped", mode, p8), "test_grouped_per_image_state", run, grid)


WTS = np.array([[0.6, 0.3, 0.1], [0.2, 0.5, 0.3], [0.1, 0.25, 0.65]], np.float32)


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[2], GRIDS[3]], ids=[IDS[0], IDS[2], IDS[3]])
def test_blended_frames_per_image_state(pkg, weights, states, grid):
    """Frames blended from three states through transfer_batch(style_weights=): conv4_1 normalises with per-image Decoder.norm[0]
    (conv_wino_split_k<5,1>), the decoder as in the grouped launch.  Mode 0."""
    frames = _mixed(pkg, 80, B, H, W)

    def run(cus, share):
        with fixed_kernels(mode=0):
            s = multi_handle(pkg, weights, cus, share, 3)
        try:
            with fixed_kernels(s, mode=0):
                for k in range(3):
                    s.set_state(states[k], k)
                s.profile_begin()
                out = np.array(s.transfer_batch(frames, style_weights=WTS))
                s.profile_end()
                s.sync()
            rec = Rec(s, out)
            first = [i for i, n in enumerate(rec.names) if n.startswith("conv_first")]
            assert len(first) == 1, rec.names
            rec.per_image = lambda i, row: i >= first[0] + 8         # conv4_1 (the ninth launch of the sequence) and the decoder
            return read_taps(pkg, s, rec, H, W, B, sets=True)
        finally:
            s.close()

    pair(("blend",), "test_blended_frames_per_image_state", run, grid)


# ---- d. frame mode -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", GRIDS, ids=IDS)
def test_frame_mode(pkg, weights, grid):
    """Batched frame mode: each image's folded KernelFilter weights (w_bstride changes inside a chain), conv_wino_split_k<0,1>, <8,1>,
    <40,1>, the raw conv_wino_k<2,0,4,1,1,0> and conv_wino_split_k<2,0> of the unfused blocks."""
    _frame_mode(pkg, weights, "test_frame_mode", FL.frames_for(pkg, B, H, W), grid, float64=True)


def _frame_mode(pkg, weights, test, frames, grid, float64=False, only=None, symbol=None):
    n, h, w, _ = frames.shape

    def run(cus, share):
        s = plain_handle(pkg, weights, cus, share, use_Global=False)
        try:
            s.prepare_style(pkg.synth_style(**STYLE))
            smean = s.debug_style_pred(0).astype(np.float64)
            d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
            d_out = torch.empty((n, h // 8 * 8, w // 8 * 8, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            s.profile_begin()
            s.transfer_batch_device(d_in.data_ptr(), n, h, w, d_out.data_ptr())
            s.profile_end()
            s.sync()
            rec = Rec(s, d_out.cpu().numpy(), images_of=lambda i, row: n, per_image=lambda i, row: "@512x32@" in row or "@32x512@" in row)
            read_taps(pkg, s, rec, h, w, n, sets=True, only=only)
            if float64 and (cus, share) == FEW:
                start = [i for i, row in enumerate(rec.names) if row.startswith("frame_sets_init")]
                fam = LR.frame_families(seq_of(rec.names[start[-1]:]))
                for b in sorted({0, n - 1}):
                    FL.check_image(s, weights, smean, fam, h, w, b, frames[b])
            return rec
        finally:
            s.close()

    return pair(("frame", n, h, w), test, run, grid, only=symbol)


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]], ids=IDS[:2])
def test_frame_mode_unsplit_filter_down(pkg, weights, grid):
    """conv_wino_split_k<2,1>, the KernelFilter down convolution WITHOUT split K on per-image folded weights, is launched from 129
    tiles of relu4_1 per frame on (kf_split): two frames of 8 x 16400, one tile row — the one case of the module above 136 x 200.
    One cout slab, so the slab never changes: the image change inside a chain stands in its place.  Output, pre-clamp image, state
    sets and the taps around the KernelFilter.  (The reference handle runs this kernel's 258 items on 258 workgroups; its other
    launches have more items than 1024 workgroups at this size and are compared as one more pair of grids.)"""
    h, w = 8, 16400
    assert GR.kf_split(h // 8, w // 8) == 1 and GR.kf_split(h // 8, w // 8 - 16) > 1
    got = _frame_mode(pkg, weights, "test_frame_mode_unsplit_filter_down", FL.frames_for(pkg, 2, h, w), grid, only=("c41", "d", "f1", "f2", "f3", "o4", "o2"),
                      symbol="conv_wino_split_k<2, 1>")
    assert sum(row.startswith("conv_wino<E_LRELU>@512x32@") for row in got.names) == 3 and not any(row.startswith("sum_parts") for row in got.names)


# ---- e. the preparation pass --------------------------------------------------------------------------------------------------------------

PREP_GRIDS = [GRIDS[0], GRIDS[1], GRIDS[2]]


@pytest.mark.parametrize("streaming", [False, True], ids=["resident", "streaming"])
@pytest.mark.parametrize("grid", PREP_GRIDS, ids=IDS[:3])
def test_preparation_pass(pkg, weights, grid, streaming):
    """compute() stopped at each of its 14 sync points on both handles side by side: the style's blob as it stands and every tensor of
    the kept workspace, every image.  The nine-product conv_wino_k<2,0,4,1,0,0> runs two workgroups per CU; the folded KernelFilter
    convolutions run on frame 0 alone (one image), the streaming pass (a one-byte cap) one frame per group."""
    frames = FL.frames_for(pkg, B, H, W)
    test = "test_preparation_pass"

    def make(cus, share):
        s = plain_handle(pkg, weights, cus, share)
        s.prepare_style(pkg.synth_style(**STYLE))
        for f in frames:
            s.add(f)
        if streaming:
            s.set_workspace_cap(1)
        return s

    def stop_at(s, stop):
        s.debug_prep_stop(stop)
        s.profile_begin()
        s.compute()
        n = 1 if streaming else B
        rec = Rec(s, s.debug_style_blob(0))
        # the first compute() encodes the frames add() collected, all in one launch sequence (conv_first and eight convolutions)
        first = [i for i, row in enumerate(rec.names) if row.startswith("conv_first")]
        assert len(first) == (stop == 0), rec.names
        enc = range(first[0], first[0] + 9) if first else ()
        rec.images_of = lambda i, row: B if i in enc else 1 if "@512x32@" in row or "@32x512@" in row else n
        for name in L.PREP_TENSORS:
            for b in range(B):
                try:
                    rec.taps[name, b] = s.debug_prep_tensor(name, b)
                except pkg.RRVError as e:
                    assert "did not allocate" in str(e) or "beyond the batch" in str(e), e
                    rec.taps[name, b] = None
        return rec

    ref, got = make(*REF), None
    try:
        got = make(*grid)
        for stop in range(14):
            r, g = stop_at(ref, stop), stop_at(got, stop)
            note(r, test, True)
            note(g, test, False)
            assert g.names == r.names
            np.testing.assert_array_equal(g.out.view(np.uint32), r.out.view(np.uint32), err_msg="blob at stop %d" % stop)
            assert sum(v is not None for v in r.taps.values()) >= 2
            for k, v in r.taps.items():
                assert (g.taps[k] is None) == (v is None), (stop, k)
                if v is not None:
                    np.testing.assert_array_equal(g.taps[k].view(np.uint32), v.view(np.uint32), err_msg="stop %d %s image %d" % ((stop,) + k))
        assert streaming == (ref.last_compute_info()[1] < B)
    finally:
        ref.close()
        if got is not None:
            got.close()


# ---- f. one masked-blend call -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[2]], ids=[IDS[0], IDS[2]])
def test_masked_blend(pkg, weights, states, grid):
    """The masked multi-style walk (mask_norm_k and mask_filter_k between raw convolutions), a mask per image, four styles."""
    S = 4
    frames = _mixed(pkg, 40, B, H, W)
    M = MR.softmax_mask(1000 + H, S, H, W, B=B)

    def run(cus, share):
        s = multi_handle(pkg, weights, cus, share, S)
        try:
            for k in range(S):
                s.set_state(states[k], k)
            x = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
            torch.cuda.synchronize()
            s.profile_begin()
            out = s.transfer_tensor(x, layout="nhwc", style_masks=M)
            s.profile_end()
            s.sync()
            rec = Rec(s, out.cpu().numpy())
            assert any(n.startswith("mask_norm") for n in rec.names) and not any(n.startswith("conv_f43") for n in rec.names), rec.names
            return read_taps(pkg, s, rec, H, W, B)
        finally:
            s.close()

    pair(("mask",), "test_masked_blend", run, grid)


# ---- g. the output forms of conv_last_k ----------------------------------------------------------------------------------------------------

F32 = "conv_last_k<false, %s, %d, false, false>"
YUV8 = "conv_last_k<true, false, 0, true, false>"
YUV16 = "conv_last_k<true, false, 0, true, true>"
# (id, transfer_tensor keywords, the instantiation that writes it: rerevst_hip.hip last_kernel)
FORMS = [("f32-%s-%s" % (lay, sp), dict(out_layout=lay, out_space=sp), F32 % ("true" if lay == "nchw" else "false", k))
         for lay in ("nhwc", "nchw") for k, sp in enumerate(("pixel", "unit", "norm"))]
FORMS += [("u8-nhwc", dict(out_layout="nhwc", out_dtype=torch.uint8), "conv_last_k<true, false, 0, false, false>"),
          ("u8-nchw", dict(out_layout="nchw", out_dtype=torch.uint8), "conv_last_k<true, true, 0, false, false>")]
FORMS += [(f, dict(out_layout=f), YUV8) for f in ("i420", "nv12", "i422", "nv16", "i444", "nv24")]
FORMS += [(f, dict(out_layout=f), YUV16) for f in ("i420p10", "p010", "i422p10", "p210", "i444p16", "p416")]
LAST_GRIDS = [(5, 1), (24, 1)]          # 20 workgroups: the round-robin walk; 96: one band per XCD


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


@pytest.fixture(scope="module")
def last_handles(pkg, weights):
    """One handle per configuration for all the forms (the form is a property of the call): reference, 20 and 96 workgroups."""
    blob = load_golden("global_a")["state"]
    hs = {}
    with fixed_kernels(mode=0):
        for g in [REF] + LAST_GRIDS:
            hs[g] = plain_handle(pkg, weights, *g)
            hs[g].set_state(blob)
    yield hs
    for s in hs.values():
        s.close()


def _form(s, x, kw, sym, ntiles):
    with fixed_kernels(s, mode=0):
        s.profile_begin()
        out = s.transfer_tensor(x, layout="nhwc", **kw)
        s.profile_end()
        s.sync()
    return Rec(s, _bytes(out), last=sym, ntiles_last=ntiles), out


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_output_forms(pkg, last_handles, form):
    """Every instantiation of conv_last_k in both of its walks: the delivered bytes against the reference handle's."""
    _, kw, sym = form
    x = torch.from_numpy(TL.frames_for(pkg, B, H, W, seed=930)).cuda()
    ntiles = ((H + 15) // 16) * ((W + 15) // 16) * B
    ref, _ = _form(last_handles[REF], x, kw, sym, ntiles)
    assert [g for n, (g, _) in zip(ref.names, ref.grids) if n == "conv_last"] == [ntiles]
    for g in LAST_GRIDS:
        got, _ = _form(last_handles[g], x, kw, sym, ntiles)
        note(got, "test_output_forms", False)
        assert GR.last_classes(dict(zip(got.names, got.grids))["conv_last"][0], ntiles) == {"rr" if g == LAST_GRIDS[0] else "band"}
        assert got.names == ref.names
        np.testing.assert_array_equal(got.out, ref.out)


def test_output_views_and_pad_crop(pkg, last_handles):
    """A ragged output view (a window of a larger canvas: nothing outside it is written) and the TF_PAD_CROP window on an odd size
    (70 x 99), each against the reference handle's bytes."""
    x = torch.from_numpy(TL.frames_for(pkg, B, H, W, seed=940)).cuda()
    odd = torch.from_numpy(TL.frames_for(pkg, B, 70, 99, seed=950)).cuda()
    outs = {}
    for g, s in last_handles.items():
        canvas = torch.full((B, H + 5, W + 7, 3), -1.0, dtype=torch.float32, device="cuda")
        with fixed_kernels(s, mode=0):
            view = canvas[:, 2:2 + H, 3:3 + W, :]
            assert s.transfer_tensor(x, layout="nhwc", out=view) is view
            crop = s.transfer_tensor(odd, layout="nhwc", pad_crop=True)
            crop8 = s.transfer_tensor(odd, layout="nhwc", pad_crop=True, out_dtype=torch.uint8)
            s.sync()
        assert tuple(crop.shape) == (B, 70, 99, 3)
        outs[g] = (_bytes(canvas), _bytes(crop), _bytes(crop8))
    assert np.all(outs[REF][0].view(np.float32).reshape(B, H + 5, W + 7, 3)[:, :2] == -1.0)
    for g in LAST_GRIDS:
        for a, r in zip(outs[g], outs[REF]):
            np.testing.assert_array_equal(a, r)


# ---- tickets and rrv_set_grid_share ---------------------------------------------------------------------------------------------------------

def test_tickets_and_grid_share(pkg, weights, last_handles):
    """Three look-ahead tickets open at once (the library gives each launch a share of 1 .. 3 by itself) deliver the reference
    handle's bytes; the share the caller set is back afterwards, seen in the next launch's reported grids; values outside 1 .. 4
    are refused and change nothing."""
    frames = TL.frames_for(pkg, 3, H, W, seed=960)
    x = torch.from_numpy(frames).cuda()
    want = None
    for g in [REF, (5, 1), (256, 1)]:
        s = last_handles[g] if g in last_handles else plain_handle(pkg, weights, *g)
        try:
            if g not in last_handles:
                s.set_state(load_golden("global_a")["state"])
            with fixed_kernels(s, mode=0):
                def grids():
                    s.profile_begin()
                    s.transfer_tensor(x, layout="nhwc")
                    s.profile_end()
                    s.sync()
                    return s.profile_grids()
                before = grids()
                tickets = [s.transfer_async(f) for f in frames]
                got = np.stack([s.result(t).copy() for t in tickets])
                assert grids() == before                      # the tickets' own shares are gone
                for bad in (0, 5, -1):
                    with pytest.raises(pkg.RRVError):
                        s.set_grid_share(bad)
                assert grids() == before
                if g == (256, 1):
                    for share, r in ((2, 128), (3, 80), (4, 64)):       # whole XCD rows of 256 / share workgroups
                        s.set_grid_share(share)
                        assert max(gr for gr, xcd in grids() if xcd >= 0) == r, share
                    s.set_grid_share(1)
                    assert grids() == before
            if want is None:
                want = got
            np.testing.assert_array_equal(got, want)
        finally:
            if g not in last_handles:
                s.close()

"""The item walks of the persistent kernels, on the CPU: tests/grid_ref.py is a MODEL of the walk arithmetic of conv_f43_k, conv_wino_k
(upsample-fused), conv_wino_split_k and conv_last_k — not the kernels.  The sweep asserts that on every grid a caller can provoke
(RRV_CUS, a CU mask, rrv_set_grid_share, look-ahead tickets) each item is visited exactly once, every coordinate stays in range and the
walk ends; it guards later edits of the walk.  What the KERNELS do on such grids is tests/test_gpu_grid_independence.py's business;
WALKS below says which of its tests runs each persistent instantiation in each class of walk, and is kept equal to the kernel ledger
here and to what the GPU module saw there."""
import os

import pytest

import grid_ref as GR
import kernel_ledger as KL

GRIDS = list(range(1, 70)) + [80, 96, 128, 256]
SLABS = (1, 2, 4, 8, 16)


@pytest.mark.parametrize("slabs", SLABS)
def test_transform_domain_walk_visits_every_item_once(slabs):
    cases = 0
    for grid in GRIDS:
        xcd = GR.host_xcd_slabs(grid, slabs)
        for tiles_x in range(1, 6):
            for tiles_y in range(1, 5):
                for B in range(1, 4):
                    seen = set()
                    for chain in GR.td_walk(grid, xcd, tiles_x, tiles_y, B, slabs):       # (td_chain asserts that it ends)
                        for tx, ty, b, nt in chain:
                            assert 0 <= tx < tiles_x and 0 <= ty < tiles_y and 0 <= b < B and 0 <= nt < slabs, (grid, tiles_x, tiles_y, B)
                            assert (tx, ty, b, nt) not in seen, (grid, tiles_x, tiles_y, B, (tx, ty, b, nt))
                            seen.add((tx, ty, b, nt))
                    assert len(seen) == tiles_x * tiles_y * B * slabs, (grid, tiles_x, tiles_y, B)
                    cases += 1
    assert cases == len(GRIDS) * 5 * 4 * 3 == 4380


def test_xcd_walk_keeps_the_slabs_of_a_tile_on_one_xcd():
    """What xcd_slabs is for (conv_wino.h:201-205): the slabs of a pixel tile run on workgroups of one XCD (w % 8), and no chain
    changes its slab."""
    for grid, slabs in ((64, 8), (128, 16), (128, 4), (16, 2), (8, 1)):
        assert GR.host_xcd_slabs(grid, slabs)
        where = {}
        for w, chain in enumerate(GR.td_walk(grid, 1, 5, 4, 3, slabs)):
            assert len({it[3] for it in chain}) <= 1
            for tx, ty, b, nt in chain:
                where.setdefault((tx, ty, b), set()).add(w % 8)
        assert all(len(x) == 1 for x in where.values())


def test_conv_last_walks_visit_every_tile_once():
    for ntiles in range(1, 300):
        for cus in list(range(1, 18)) + [24, 64, 256]:
            grid = min(ntiles, 4 * cus)
            tiles = sorted(t for chain in GR.last_walk(grid, ntiles) for t in chain)
            assert tiles == list(range(ntiles)), (grid, ntiles)


def test_classes_of_the_module_s_grids():
    """The arithmetic behind the configurations of the GPU module (136 x 200 frames, three per launch): the 1/8 level has 2 x 2 tiles
    of 16 x 16 per image, twelve tile-images."""
    assert GR.td_classes(5, GR.host_xcd_slabs(5, 16), 2, 2, 3, 16, False) == {"C"}
    assert GR.td_classes(24, GR.host_xcd_slabs(24, 8), 2, 2, 3, 8, False) == {"B"}
    assert GR.td_classes(24, GR.host_xcd_slabs(24, 16), 2, 2, 3, 16, False) == {"C"}
    assert GR.td_classes(80, GR.host_xcd_slabs(80, 16), 2, 2, 3, 16, True) == {"B", "I"}
    assert GR.td_classes(128, GR.host_xcd_slabs(128, 16), 2, 2, 3, 16, False) == {"A"}
    assert GR.td_classes(64, GR.host_xcd_slabs(64, 8), 2, 2, 3, 8, False) == {"A"}
    assert GR.td_classes(96, GR.host_xcd_slabs(96, 8), 2, 2, 3, 8, False) == set()           # 96 items on 96 workgroups: no chain
    assert GR.td_classes(5, 0, 2, 2, 3, 1, True) == {"B", "I"} and GR.td_classes(3, 0, 2, 2, 1, 1, True) == {"B"}
    assert GR.last_classes(20, 351) == {"rr"} and GR.last_classes(96, 351) == {"band"} and GR.last_classes(351, 351) == set()


# ---- which GPU test runs which instantiation in which walk ---------------------------------------------------------------------------------
# Classes (grid_ref.td_classes): A the XCD walk with a chain of two or more items; B the plain walk with grid % slabs == 0 and a chain;
# C the plain walk with grid % slabs != 0: the slab changes inside a chain and the kernel re-stages its epilogue parameters; I, for the
# launches with per-image state only: the image changes inside a chain (the same re-stage, and the per-image weights).  conv_last_k:
# band (one band of tiles per XCD) and rr (round robin), each with two or more tiles per workgroup.
# A value is the test that runs the class, or the reason why the class does not occur ("no: ...").
T = "tests/test_gpu_grid_independence.py::"
WALKS = {}


def _row(keys, **classes):
    for k in ([keys] if isinstance(keys, str) else keys):
        assert k not in WALKS, k
        WALKS[k] = dict(classes)


ONE_SLAB = "no: one cout slab (32 couts) wherever this instantiation is launched, so the slab cannot change"
G0, G2, GRP, BLD, FRM, BIG, PRE, OUT = (T + n for n in ("test_global_mode0", "test_global_mode2", "test_grouped_per_image_state", "test_blended_frames_per_image_state",
                                                            "test_frame_mode", "test_frame_mode_unsplit_filter_down", "test_preparation_pass", "test_output_forms"))
# (A test is cited where it runs the class under every kernel family: the F(2x2,3x3) encoder rows from frame mode, which never runs F(4x4,3x3).)
# conv_wino_split_k<EPI, PERIMG>
_row(["conv_wino_split_k<1, 0>", "conv_wino_split_k<65, 0>"], A=FRM, B=FRM, C=FRM)
_row(["conv_wino_split_k<5, 0>", "conv_wino_split_k<54, 0>", "conv_wino_split_k<8, 0>", "conv_wino_split_k<40, 0>"], A=G0, B=G0, C=G0)
_row("conv_wino_split_k<0, 0>", A=G0, B=G0, C=G0)
_row("conv_wino_split_k<2, 0>", A=FRM, B=FRM, C=FRM)
_row(["conv_wino_split_k<54, 1>", "conv_wino_split_k<0, 1>", "conv_wino_split_k<8, 1>", "conv_wino_split_k<40, 1>"], A=GRP, B=GRP, C=GRP, I=GRP)
_row("conv_wino_split_k<5, 1>", A=BLD, B=BLD, C=BLD, I=BLD)
_row("conv_wino_split_k<2, 1>", A=BIG, B=BIG, C=ONE_SLAB, I=BIG)
# the upsample-fused conv_wino_k<EPI, 0, 4, 1, SC, PERIMG>
_row("conv_wino_k<6, 0, 4, 1, 1, 0>", A=G0, B=G0, C=G0)
_row("conv_wino_k<6, 0, 4, 1, 1, 1>", A=GRP, B=GRP, C=GRP, I=GRP)
_row("conv_wino_k<2, 0, 4, 1, 1, 0>", A=FRM, B=FRM, C=FRM)
_row("conv_wino_k<2, 0, 4, 1, 0, 0>", A=PRE, B=PRE, C=PRE)
# conv_f43_k<EPI, LAY>
_row(["conv_f43_k<1, 0>", "conv_f43_k<65, 0>", "conv_f43_k<65, 3>", "conv_f43_k<1, 3>", "conv_f43_k<65, 1>"], A=G2, B=G2, C=G2)
# ResidualBlock.conv2: the one conv_f43_k layer that a launch with per-image state reaches (it reads ConvP::par_bstride itself)
_row(["conv_f43_k<54, 0>", "conv_f43_k<54, 1>"], A=G2, B=G2, C=G2, I=GRP)
# conv_last_k<U8, CHW, SPACE, YUV, Y16>
_row([k for k in KL.LEDGER if k.startswith("conv_last_k")], band=OUT, rr=OUT)

PERSISTENT = ("conv_f43_k", "conv_wino_k", "conv_wino_split_k", "conv_last_k")
CLASSES = {"conv_last_k": {"band", "rr"}}


def expected(forced):
    """{symbol: {class: test}} of the classes that are run; forced = RRV_F43 of a suite on one kernel family ('0' / '2' drop the
    rows only the other family's fixed mode launches)."""
    out = {}
    for sym, classes in WALKS.items():
        if forced == "0" and sym.startswith("conv_f43_k"):
            continue
        if forced == "2" and sym in F23_OF_PACKED_LAYERS:
            continue
        run = {c: t for c, t in classes.items() if not t.startswith("no: ")}
        if run:
            out[sym] = run
    return out


# F(2x2,3x3) instantiations that only a mode-0 launch of a layer with an F(4x4,3x3) pack reaches
F23_OF_PACKED_LAYERS = {"conv_wino_split_k<54, 0>", "conv_wino_split_k<54, 1>"}


def test_walks_and_ledger_are_equal_both_ways():
    reachable = {k for k, e in KL.LEDGER.items() if k.startswith(tuple(p + "<" for p in PERSISTENT)) and e[0] != "unreachable"}
    assert reachable - set(WALKS) == set(), "persistent instantiations without a row"
    assert set(WALKS) - reachable == set(), "rows for kernels the ledger does not list as reachable"


def test_rows_are_well_formed_and_cited_tests_exist():
    mod = None
    for sym, classes in WALKS.items():
        fam = sym.split("<")[0]
        per_image = sym.startswith("conv_f43_k<54, ") or fam not in ("conv_f43_k", "conv_last_k") and sym.endswith(", 1>")
        want = CLASSES.get(fam, {"A", "B", "C"} | ({"I"} if per_image else set()))
        assert set(classes) == want, (sym, sorted(classes))
        for c, t in classes.items():
            if t.startswith("no: "):
                assert len(t) > 10, (sym, c)
                continue
            path, name = t.split("::")
            assert os.path.isfile(os.path.join(KL.ROOT, path)), t
            if mod is None:
                with open(os.path.join(KL.ROOT, path)) as f:
                    mod = f.read()
            assert ("\ndef %s(" % name) in mod, t       # (the module imports torch: read, not imported)
    assert expected("0").keys() < expected(None).keys() and expected("2").keys() < expected(None).keys()

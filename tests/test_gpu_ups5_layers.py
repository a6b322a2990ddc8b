"""The shortcut-fused ResidualBlock.conv1 (the five-product form, csrc/conv_ups5.h) against a float64 reference of its own
GPU input (tests/layer_ref.py): both outputs of the kernel, the conv1 activation a* and the low-resolution shortcut xs*, at
the headline's decoder shapes (a 640 x 640 frame: 80^2 -> 160^2, 160^2 -> 320^2, 320^2 -> 640^2) and at odd sizes whose
low-resolution tensors end inside a 16 x 16 work item (masked edges)."""
import pytest

import layer_ref as LR
from state_bounds import load_golden
from test_gpu_layers import check_image, frames_for, launch

pytestmark = pytest.mark.gpu

CONV1 = ("xs4", "a4", "xs3", "a3", "xs2", "a2")
SHAPES = [(1, 640, 640), (2, 141, 203), (1, 9, 15)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_conv1_and_shortcut_against_their_own_input(pkg, weights, shape):
    B, H, W = shape
    blob = load_golden("global_a")["state"]
    st = LR.parse_state(blob)
    frames = frames_for(pkg, B, H, W)
    s, seq, _ = launch(pkg, weights, frames, blob, 2, p8=3)
    try:
        assert sum(n.startswith("conv_upw_sc") for n, _ in seq) == 3, seq
        for b in sorted({0, B - 1}):
            fam, _ = check_image(s, weights, st, seq, H, W, b, frames[b], names=CONV1)
            assert all(fam[n] == "ups" for n in CONV1), fam
    finally:
        s.close()

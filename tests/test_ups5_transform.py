"""The five-product transform of the shortcut-fused ResidualBlock.conv1 kernel (csrc/conv_ups5.h), checked in float64:
the coefficient table the kernel is generated from (struct Ups5Tab) reproduces "nearest x2, then 3x3 conv" in 1-D and 2-D, and the four shortcut positions
reproduce up(conv1x1(x)).  No GPU."""
import ast
import os
import re

import numpy as np

HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rerevst-code_amd", "csrc", "conv_ups5.h")


def _table():
    """The arrays of struct Ups5Tab, from which the kernel's pack, input transform and output transform are generated."""
    src = open(HDR).read()
    body = re.search(r"struct Ups5Tab \{(.*?)\n\};", src, re.S).group(1)

    def get(name):
        m = re.search(r"static constexpr int " + name + r"(?:\[\d+\])+ = (\{.*?\});", body, re.S)
        return np.array(ast.literal_eval(m.group(1).replace("{", "[").replace("}", "]")), float)

    G = get("G2") / 2
    BT4, DS = get("BT4"), get("DS").astype(int)
    return G, BT4[DS], get("AT")


G, BT, AT = _table()
DS = (0, 1, 2, 2, 3)       # data slot of each product row (rows 2 and 3 share x2 - x1)


def test_table_shape_and_shared_rows():
    assert G.shape == (5, 3) and BT.shape == (5, 4) and AT.shape == (4, 5)
    assert np.array_equal(BT[2], BT[3])
    assert len({tuple(r) for r in BT}) == 4


def test_one_axis_exact():
    rng = np.random.default_rng(1)
    for _ in range(200):
        x, g = rng.standard_normal(4), rng.standard_normal(3)
        u = np.array([x[0], x[1], x[1], x[2], x[2], x[3]])
        want = np.array([u[k:k + 3] @ g for k in range(4)])
        np.testing.assert_allclose(AT @ ((G @ g) * (BT @ x)), want, rtol=0, atol=1e-13)


def test_two_axes_exact_upsample_conv():
    rng = np.random.default_rng(2)
    C = 8
    for _ in range(20):
        X, W = rng.standard_normal((C, 4, 4)), rng.standard_normal((C, 3, 3))
        up = np.repeat(np.repeat(X, 2, 1), 2, 2)
        want = np.array([[np.sum(up[:, 1 + i:4 + i, 1 + j:4 + j] * W) for j in range(4)] for i in range(4)])
        U = np.einsum("ia,cab,jb->cij", G, W, G)
        V = np.einsum("ia,cab,jb->cij", BT, X, BT)
        # the kernel keeps 16 distinct V values per channel: V[s(i)][s(j)]
        V16 = np.einsum("ia,cab,jb->cij", BT[[0, 1, 2, 4]], X, BT[[0, 1, 2, 4]])
        assert np.allclose(V, V16[:, DS][:, :, DS])
        got = AT @ np.sum(U * V, 0) @ AT.T
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_shortcut_positions_reproduce_up_conv1x1():
    rng = np.random.default_rng(3)
    C = 16
    X, Wsc = rng.standard_normal((C, 4, 4)), rng.standard_normal(C)
    V = np.einsum("ia,cab,jb->cij", BT[[0, 1, 2, 4]], X, BT[[0, 1, 2, 4]])      # slots: a, m, d, e
    P = {k: np.sum(Wsc / 4 * V[:, r, c]) for k, (r, c) in {"mm": (1, 1), "md": (1, 2), "dm": (2, 1), "dd": (2, 2)}.items()}
    for a, sa in ((0, -1), (1, 1)):
        for b, sb in ((0, -1), (1, 1)):
            got = P["mm"] + sb * P["md"] + sa * P["dm"] + sa * sb * P["dd"]
            want = np.sum(Wsc * X[:, 1 + a, 1 + b])      # conv1x1 at low-res pixel (a, b); up() repeats it over 2x2 outputs
            assert abs(got - want) < 1e-12

"""Five-product transform of "nearest x2, then 3-tap conv" (ResidualBlock.conv1, conv_ups5.h).

Per axis the low-resolution pixels x0..x3 (x1, x2 = the tile) give four outputs, y_k = [u_k, u_k+1, u_k+2] . g with
u = (x0, x1, x1, x2, x2, x3).  A rank-5 decomposition y = A^T [(G g) * (B^T x)] with data rows
(x0 + a x1 + b x2, d, d, c x1 + e x2, x3 + f x1 + h x2), d = x2 - x1, exists along a one-parameter family (delta below,
solved by hand from the output equations); delta = 1/2 makes every data and output coefficient 0 / +-1 and the
weight coefficients halves.  This script rebuilds the family, checks exactness in float64 and ranks members by an
fp32 error study against today's 3-products-per-pixel form (sequential fp32 accumulation over Cin, U rounded once).

    python tools/ups5_search.py [--patches 300] [--cin 128 256 512]      (profiles/r07_ups5_search.txt)
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the table conv_ups5.h uses
G = np.array([[1, 0, 0], [.5, .5, .5], [-.5, -.5, .5], [-.5, .5, .5], [0, 0, 1]])
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], float)
AT = np.array([[1, 1, 0, -1, 0], [0, 1, 1, 0, 0], [0, 1, 0, 1, 0], [0, 1, -1, 0, 1]], float)


def family(delta):
    """G, B^T, A^T of family member delta (delta != 0, 1)."""
    beta = -delta / (1 - delta); alpha = -1 - beta
    zeta = (1 - 2 * delta) / delta; eps = -1 - zeta
    s = np.array([1., 1., 1.])
    w1 = np.array([0., 0., 1.]) - delta * s               # g2 - delta s
    w2 = np.array([0., 1., 1.]) - delta * s               # g1 + g2 - delta s
    Gm = np.array([[1, 0, 0], (1 - delta) * s, w1, w2, [0, 0, 1]])      # the m product scaled so that its data row starts with 1
    Bm = np.array([[1, alpha, beta, 0], [0, 1, delta / (1 - delta), 0], [0, -1, 1, 0], [0, -1, 1, 0], [0, eps, zeta, 1]])
    # y0 = Pa + Pm + f3 d, y1 = Pm + w1 d, y2 = Pm + w2 d, y3 = Pe + Pm + f4 d; f3, f4 in span(w1, w2)
    f3 = -beta * np.array([1., 0, 0]) - delta * s
    f4 = np.array([1., 1, 0]) - zeta * np.array([0, 0, 1.]) - delta * s
    c3 = np.linalg.lstsq(np.stack([w1, w2], 1), f3, rcond=None)[0]
    c4 = np.linalg.lstsq(np.stack([w1, w2], 1), f4, rcond=None)[0]
    Am = np.array([[1, 1, c3[0], c3[1], 0], [0, 1, 1, 0, 0], [0, 1, 0, 1, 0], [0, 1, c4[0], c4[1], 1]])
    return Gm, Bm, Am


def direct1(x, g):
    u = np.array([x[0], x[1], x[1], x[2], x[2], x[3]])
    return np.array([u[k:k + 3] @ g for k in range(4)])


def ref2(X, W):
    up = np.repeat(np.repeat(X, 2, 1), 2, 2)
    return np.array([[np.sum(up[:, 1 + i:4 + i, 1 + j:4 + j] * W) for j in range(4)] for i in range(4)])


def fp32_form(X, W, Gm, Bm, Am):
    f = np.float32
    U = np.einsum('ia,cab,jb->cij', Gm, W, Gm).astype(f)
    V = np.einsum('ia,cab,jb->cij', Bm.astype(f), X.astype(f), Bm.astype(f)).astype(f)
    M = np.zeros(U.shape[1:], f)
    for c in range(X.shape[0]):
        M = (M + U[c] * V[c]).astype(f)
    return Am.astype(f) @ M @ Am.T.astype(f)


def fp32_today(X, W):
    G0 = np.array([[1, 1, 1], [1, 0, 0], [0, 0, 1]], float)
    B0 = np.array([[0, 1, 0], [1, -1, 0], [0, -1, 1]], float)
    A0 = np.array([[1, 1, 0], [1, 0, 1]], float)
    out = np.zeros((4, 4))
    for py in range(2):
        for px in range(2):
            out[2 * py:2 * py + 2, 2 * px:2 * px + 2] = fp32_form(X[:, py:py + 3, px:px + 3], W, G0, B0, A0)
    return out


def study(form, cin, patches, rng, weights=None):
    err = []
    for _ in range(patches):
        z = rng.standard_normal((cin, 4, 4))
        X = np.maximum(z, 0.2 * z)                            # post-norm, leaky
        W = weights[rng.integers(len(weights))] if weights is not None else rng.standard_normal((cin, 3, 3)) * 0.05
        r = ref2(X, W)
        err.append(np.abs(form(X, W) - r).max() / np.abs(r).max())
    err = np.array(err)
    return err.max(), np.sqrt(np.mean(err ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=300)
    ap.add_argument("--cin", type=int, nargs="+", default=[128, 256, 512])
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    assert np.allclose(family(0.5)[0], G) and np.allclose(family(0.5)[1], BT) and np.allclose(family(0.5)[2], AT)
    for delta in (0.5, 0.25, 0.75, 1 / 3, 2 / 3):
        Gm, Bm, Am = family(delta)
        ex = max(np.abs(Am @ ((Gm @ g) * (Bm @ x)) - direct1(x, g)).max()
                 for x, g in ((rng.standard_normal(4), rng.standard_normal(3)) for _ in range(100)))
        line = "delta %.4f  exact %.1e" % (delta, ex)
        for cin in a.cin:
            mx, rms = study(lambda X, W: fp32_form(X, W, Gm, Bm, Am), cin, a.patches, rng)
            line += "  | Cin %d max %.2e rms %.2e" % (cin, mx, rms)
        print(line)
    line = "today (3 products / pixel)"
    for cin in a.cin:
        mx, rms = study(fp32_today, cin, a.patches, rng)
        line += "  | Cin %d max %.2e rms %.2e" % (cin, mx, rms)
    print(line)
    # the x4-decoder weight set of the parity fixtures (tests/golden/global_a_dec4.npz names it; weights.weight_variant builds it)
    sys.path.insert(0, ROOT)
    wv = importlib.import_module("rerevst-code_amd").weight_variant("dec4")
    Gm, Bm, Am = family(0.5)
    for blk in ("slice4", "slice3", "slice2"):
        w = np.asarray(wv["Decoder.%s.conv1.weight" % blk], np.float64)      # [Cout][Cin][3][3]
        cin = w.shape[1]
        line = "x4-decoder %s.conv1 (Cin %d)" % (blk, cin)
        for name, form in (("delta 1/2", lambda X, W: fp32_form(X, W, Gm, Bm, Am)), ("today", fp32_today)):
            mx, rms = study(form, cin, a.patches, np.random.default_rng(1), weights=w)
            line += "  | %s max %.2e rms %.2e" % (name, mx, rms)
        print(line)
    print("chosen: delta = 1/2\nG =", G.tolist(), "\nB^T =", BT.tolist(), "\nA^T =", AT.tolist())


if __name__ == "__main__":
    main()

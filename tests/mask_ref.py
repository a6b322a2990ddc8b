"""Numpy float32 reference of the masked multi-style transfer (rrv_transfer_image_mask_device, rrv_transfer_mask_batch), built
from the oracle's own operations.  Test infrastructure, as the oracle is.

The model: S computed states (the oracle's get_state blobs), a float32 mask M[S][H][W] at the resolution of the network's
input frame.  For a decoder tensor at stride r in {1, 2, 4, 8} of that frame m_s(y, x) is the mean of M[s] over the r x r
block of input pixels the tensor pixel covers, taken as successive 2 x 2 means ((a + b) + (c + d)) * 0.25 in float32.  Every
saved quantity is blended at a tensor pixel p of its level as q(p)[c] = sum_s m_s(p) q_s[c] (s ascending, float32) and
Decoder.run(compute=False) uses q(p) where it used q: clamp((x - mean(p)) rstd(p), lo(p), hi(p)), the AdaIN affine
* std(p) + mean(p), apply_filter with F1(p) on down_sample's output before the LeakyReLU and F2(p) on that result before the
upsample convolution.  The encoder does not see the mask.
"""
import numpy as np

import rerevst_oracle as O

F32 = np.float32


def halve(m):
    """[..., h, w] -> [..., h/2, w/2]: ((a + b) + (c + d)) * 0.25, a b the upper row of each 2 x 2 block"""
    a, b, c, d = m[..., 0::2, 0::2], m[..., 0::2, 1::2], m[..., 1::2, 0::2], m[..., 1::2, 1::2]
    return (((a + b) + (c + d)) * F32(0.25)).astype(F32)


def level_masks(mask):
    """mask [S][H][W] float32 for the network's input frame -> the masks at stride 1, 2, 4, 8: [S][H/r][W/r] over the
    8*(H/8) x 8*(W/8) pixels the decoder returns (rows and columns beyond are ignored, as the frame's are)"""
    mask = np.asarray(mask)
    assert mask.dtype == np.float32 and mask.ndim == 3
    H, W = mask.shape[1] // 8 * 8, mask.shape[2] // 8 * 8
    lv = [np.ascontiguousarray(mask[:, :H, :W])]
    for _ in range(3):
        lv.append(halve(lv[-1]))
    return lv


def pad_mask(mask, PH, PW):
    """the mask of an unpadded frame behind oracle.reflect_pad (edge-inclusive reflection, 64 pixels on top and left)"""
    S, H, W = mask.shape
    return np.ascontiguousarray(O.reflect_pad(mask.transpose(1, 2, 0), PH, PW).transpose(2, 0, 1))


def blend(m, rows):
    """m [S][h][w], rows: S arrays [C] -> [1][h][w][C] = sum_s m_s(p) * rows_s, s ascending, float32 products and sums"""
    out = np.zeros(m.shape[1:] + (rows[0].shape[0],), F32)
    for s in range(m.shape[0]):
        out = out + m[s][..., None] * rows[s][None, None, :]
    return out[None].astype(F32)


def _unpack(blob):
    t = O.Stylization({})
    t.set_state(np.asarray(blob, F32))
    norms = list(t.dec.norm) + [n for b in ("slice4", "slice3", "slice2") for n in t.dec.bnorm[b]]
    return dict(norm=norms, filt=[t.dec.filters[n] for n in O.FILTER_NAMES], sty=[t.F_style[n] for n in O.STYLE_NAMES])


class MaskedDecoder:
    """Decoder.run(compute=False) of the oracle with every saved quantity blended per pixel."""

    def __init__(self, net, states):
        self.net = net
        self.st = [_unpack(b) for b in states]
        self.S = len(states)

    def _w(self, k):
        return self.net.w["Decoder." + k]

    def _norm(self, x, n, m):
        q = [blend(m, [getattr(st["norm"][n], f) for st in self.st]) for f in ("mean", "rstd", "lo", "hi")]
        y = (x - q[0]) * q[1]
        return np.minimum(q[3], np.maximum(q[2], y)).astype(F32)

    def _adain(self, x, n, sty, m):
        y = self._norm(x, n, m)
        return (y * blend(m, [st["sty"][sty][1] for st in self.st]) + blend(m, [st["sty"][sty][0] for st in self.st])).astype(F32)

    def _apply(self, x, k, m):
        """apply_filter with F(p) = sum_s m_s(p) F_s: out[p][i] = sum_j F(p)[i][j] x[p][j]"""
        F = np.zeros(m.shape[1:] + (32, 32), F32)
        for s in range(self.S):
            F = F + m[s][..., None, None] * self.st[s]["filt"][k][None, None]
        return np.einsum("hwij,hwj->hwi", F.astype(F32), x[0]).astype(F32)[None]

    def _kernel_filter(self, f, x, m):
        p = "Filter%d." % (f + 1)
        d = O.conv3x3(x, self._w(p + "down_sample.0.weight"), self._w(p + "down_sample.0.bias"))
        d = O.lrelu(self._apply(d, 2 * f, m))
        d = self._apply(d, 2 * f + 1, m)
        return x + O.conv3x3(d, self._w(p + "upsample.0.weight"), self._w(p + "upsample.0.bias"))

    def _resblock(self, blk, n1, n2, x, m):
        x = O.upsample2(x)
        xs = O.conv1x1(x, self._w(blk + ".conv_shortcut.weight"))
        h = O.lrelu(O.conv3x3(x, self._w(blk + ".conv1.weight"), self._w(blk + ".conv1.bias")))
        h = self._norm(h, n1, m)
        h = O.lrelu(O.conv3x3(h, self._w(blk + ".conv2.weight"), self._w(blk + ".conv2.bias")))
        h = self._norm(h, n2, m)
        return xs + h

    def run(self, x, lv):
        """x: raw relu4_1 feature [1][h][w][512]; lv: level_masks(...)"""
        h = self._norm(x, 0, lv[3])
        for f in range(3):
            h = self._kernel_filter(f, h, lv[3])
        h = self._adain(h, 1, 3, lv[3])
        h = self._resblock("slice4", 5, 6, h, lv[2])
        h = self._adain(h, 2, 2, lv[2])
        h = self._resblock("slice3", 7, 8, h, lv[1])
        h = self._adain(h, 3, 1, lv[1])
        h = self._resblock("slice2", 9, 10, h, lv[0])
        h = self._adain(h, 4, 0, lv[0])
        return O.conv3x3(h, self._w("slice1.weight"), self._w("slice1.bias"))


PATCHES = ((0, 2), (1,), (0, 1), (1, 2))      # the multistyle_s4 setup's frames that style k's state is computed over


def distinct_states(s, padded):
    """Four computed states of the multistyle_s4 setup (its handle `s` with style 0's state computed, closed here, and its padded
    frames), style k's over the frames PATCHES[k]: style 0's is the setup's own.  Decoder.norm[0] holds statistics of the sampled
    CONTENT alone, so states computed over one set of frames share it to the bit; a blend of such states holds the same value
    there under any weights, masks or style order, and a check of c41 could then see no wrong image, mask or style index.  Every
    pair of these differs there by more than 1e-4 relative (asserted)."""
    import layer_ref as LR
    feats = [s.generate_content_features(p) for p in padded]
    blobs = [s.get_state(0).copy()]
    for k in range(1, 4):
        s.clean()
        for i in PATCHES[k]:
            s.add_patch(feats[i])
        s.compute_norm()
        blobs.append(s.get_state(k).copy())
    s.close()
    mean0 = [LR.parse_state(b)["norm"][0][0] for b in blobs]
    for i in range(4):
        for j in range(i):
            assert np.abs(mean0[i] - mean0[j]).max() > 1e-4 * np.abs(mean0[i]).max(), (i, j)
    return blobs


def transfer(net, states, frame_bgr_u8, mask, return_preclamp=False):
    """frame [H][W][3] uint8 BGR (the network's input frame, already padded), mask [S][H][W] float32 -> the stylized frame
    [8*(H/8)][8*(W/8)][3] float32 BGR in 0..255, or the pre-clamp network output [1][..][..][3]"""
    feat = net.encoder(O.rgb2gray(O.image_to_tensor(frame_bgr_u8)))
    y = MaskedDecoder(net, states).run(feat, level_masks(mask))
    return y if return_preclamp else O.tensor_to_image(y)

"""Float64 references for the 14 sync points of the once-per-video preparation pass (prepare_style, add, compute: resident and
streaming), one function per sync point, and the bounds they are held to.  Plain module (no pytest): imported by
tests/test_gpu_prep_layers.py and tests/test_layer_ref.py.  The operators, `check` and the magnitude model are layer_ref's.

A pass ended at sync point s (rrv_debug_prep_stop) leaves its workspace and the blob as far as it got.  Every check is teacher
-forced on what the GPU held: a convolution on its own input tap, a statistic on its own raw tap, a predicted filter on the
tap (or the float64 convolution of the tap) it averaged, a normalised tensor on the raw tensor THE PREVIOUS STOP'S RUN left at
the same place (the pass normalises in place and has no atomics, so two runs hold the same bits: the caller asserts that the
blob entries of the stages before s are bit-equal between the two runs first) and the blob's own statistics.

What a tensor holds after the run that stopped at s (resident pass; B images unless noted):
  0        content raw.                                                      norm[0] <- content
  1 + f    IN = (cn, nxt, cn)[f] the filter's input, intact; t32 = F2.down_sample(IN) (F1's was overwritten); d32, u of image 0;
           OUT = (nxt, cn, nxt)[f] = IN + u for every image (quirk Q1).      Filter f.F1, .F2 <- means + FC
  4        nxt raw.                                                          norm[1] <- nxt
  5 + 3k   the block's input (nxt / o[k-1]) normalised + AdaIN in place; a[k] raw.          norm[n1] <- a[k]
  6 + 3k   a[k] normalised in place; o[k] raw = LeakyReLU(conv2).                           norm[n2] <- o[k]
  7 + 3k   xs[k] = the 1 x 1 shortcut of the block's input; o[k] = norm2(raw) + up(xs[k]).  norm[nada] <- o[k]
The streaming pass re-runs this prefix per group; with ONE group the same tensors hold the same things except at the filter
stages, where the group's residual add has not run yet and frame 0's chain is f0 (its stored feature) -> cn[0] (norm[0], then
the earlier residuals su[0..f-1] added in place) -> d32 -> su[f].

Bounds: |gpu - ref| <= K_family 2^-24 m + 2^-24 |ref| on every element (LR.check), with three families of this module:
  pstat   a statistic against the float64 statistic of its raw tap x over (B, H, W):
            mean      m = mean |x|
            variance  var_gpu recovered as 1 / rstd^2 - 1e-8 (style: std^2 - 1e-5), m = mean (|x| + |mean|)^2 + the epsilon
            lo, hi    a float32 minimum is exact: (min_tap - mean_gpu) rstd_gpu from the tap's exact extremum and the blob's own
                      mean and rstd, within that expression's two float32 roundings, 2^-23 relative.  No K.
  gemm    conv_mfma_k raw outputs (the 512 -> 32 predictor convolutions, the 1 x 1 shortcuts as their own launch).
  ppred   chan_stat_k's mean + fc_filter_k: the FC of [mean of a tap, cached style half], m the same on absolute values.  Where the
          averaged tensor is gone (F1's t32; the streamed groups) the float64 convolution of its input stands in and its
          per-element bound b enters as |W_fc| mean(b), as in the frame-mode statistic checks.
The existing families keep their K: f23 (d32, u, conv2), ups (conv1 behind the upsample), point (every pointwise_k result).
"""
import numpy as np

import layer_ref as LR
from layer_ref import U, EPS32, RES, check, conv1, conv3, fold_up, lrelu

EPS_STY = float(np.float32(1e-5))
N_STOPS = 14
FILTER_IO = (("cn", "nxt"), ("nxt", "cn"), ("cn", "nxt"))
BLOCKS = (("slice4", "xs4", "a4", "o4"), ("slice3", "xs3", "a3", "o3"), ("slice2", "xs2", "a2", "o2"))
BLOCK_IN = ("nxt", "o4", "o3")
STYLE_TAPS = ("style_c11", "style_c21", "style_c31", "style_c41")


def whole(H):
    return [(0, H)]


# ---- the blob ------------------------------------------------------------------------------------------------------------

def _offsets():
    off, o = {}, 0
    for i, C in enumerate(LR.NORM_CH):
        off["norm", i] = (o, 4 * C)
        o += 4 * C
    for i in range(6):
        off["filt", i] = (o, 1024)
        o += 1024
    for i, C in enumerate(LR.STYLE_CH):
        off["sty", i] = (o, 2 * C)
        o += 2 * C
    return off


OFFSETS = _offsets()


def stage_entries(stop):
    """The blob entries the sync point `stop` writes."""
    if stop == 0:
        return [("norm", 0)]
    if stop <= 3:
        return [("filt", 2 * (stop - 1)), ("filt", 2 * (stop - 1) + 1)]
    if stop == 4:
        return [("norm", 1)]
    k, j = divmod(stop - 5, 3)
    return [("norm", RES[BLOCKS[k][0]][j])]


def entries_bit_equal(blob_a, blob_b, stop):
    """Whether the entries of every stage before `stop` (and the style statistics) hold the same bits in the two blobs."""
    a, b = (np.ascontiguousarray(x, np.float32).view(np.uint32) for x in (blob_a, blob_b))
    keys = [e for t in range(stop) for e in stage_entries(t)] + [("sty", i) for i in range(4)]
    return all(np.array_equal(a[o:o + n], b[o:o + n]) for o, n in (OFFSETS[k] for k in keys))


# ---- statistics -------------------------------------------------------------------------------------------------------------

def raw_stats(x):
    """Float64 statistics of a raw tap x [..., C] over everything but the channel: the values and their magnitudes."""
    x = np.asarray(x, np.float64).reshape(-1, np.shape(x)[-1])
    mean = x.mean(axis=0)
    ax = np.abs(x)
    return {"n": x.shape[0], "mean": mean, "var": x.var(axis=0), "lo": x.min(axis=0), "hi": x.max(axis=0),
            "m_mean": ax.mean(axis=0), "m_var": ((ax + np.abs(mean)) ** 2).mean(axis=0)}


def _pstat(em, bm, sm, ev, bv, sv, extra_ok=True):
    ok = bool(np.all(em <= bm) and np.all(ev <= bv) and extra_ok)
    worst = max(float((em / np.maximum(bm, 1e-300)).max()), float((ev / np.maximum(bv, 1e-300)).max()))
    if not extra_ok:
        worst = max(worst, np.inf)
    ratio = max(float((em / np.maximum(sm, 1e-300)).max()), float((ev / np.maximum(sv, 1e-300)).max()))
    return ok, worst, ratio


def check_pstat(entry, rs, k):
    """A norm entry (mean, rstd, lo, hi) against raw_stats() of its tap: (passes, worst fraction of a bound, ratio)."""
    mean_g, rstd_g, lo_g, hi_g = entry
    em, sm = np.abs(mean_g - rs["mean"]), U * rs["m_mean"]
    var_g = 1.0 / (rstd_g * rstd_g) - EPS32
    ev, sv = np.abs(var_g - rs["var"]), U * (rs["m_var"] + EPS32)
    ends = True
    for got, ext in ((lo_g, rs["lo"]), (hi_g, rs["hi"])):
        ref = (ext - mean_g) * rstd_g
        ends = ends and bool(np.all(np.abs(got - ref) <= 2.0 * U * np.abs(ref)))
    return _pstat(em, k * sm + U * np.abs(rs["mean"]), sm, ev, k * sv + U * rs["var"], sv, ends)


def check_pstat_style(entry, rs, k):
    """A style entry (mean, std) against the unbiased statistic (+ 1e-5, sqrt) of its tap."""
    mean_g, std_g = entry
    f = rs["n"] / (rs["n"] - 1.0)
    em, sm = np.abs(mean_g - rs["mean"]), U * rs["m_mean"]
    ev, sv = np.abs(std_g * std_g - EPS_STY - f * rs["var"]), U * (f * rs["m_var"] + EPS_STY)
    return _pstat(em, k * sm + U * np.abs(rs["mean"]), sm, ev, k * sv + U * f * rs["var"], sv)


# ---- the pointwise steps in float64, on the blob's own statistics (no clamp: the pass has none) -----------------------------------

def normed(x, entry, sty=None):
    """(x - mean) rstd [* std + smean]: (v, m)."""
    x = np.asarray(x, np.float64)
    v, m = (x - entry[0]) * entry[1], (np.abs(x) + np.abs(entry[0])) * entry[1]
    if sty is not None:
        v, m = v * sty[1] + sty[0], m * np.abs(sty[1]) + np.abs(sty[0])
    return v, m


def added(x, r):
    x, r = np.asarray(x, np.float64), np.asarray(r, np.float64)
    return x + r, np.abs(x) + np.abs(r)


# ---- filter predictions ---------------------------------------------------------------------------------------------------------

def fc(w, name, cmean, cmag, smean):
    """FilterPredictor's FC on [content means, style half]: (filter [32, 32], magnitude, |W_content| for an input bound)."""
    p = "Decoder.%s.FC." % name
    W, bias = np.asarray(w[p + "weight"], np.float64), np.asarray(w[p + "bias"], np.float64)
    sm = np.asarray(smean, np.float64)
    v = W @ np.concatenate([cmean, sm]) + bias
    m = np.abs(W) @ np.concatenate([cmag, np.abs(sm)]) + np.abs(bias)
    return v.reshape(32, 32), m.reshape(32, 32), np.abs(W[:, :32])


def check_pred(got, w, name, cmean, cmag, smean, k, slack=None):
    """A predicted filter against fc(); slack [32]: a bound on how far the GPU's content means may be from cmean for reasons
    that are not this family's (the convolution's own rounding).  The ratio is the excess over that term."""
    v, m, Wc = fc(w, name, cmean, cmag, smean)
    s = 0.0 if slack is None else (Wc @ slack).reshape(32, 32)
    err = np.abs(np.asarray(got, np.float64) - v)
    bound = k * U * m + U * np.abs(v) + s
    return (bool(np.all(err <= bound)), float((err / np.maximum(bound, 1e-300)).max()),
            float((np.maximum(err - s, 0.0) / np.maximum(U * m, 1e-300)).max()))


def pred_conv(x, w, name, e=None):
    """FilterPredictor's down_sample on one image x [H, W, 512] in float64: (values, magnitudes, conv(|W|, e) for an input
    bound e), each [H W, 32]."""
    p = "Decoder.%s.down_sample.0." % name
    v, m = conv3(x, w[p + "weight"], w[p + "bias"], 0, x.shape[0])
    ce = None if e is None else conv3(e, np.abs(w[p + "weight"]), None, 0, x.shape[0])[0].reshape(-1, 32)
    return v.reshape(-1, 32), m.reshape(-1, 32), ce


# ---- the sync points ----------------------------------------------------------------------------------------------------------
# Every function returns [(name, family, passes, worst fraction of its bound, ratio |gpu - ref| / (2^-24 m))].
# run / prev: this run's and the previous stop's, each with .get(name, image) -> [H][W][C] float32, .st (the parsed blob as it
# stands), .B (images the pass's tensors hold).  c: a Ctx.

class Ctx:
    def __init__(self, w, smean, images, k=None, strips=whole, streaming=False):
        self.w, self.smean, self.images, self.k, self.strips, self.streaming = w, np.asarray(smean, np.float64), images, k or LR.K, strips, streaming


def _plain(out, name, fam, got, v, m, c):
    ok, worst, ratio = check(got, v, m, c.k[fam])
    out.append((name, fam, ok, worst, ratio))


def _stat(out, name, entry, run, tap, c):
    rs = raw_stats(np.stack([run.get(tap, b) for b in range(run.B)]))
    out.append((name, "pstat") + check_pstat(entry, rs, c.k["pstat"]))


def stage_norm0(run, prev, c):
    out = []
    _stat(out, "norm0", run.st["norm"][0], run, "grp" if c.streaming else "content", c)
    return out


def stage_filter(f):
    def stage(run, prev, c):
        out, w, st = [], c.w, run.st
        tin, tout = FILTER_IO[f]
        fn = "Filter%d" % (f + 1)
        n0 = st["norm"][0]
        if f == 0:      # cn is the normalised content, which is still there
            for b in c.images:
                _plain(out, "cn[%d]" % b, "point", run.get("cn", b), *normed(run.get("grp" if c.streaming else "content", b), n0), c)
        # both predictions from the taps: F2's averaged tensor is t32 itself, F1's is gone
        p = "Decoder.%s.F2.down_sample.0." % fn
        for b in c.images:
            x = run.get(tin, b)
            _plain(out, "t32[%d]" % b, "gemm", run.get("t32", b), *conv3(x, w[p + "weight"], w[p + "bias"], 0, x.shape[0]), c)
        t = np.stack([run.get("t32", b) for b in range(run.B)]).astype(np.float64).reshape(-1, 32)
        out.append(("%s.F2" % fn, "ppred") + check_pred(st["filt"][fn + ".F2"], w, fn + ".F2", t.mean(axis=0), np.abs(t).mean(axis=0),
                                                        c.smean[2 * f + 1], c.k["ppred"]))
        cv = [pred_conv(run.get(tin, b), w, fn + ".F1") for b in range(run.B)]
        v, m = np.concatenate([a for a, _, _ in cv]), np.concatenate([a for _, a, _ in cv])
        out.append(("%s.F1" % fn, "ppred") + check_pred(st["filt"][fn + ".F1"], w, fn + ".F1", v.mean(axis=0), m.mean(axis=0), c.smean[2 * f],
                                                        c.k["ppred"], slack=c.k["gemm"] * U * m.mean(axis=0)))
        # frame 0's chain on the blob's own filters
        if c.streaming:
            x0, mx = normed(run.get("f0", 0), n0)
            for j in range(f):
                r = np.asarray(run.get("su%d" % (j + 1), 0), np.float64)
                x0, mx = x0 + r, mx + np.abs(x0 + r)       # every pass's own result, as LR.frame_checks carries them
            _plain(out, "cn[0] (frame 0)", "point", run.get("cn", 0), x0, mx, c)
            x = run.get("cn", 0)
        else:
            x = run.get(tin, 0)
        _plain(out, "d32", "f23", run.get("d32", 0), *LR._down(f)([x], w, st, 0, x.shape[0]), c)
        d = run.get("d32", 0)
        utap = "su%d" % (f + 1) if c.streaming else "u"
        _plain(out, utap, "f23", run.get(utap, 0), *fold_up(f, d, w, st, 0, d.shape[0]), c)
        if c.streaming:
            # the group's own walk: IN = the earlier output + frame 0's earlier residual.  Image 0's earlier output is gone (frame
            # 0's chain runs in place in cn[0]): its IN is that chain's result, bit for bit
            for b in c.images if f else ():
                if b:
                    _plain(out, "%s[%d]" % (tin, b), "point", run.get(tin, b), *added(run.get(tout, b), run.get("su%d" % f, 0)), c)
                elif tin != "cn":
                    same = np.array_equal(run.get(tin, 0).view(np.uint32), run.get("cn", 0).view(np.uint32))
                    out.append(("%s[0] == cn[0]" % tin, None, bool(same), 0.0 if same else np.inf, 0.0))
        else:
            u = run.get("u", 0)
            for b in range(run.B):      # frame 0's residual for EVERY image (quirk Q1)
                _plain(out, "%s[%d]" % (tout, b), "point", run.get(tout, b), *added(run.get(tin, b), u), c)
        return out
    return stage


def stage_norm1(run, prev, c):
    out = []
    if c.streaming:
        for b in c.images:
            _plain(out, "nxt[%d]" % b, "point", run.get("nxt", b), *added(run.get("cn", b), run.get("su3", 0)), c)
    _stat(out, "norm1", run.st["norm"][1], run, "nxt", c)
    return out


def stage_block(k, j):
    blk, xs, a, o = BLOCKS[k]
    tin = BLOCK_IN[k]
    n1, n2, na, si = RES[blk]
    pre = "Decoder.%s." % blk

    def stage(run, prev, c):
        out, w, st = [], c.w, run.st
        if j == 0:
            if prev is not None:      # the block's input: normalised + AdaIN in place since the previous stop
                e, s = (st["norm"][1], st["sty"][3]) if k == 0 else (st["norm"][RES[BLOCKS[k - 1][0]][2]], st["sty"][RES[BLOCKS[k - 1][0]][3]])
                for b in c.images:
                    _plain(out, "%s[%d] AdaIN" % (tin, b), "point", run.get(tin, b), *normed(prev.get(tin, b), e, s), c)
            for b in c.images:
                x, got = run.get(tin, b), run.get(a, b)
                for y0, y1 in c.strips(got.shape[0]):
                    _plain(out, "%s[%d] raw" % (a, b), "ups", got[y0:y1], *lrelu(*conv3(x, w[pre + "conv1.weight"], w[pre + "conv1.bias"], y0, y1, ups=True)), c)
            _stat(out, "norm[%d] <- %s" % (n1, a), st["norm"][n1], run, a, c)
        elif j == 1:
            for b in c.images:
                if prev is not None:
                    _plain(out, "%s[%d] norm1" % (a, b), "point", run.get(a, b), *normed(prev.get(a, b), st["norm"][n1]), c)
                x, got = run.get(a, b), run.get(o, b)
                for y0, y1 in c.strips(got.shape[0]):
                    _plain(out, "%s[%d] raw" % (o, b), "f23", got[y0:y1], *lrelu(*conv3(x, w[pre + "conv2.weight"], w[pre + "conv2.bias"], y0, y1)), c)
            _stat(out, "norm[%d] <- %s" % (n2, o), st["norm"][n2], run, o, c)
        else:
            for b in c.images:
                x, got = run.get(tin, b), run.get(xs, b)
                _plain(out, "%s[%d]" % (xs, b), "gemm", got, *conv1(x, w[pre + "conv_shortcut.weight"], 0, x.shape[0]), c)
                if prev is not None:
                    raw = prev.get(o, b)
                    v, m = normed(raw, st["norm"][n2])
                    _plain(out, "%s[%d] norm2 + shortcut" % (o, b), "point", run.get(o, b), *added_up(v, m, got, raw.shape), c)
            _stat(out, "norm[%d] <- %s" % (na, o), st["norm"][na], run, o, c)
        return out
    return stage


def added_up(v, m, xs, shape):
    r = LR._up2(xs, shape[0], shape[1])
    return v + r, m + np.abs(r)


# the taps of the pass stopped at s that the checks of stop s + 1 read (its raw tensors, normalised in place by then)
KEEP = {4: ("nxt",), 5: ("a4",), 6: ("o4",), 7: ("o4",), 8: ("a3",), 9: ("o3",), 10: ("o3",), 11: ("a2",), 12: ("o2",)}
STAGES = [stage_norm0, stage_filter(0), stage_filter(1), stage_filter(2), stage_norm1] + [stage_block(k, j) for k in range(3) for j in range(3)]
assert len(STAGES) == N_STOPS


# ---- several groups (the streaming pass over ragged groups): stops 0 .. 3 from the stored features -----------------------------

def multi_norm0(patches, st, c):
    rs = raw_stats(np.stack(patches))
    return [("norm0 (merged)", "pstat") + check_pstat(st["norm"][0], rs, c.k["pstat"])]


def multi_filter(f, patches, run, c):
    """Filter f's two predictions from the stored features of ALL frames: frame b's input is the float64 pointwise result
    norm[0](patch b) + su[0] + .. + su[f-1]; what the GPU held differs from it by the pointwise passes' own rounding (the point
    family's bound on each pass's result), which enters through |W_conv| and the mean like the convolution's own term.  Then
    frame 0's chain cn[0] -> d32 -> su[f] from its taps."""
    out, w, st = [], c.w, run.st
    fn = "Filter%d" % (f + 1)
    n0 = st["norm"][0]
    su = [np.asarray(run.get("su%d" % (j + 1), 0), np.float64) for j in range(f)]
    for g in (1, 2):
        name = "%s.F%d" % (fn, g)
        vs, ms, es = [], [], []
        for pt in patches:
            x, mx = normed(pt, n0)
            e = c.k["point"] * U * mx + U * np.abs(x)
            for r in su:
                x = x + r
                e = e + c.k["point"] * U * (np.abs(x - r) + np.abs(r)) + U * np.abs(x)
            v, m, ce = pred_conv(x, w, name, e)
            vs.append(v), ms.append(m), es.append(ce)
        v, m, ce = np.concatenate(vs), np.concatenate(ms), np.concatenate(es)
        out.append((name + " (merged)", "ppred") + check_pred(st["filt"][name], w, name, v.mean(axis=0), m.mean(axis=0), c.smean[2 * f + g - 1],
                                                              c.k["ppred"], slack=(c.k["gemm"] * U * m + ce).mean(axis=0)))
    x0, mx = normed(patches[0], n0)
    for r in su:
        x0, mx = x0 + r, mx + np.abs(x0 + r)
    _plain(out, "cn[0] (frame 0)", "point", run.get("cn", 0), x0, mx, c)
    x = run.get("cn", 0)
    _plain(out, "d32", "f23", run.get("d32", 0), *LR._down(f)([x], w, st, 0, x.shape[0]), c)
    d = run.get("d32", 0)
    _plain(out, "su%d" % (f + 1), "f23", run.get("su%d" % (f + 1), 0), *fold_up(f, d, w, st, 0, d.shape[0]), c)
    return out


# ---- the style side (prepare_style) ---------------------------------------------------------------------------------------------

def style_checks(get, st, smean, w, k=None):
    """get(name) -> [H][W][C] of style_c11 .. style_c41 and map; st: the parsed blob; smean [6][32]: the cached style half."""
    k = k or LR.K
    out = []
    for i, name in enumerate(STYLE_TAPS):
        out.append(("sty[%d] <- %s" % (i, name), "pstat") + check_pstat_style(st["sty"][i], raw_stats(get(name)), k["pstat"]))
    same = np.array_equal(get("map").view(np.uint32), get("style_c41").view(np.uint32))
    out.append(("map == style_c41", None, bool(same), 0.0 if same else np.inf, 0.0))
    # pointwise_k's division form, then the predictor convolution and the mean, three kernels in one figure: the bound carries
    # the division's and the convolution's terms through the mean, the ratio is the excess over them
    mean, std = st["sty"][3]
    x = np.asarray(get("map"), np.float64)
    sn, msn = (x - mean) / std, (np.abs(x) + np.abs(mean)) / std
    e = k["point"] * U * msn + U * np.abs(sn)
    for i, name in enumerate(LR.FILTER_NAMES):
        v, m, ce = pred_conv(sn, w, name, e)
        ref, mag, slack = v.mean(axis=0), m.mean(axis=0), (k["gemm"] * U * m + ce).mean(axis=0)
        err = np.abs(np.asarray(smean[i], np.float64) - ref)
        bound = k["ppred"] * U * mag + U * np.abs(ref) + slack
        out.append(("style half of %s" % name, "ppred", bool(np.all(err <= bound)), float((err / np.maximum(bound, 1e-300)).max()),
                    float((np.maximum(err - slack, 0.0) / np.maximum(U * mag, 1e-300)).max())))
    return out

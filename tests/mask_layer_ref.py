"""Float64 references and the error model for the masked multi-style walk (mask_mode_device; csrc/mask_kernels.h:
mask_pyramid_k, mask_norm_k, mask_filter_k), in the manner of tests/layer_ref.py.  Plain module (no pytest): imported by
tests/test_gpu_mask_layers.py, tests/test_gpu_mask_blend.py and tests/test_layer_ref.py.

Every stage is teacher-forced on the GPU's own input tap(s) AND on the GPU's own level-mask tap, so a check sees one kernel's
rounding and nothing upstream.  The level masks themselves (taps 33..36) are compared bit for bit with
mask_ref.level_masks of the mask the caller passed.  What a masked launch leaves behind:
  lm0..lm3  the level masks at stride 1, 2, 4, 8: RRV_MAX_STYLES-channel ring-layout tensors, row y + 1 holding w * S floats
            from its first interior pixel on (mask_kernels.h LevelMask), every other float 0 on a fresh handle
  c11..p3   the encoder, as on the global path
  c41       masked Decoder.norm[0], in place, of ReLU(conv4_1(p3))                      conv + mask_norm_k
  dpart     (split > 1) the raw split-K partial sums of Filter3.down_sample(f2): their float64 sum against the float64
            convolution with bias 0
  d         mask_filter_k's output for Filter3: in-order slice sum + bias, F1(p), LeakyReLU, F2(p), with
            F(p) = sum_s m_s(p) F_s.  Split > 1: against its own input dpart (the kernel alone); split 1 (filtered in place):
            composite with the convolution from f2
  f1, f2    composite: d of Filter1 / Filter2 is overwritten, so it is recomputed in float64 (convolution, mask_filter_k,
            convolution); its error enters through |W_up|
  f3        masked norm[1] + AdaIN, in place, of f2 + upsample_conv(d)                  conv + mask_norm_k
  xs        the raw fused 1 x 1 shortcut
  a         masked norm1, in place, of LeakyReLU(conv1(up(in)))                         conv + mask_norm_k
  o         masked AdaIN of (masked norm2 of LeakyReLU(conv2(a)) + up(xs)), in place    conv + mask_norm_k twice
  pre       slice1

Masked normalisation: q(p) = sum_s m_s(p) q_s in float64 from the float32 mask tap and the float32 blobs,
  v = clamp((x - mean(p)) rstd(p), lo(p), hi(p)) [+ r] [std(p) + smean(p)]
with the magnitude of LR.norm / LR.adain, every blended parameter replaced by sum_s |m_s| |q_s|.  As in frame mode,
  |gpu - ref| <= 2^-24 (K_conv m_conv + K_mnorm m_point + |ref|)
with m_conv the convolution's magnitude carried through the later steps' scales only, and m_point the magnitude of every
mask_norm_k pass's own result carried the same way.  Two families (figures and K in layer_ref.MEASURED / K):
  mnorm  mask_norm_k.  In place, so never visible alone: measured like `point`, the WHOLE error of a normalised tap over
         2^-24 m_point.
  mfilt  mask_filter_k.  Visible alone at d (split > 1): |gpu - ref| <= K_mfilt 2^-24 m + 2^-24 |ref|, m the same arithmetic on
         absolute values: |F2|(p) |F1|(p) (sum |slices| + |bias|); the unobservable e = LeakyReLU(F1 d) enters through
         |F2|(p) m_e.
"""
import numpy as np

import layer_ref as LR

U = LR.U
LM_TAP = (33, 34, 35, 36)           # rrv_debug_copy_tensor_ex: DecPlan::lm[0..3]
MASK_CH = 8                         # RRV_MAX_STYLES: the channels of a level-mask tensor

# the profile rows of one masked launch sequence ("conv": any conv_* row but conv_first / conv_last); no sum_parts anywhere
MASK_SEQ = (["mask_pyramid", "conv_first"] + ["conv"] * 8 + ["mask_norm"] + ["conv", "mask_filter", "conv"] * 3 + ["mask_norm"]
            + ["conv", "mask_norm", "conv", "mask_norm", "mask_norm"] * 3 + ["conv_last"])
MASK_BLOCKS = tuple(b + (l,) for b, l in zip(LR.FRAME_BLOCKS, (2, 1, 0)))      # (block, input, xs, a, o, mask level)
MASK_STAGES = (("lm0", "lm1", "lm2", "lm3") + LR.FRAME_ENC + ("c41", "f1", "f2", "dpart", "d", "f3")
               + tuple(n for _, _, xs, a, o, _ in MASK_BLOCKS for n in (xs, a, o)) + ("pre",))
EIGHTH = ("lm3", "c41", "dpart", "d", "f1", "f2", "f3")        # the stages of the 1/8 level behind the encoder


def mask_families(rows):
    """rows: the profile row names of one masked launch.  Asserts that they are MASK_SEQ exactly (so no sum_parts row: the
    slices are summed by mask_filter_k), without F(4x4,3x3), the upsample-fused family on every conv1; returns {stage: family}."""
    assert len(rows) == len(MASK_SEQ) == 37, rows
    fams = []
    for name, want in zip(rows, MASK_SEQ):
        k = name.split("@")[0]
        if want == "conv":
            assert k.startswith("conv_") and not k.startswith(("conv_first", "conv_last", "conv_f43")), (name, want)
            fams.append(LR.family_of(name, False))
        else:
            assert k == want, (name, want)
            if want in ("conv_first", "conv_last"):
                fams.append("direct")
    keys = LR.FRAME_ENC + ("c41", "d0", "u0", "d1", "u1", "d2", "u2", "a4", "o4", "a3", "o3", "a2", "o2", "pre")
    assert len(fams) == len(keys), (len(fams), len(keys))
    fam = dict(zip(keys, fams))
    assert fam["a4"] == fam["a3"] == fam["a2"] == "ups", fam
    return fam


def decode_level_mask(flat, h, w, S):
    """A level-mask tap (ring layout [h+2][w+2][8]) -> [S][h][w].  Row y + 1 holds w * S floats from its first interior pixel
    on; every float outside those runs must be exactly 0."""
    a = np.asarray(flat, np.float32).reshape(h + 2, (w + 2) * MASK_CH)
    run = a[1:h + 1, MASK_CH:MASK_CH + w * S]
    rest = a.copy()
    rest[1:h + 1, MASK_CH:MASK_CH + w * S] = 0
    assert not np.any(rest), "level mask: %d non-zero floats outside the w * S run of a row" % np.count_nonzero(rest)
    return np.ascontiguousarray(run.reshape(h, w, S).transpose(2, 0, 1))


def mask_states(base, S):
    """S distinct state blobs from the four computed ones: the first four as they are, the rest fixed float32 blends of pairs of
    them (the layer checks are teacher-forced, so a state need not come from a real style)."""
    base = [np.asarray(b, np.float32).reshape(-1) for b in base]
    assert len(base) >= min(S, 4)
    out = list(base[:min(S, 4)])
    for k in range(4, S):
        t = np.float32(0.25 + 0.125 * (k - 4))
        out.append((t * base[(k - 4) % 4] + (np.float32(1) - t) * base[(k - 3) % 4]).astype(np.float32))
    for i in range(S):
        for j in range(i):
            assert not np.array_equal(out[i], out[j]), (i, j)
    return out


def softmax_mask(seed, S, H, W, B=None):
    """m = softmax(N(0, 1)) over S per pixel, float32: no two neighbouring pixels and no two levels carry the same weights."""
    r = np.random.default_rng(seed)
    z = r.standard_normal(((B or 1), S, H, W)).astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    m = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    return m if B else m[0]


def odd_edge_mask(S, H, W, row=27, col=13):
    """style 0 left of column `col` and above row `row`, style 1 elsewhere: a hard edge on no multiple of 2"""
    m = np.zeros((S, H, W), np.float32)
    m[1] = 1
    m[0, :row, :col], m[1, :row, :col] = 1, 0
    return m


# ---- blended parameters ------------------------------------------------------------------------------------------------

def _blend(mk, rows):
    """mk [S][h][w] float64, rows: S arrays of one shape -> (sum_s m_s rows_s, sum_s |m_s| |rows_s|) as [h][w][...]"""
    R = np.stack([np.asarray(r, np.float64) for r in rows])
    return np.tensordot(mk, R, axes=([0], [0])), np.tensordot(np.abs(mk), np.abs(R), axes=([0], [0]))


def _pass(v, m, mc, mp, mk, sts, n, r=None, sty=None):
    """v: value; m: its magnitude (what this pass reads); mc: the convolution's magnitude so far; mp: the sum of the earlier
    passes' own magnitudes so far.  Returns the same four after the pass."""
    (mean, amean), (rstd, arstd), (lo, _), (hi, _) = (_blend(mk, [st["norm"][n][i] for st in sts]) for i in range(4))
    v = np.minimum(hi, np.maximum(lo, (v - mean) * rstd))
    m, mc, mp = (m + amean) * arstd, mc * arstd, mp * arstd
    if r is not None:
        v, m = v + r, m + np.abs(r)
    if sty is not None:
        (sm, asm), (sd, asd) = (_blend(mk, [st["sty"][sty][i] for st in sts]) for i in range(2))
        v, m, mc, mp = v * sd + sm, m * asd + asm, mc * asd, mp * asd
    return v, m, mc, mp + m



def filt(mk, sts, f):
    """(F1, |F1|, F2, |F2|) of KernelFilter f + 1 blended per pixel: [h][w][32][32] each"""
    F1, A1 = _blend(mk, [st["filt"]["Filter%d.F1" % (f + 1)] for st in sts])
    F2, A2 = _blend(mk, [st["filt"]["Filter%d.F2" % (f + 1)] for st in sts])
    return F1, A1, F2, A2


def _mv(F, x):
    return np.einsum("hwij,hwj->hwi", F, x)


def mask_filter(x, mx, mk, sts, f, mconv=None):
    """mask_filter_k behind the slice sum: out = F2(p) LeakyReLU(F1(p) x).  Returns (out, its magnitude, mconv carried through
    |F2| |F1|)."""
    F1, A1, F2, A2 = filt(mk, sts, f)
    e = _mv(F1, x)
    e = np.where(e >= 0, e, 0.2 * e)
    return _mv(F2, e), _mv(A2, _mv(A1, mx)), None if mconv is None else _mv(A2, _mv(A1, mconv))


def slices(part, split):
    """dpart rows [h][w][32 * split] -> (in-order float64 sum, sum of absolute values) [h][w][32]"""
    p = np.asarray(part, np.float64).reshape(part.shape[0], part.shape[1], split, 32)
    v = p[:, :, 0].copy()
    for k in range(1, split):
        v = v + p[:, :, k]
    return v, np.abs(p).sum(axis=2)


def check_level_masks(get, lv, S, levels=(0, 1, 2, 3)):
    """The level-mask taps against mask_ref.level_masks(...) bit for bit: [(stage, None, passes, mismatches, 0)]"""
    out = []
    for l in levels:
        got = get("lm%d" % l)
        same = got.shape == lv[l].shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(lv[l]).view(np.uint32))
        bad = float(np.count_nonzero(got != lv[l])) if got.shape == lv[l].shape else np.inf
        out.append(("lm%d" % l, None, bool(same), 0.0 if same else max(bad, 1.0), 0.0))
    return out


def mask_checks(get, w, sts, fam, split, k=None, names=None):
    """Every stage behind the level masks (or `names`, of MASK_STAGES) of one image of a masked launch.  get(name): the tap
    [H][W][C] ("frame": grey_input of the frame, "pre": the pre-clamp output, "lm<l>": the decoded level mask [S][h][w],
    "dpart": the slices [h][w][32 * split]); sts: the S parsed states in style order; fam: mask_families(); split: the slices
    of the KernelFilter down convolution.  Returns [(stage, family or None, passes, worst fraction of its bound, ratio)]:
    `ratio` is the family's measured figure; family None: a composite of several kernels, no figure."""
    k = LR.K if k is None else k
    res = {}
    order = []

    def want(n):
        return names is None or n in names

    def note(name, f, err, bound, mag):
        ok = bool(np.all(err <= bound))
        worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        ratio = float((err / np.maximum(U * mag, 1e-300)).max()) if (err.size and mag is not None) else 0.0
        if name not in res:
            order.append(name)
            res[name] = (name, f, ok, worst, ratio)
        else:
            _, _, ok0, w0, r0 = res[name]
            res[name] = (name, f, ok and ok0, max(worst, w0), max(ratio, r0))

    def plain(name, got, v, m, f):
        err = np.abs(np.asarray(got, np.float64) - v)
        note(name, f, err, k[f] * U * m + U * np.abs(v), m)

    def forced(name, got, v, mc, mp, f):
        err = np.abs(np.asarray(got, np.float64) - v)
        note(name, "mnorm", err, U * (k[f] * mc + k["mnorm"] * mp + np.abs(v)), mp)

    def lm(l, y0, y1):
        return np.asarray(get("lm%d" % l), np.float64)[:, y0:y1]

    for name in LR.FRAME_ENC:
        if not want(name):
            continue
        _, inputs, op, _ = LR.STAGES[name]
        got, inp = get(name), [get(i) for i in inputs]
        for y0, y1 in LR.strips(got.shape[0]):
            plain(name, got[y0:y1], *op(inp, w, sts[0], y0, y1), fam[name])
    if want("c41"):
        p3, got = get("p3"), get("c41")
        for y0, y1 in LR.strips(got.shape[0]):
            v, m = LR._enc_stage(19, ())([p3], w, None, y0, y1)
            v, _, mc, mp = _pass(v, m, m, 0.0, lm(3, y0, y1), sts, 0)
            forced("c41", got[y0:y1], v, mc, mp, fam["c41"])
    cur = ("c41", "f1", "f2")
    for f in range(2):
        name = "f%d" % (f + 1)
        if not want(name):
            continue
        x, got = get(cur[f]), get(name)
        p = "Decoder.Filter%d." % (f + 1)
        for y0, y1 in LR.strips(got.shape[0]):
            r0, r1 = max(0, y0 - 1), min(x.shape[0], y1 + 1)
            cv, cm = LR.conv3(x, w[p + "down_sample.0.weight"], None, r0, r1)
            b = np.asarray(w[p + "down_sample.0.bias"], np.float64)
            dv, dm, dc = mask_filter(cv + b, cm + np.abs(b), lm(3, r0, r1), sts, f, mconv=cm)
            full = np.zeros((3, x.shape[0]) + dv.shape[1:])
            full[0, r0:r1], full[1, r0:r1], full[2, r0:r1] = dv, dm, dc
            wu = w[p + "upsample.0.weight"]
            v, mu = LR.conv3(full[0], wu, w[p + "upsample.0.bias"], y0, y1)
            _, mf = LR.conv3(full[1], wu, None, y0, y1)
            _, md = LR.conv3(full[2], wu, None, y0, y1)
            r = np.asarray(x[y0:y1], np.float64)
            v, mu = v + r, mu + np.abs(r)
            err = np.abs(got[y0:y1].astype(np.float64) - v)
            note(name, None, err, U * (k[fam["d%d" % f]] * md + k["mfilt"] * mf + k[fam["u%d" % f]] * mu + np.abs(v)), None)
    pd = "Decoder.Filter3."
    if want("dpart") and split > 1:
        x, part = get("f2"), get("dpart")
        for y0, y1 in LR.strips(part.shape[0]):
            sv, _ = slices(part[y0:y1], split)
            plain("dpart", sv, *LR.conv3(x, w[pd + "down_sample.0.weight"], None, y0, y1), fam["d2"])
    if want("d"):
        got = get("d")
        b = np.asarray(w[pd + "down_sample.0.bias"], np.float64)
        for y0, y1 in LR.strips(got.shape[0]):
            if split > 1:
                xv, xm = slices(get("dpart")[y0:y1], split)
                v, m, _ = mask_filter(xv + b, xm + np.abs(b), lm(3, y0, y1), sts, 2)
                plain("d", got[y0:y1], v, m, "mfilt")
            else:       # filtered in place: the convolution's raw output is gone
                cv, cm = LR.conv3(get("f2"), w[pd + "down_sample.0.weight"], None, y0, y1)
                v, m, mc = mask_filter(cv + b, cm + np.abs(b), lm(3, y0, y1), sts, 2, mconv=cm)
                err = np.abs(got[y0:y1].astype(np.float64) - v)
                note("d", None, err, U * (k[fam["d2"]] * mc + k["mfilt"] * m + np.abs(v)), None)
    if want("f3"):
        d, x, got = get("d"), get("f2"), get("f3")
        for y0, y1 in LR.strips(got.shape[0]):
            v, m = LR.conv3(d, w[pd + "upsample.0.weight"], w[pd + "upsample.0.bias"], y0, y1)
            r = np.asarray(x[y0:y1], np.float64)
            v, m = v + r, m + np.abs(r)
            v, _, mc, mp = _pass(v, m, m, 0.0, lm(3, y0, y1), sts, 1, sty=3)
            forced("f3", got[y0:y1], v, mc, mp, fam["u2"])
    for blk, xin, xs, a, o, l in MASK_BLOCKS:
        n1, n2, na, si = LR.RES[blk]
        pre = "Decoder.%s." % blk
        if want(xs):
            x, got = get(xin), get(xs)
            for y0, y1 in LR.strips(got.shape[0]):
                plain(xs, got[y0:y1], *LR.conv1(x, w[pre + "conv_shortcut.weight"], y0, y1), fam[a])
        if want(a):
            x, got = get(xin), get(a)
            for y0, y1 in LR.strips(got.shape[0]):
                v, m = LR.lrelu(*LR.conv3(x, w[pre + "conv1.weight"], w[pre + "conv1.bias"], y0, y1, ups=True))
                v, _, mc, mp = _pass(v, m, m, 0.0, lm(l, y0, y1), sts, n1)
                forced(a, got[y0:y1], v, mc, mp, fam[a])
        if want(o):
            at, xt, got = get(a), get(xs), get(o)
            for y0, y1 in LR.strips(got.shape[0]):
                v, m = LR.lrelu(*LR.conv3(at, w[pre + "conv2.weight"], w[pre + "conv2.bias"], y0, y1))
                xsu = np.repeat(np.asarray(xt, np.float64)[np.arange(y0, y1) // 2], 2, axis=1)[:, :v.shape[1]]
                mk = lm(l, y0, y1)
                v, m, mc, mp = _pass(v, m, m, 0.0, mk, sts, n2, r=xsu)
                v, _, mc, mp = _pass(v, m, mc, mp, mk, sts, na, sty=si)
                forced(o, got[y0:y1], v, mc, mp, fam[o])
    if want("pre"):
        o2, got = get("o2"), get("pre")
        for y0, y1 in LR.strips(got.shape[0]):
            plain("pre", got[y0:y1], *LR._last([o2], w, None, y0, y1), fam["pre"])
    return [res[n] for n in order]

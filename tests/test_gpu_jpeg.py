"""The JPEG output stage on the GPU (include/rerevst_hip.h "JPEG output"), each half against a reference of its own (tests/jpeg_ref.py): the
samples against the delivery stage's I4xx frame, the coefficient blocks against the float64 transform, the streams bit for bit against the
reference's coder on the GPU's own and on built coefficient blocks; capacity, stale scratch and the failure paths.  Tiny frames."""
import ctypes as C
import importlib
import io

import numpy as np
import pytest

import jpeg_ref as R
from conftest import load_golden, fixed_kernels

pytestmark = pytest.mark.gpu

RRV_OK, RRV_E_ARG, RRV_E_NOMEM = 0, -1, -5
L = importlib.import_module("rerevst-code_amd._lib")
F = importlib.import_module("rerevst-code_amd.framework")
CHROMAS = ("420", "422", "444")                      # the jpeg_blocks_k instantiation a chroma format launches: <2, 2>, <2, 1>, <1, 1>
SIZES = ((17, 23), (48, 80), (8, 8))                 # odd and below one MCU row of the workgroup; several workgroups; one block
PIL_SUB = {"444": 0, "422": 1, "420": 2}
DECODE_MARGIN = 1.05                                 # tests/test_jpeg_host.py calibrates it on the reference alone (profiles/jpeg.txt)


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _np(s, t):
    _torch().cuda.synchronize()
    s.sync()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def hip(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    s.set_state(load_golden("global_a")["state"])
    yield s
    s.close()


def _frames(B, H, W, seed=3):
    """B frames: white noise and smooth-plus-noise in turn, the noise frame first"""
    return np.concatenate([R.bgr_frames(seed + b, 1, H, W, "noise" if b % 2 == 0 else "smooth") for b in range(B)])


def _both_kinds(B, H, W):
    return [np.concatenate([R.bgr_frames(11 + b, 1, H, W, kind) for b in range(B)]) for kind in ("noise", "smooth")]


def _bound(H, W, chroma="420", restart=None):
    return F.jpeg_plan(H, W, chroma, restart)["bound"]


def _streams(s, data, sizes):
    return F.jpeg_frames(_np(s, data), _np(s, sizes))


# ---- samples
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("size", SIZES[:2])
def test_samples_are_the_delivered_yuv_frame(hip, size, chroma):
    """at quality 100 every quantiser is 1: a block's DC is rint(sum(sample - 128) / 8), exact in float32 up to the tie at a half, and the float64
    inverse of the blocks returns the samples to within the coefficients' rounding: an orthonormal transform keeps the L2 norm, so the rms
    error of a block is at most 0.5.  The samples are deliver_tensor's I4xx bytes of the same frames with BT.601 full range set, each plane
    continued by its last sample to whole MCUs."""
    H, W = size
    x = _frames(2, H, W)
    hs, vs = R.FACTORS[chroma]
    p = R.plan(H, W, chroma)
    hip.set_yuv_matrix("bt601", True)
    try:
        yuv = _np(hip, hip.deliver_tensor(_dev(x), (H, W), out_layout="i" + chroma))
    finally:
        hip.set_yuv_matrix(None)
    import chroma_ref
    planes = chroma_ref.planes(yuv.reshape(2, -1), H, W, "i" + chroma)
    want = []
    for pl, ph, pw in zip(planes, (p["mcu_rows"] * 8 * vs, p["mcu_rows"] * 8, p["mcu_rows"] * 8), (p["mcu_cols"] * 8 * hs, p["mcu_cols"] * 8, p["mcu_cols"] * 8)):
        want.append(np.pad(pl, ((0, 0), (0, ph - pl.shape[1]), (0, pw - pl.shape[2])), mode="edge").astype(np.float64))
    coef = _np(hip, hip.jpeg_blocks_tensor(_dev(x), jpeg_quality=100, jpeg_chroma=chroma))
    got = R.dequantised_planes(coef, H, W, chroma, 100)
    for name, g, w in zip("Y Cb Cr".split(), got, want):
        assert g.shape == w.shape
        e = (g - w).reshape(2, w.shape[1] // 8, 8, w.shape[2] // 8, 8)
        rms = np.sqrt((e ** 2).mean(axis=(2, 4)))
        assert rms.max() <= 0.5 + 1e-3, (name, float(rms.max()))
    # the DCs: the blocks of the reference layout of the delivered planes
    blocks = np.empty((2, p["mcu_rows"], p["mcu_cols"], hs * vs + 2))
    sums = [(w - 128.0).reshape(2, w.shape[1] // 8, 8, w.shape[2] // 8, 8).sum(axis=(2, 4)) / 8.0 for w in want]
    blocks[..., :hs * vs] = sums[0].reshape(2, p["mcu_rows"], vs, p["mcu_cols"], hs).transpose(0, 1, 3, 2, 4).reshape(2, p["mcu_rows"], p["mcu_cols"], hs * vs)
    blocks[..., hs * vs], blocks[..., hs * vs + 1] = sums[1], sums[2]
    dc_exact = blocks.reshape(2, -1)
    dc = coef[:, :, 0].astype(np.float64)
    tie = np.abs(dc_exact - np.floor(dc_exact) - 0.5) < 1e-9
    assert np.array_equal(dc[~tie], np.rint(dc_exact[~tie]))
    assert np.all(np.abs(dc[tie] - dc_exact[tie]) == 0.5)


# ---- coefficients
def _check_coefficients(x, chroma, quality, got):
    """the rule of the issue: equal to rint of the exact quotient, except inside the tie zone of a half-integer, where +-1 is allowed; the zone's
    half-width is 4 x the largest |float32 numpy separable DCT - float64| on the same blocks, divided by the quantiser; at most 2 % may lie in it"""
    s = R.sample_blocks(x, chroma)
    f32_err = float(np.abs(R.dct(s, np.float32).astype(np.float64) - R.dct(s)).max())
    assert f32_err < 2e-4, f32_err
    qt = R.block_quantisers(chroma, quality, s.shape[1]).reshape(-1, 64)[:, R.ZIGZAG][None]
    quo = R.quotients(x, chroma, quality)
    zone = np.abs(quo - np.floor(quo) - 0.5) <= 4.0 * f32_err / qt
    share = float(zone.mean())
    print("%s q%d %s: float32 error %.2e, %.3f %% of the coefficients in the tie zone" % (chroma, quality, x.shape, f32_err, 100 * share))
    assert share <= 0.02
    want = np.rint(quo)
    assert got.shape == want.shape and got.dtype == np.int16
    assert np.array_equal(got[~zone], want[~zone]), int((got[~zone] != want[~zone]).sum())
    g, q = got[zone].astype(np.float64), quo[zone]
    assert np.all((g == np.floor(q)) | (g == np.ceil(q)))


@pytest.mark.parametrize("quality", (50, 90, 100))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("size", SIZES)
def test_blocks_against_the_float64_transform(hip, size, B, chroma, quality):
    H, W = size
    for x in _both_kinds(B, H, W):
        got = _np(hip, hip.jpeg_blocks_tensor(_dev(x), jpeg_quality=quality, jpeg_chroma=chroma))
        assert got.shape == (B, R.plan(H, W, chroma)["blocks"], 64)
        _check_coefficients(x, chroma, quality, got)


# ---- the entropy half
def _assert_streams(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        if g != w:
            first = next((i for i, (u, v) in enumerate(zip(g, w)) if u != v), min(len(g), len(w)))
            raise AssertionError("%s frame %d: %d bytes against the reference's %d, first difference at byte %d" % (what, b, len(g), len(w), first))


@pytest.mark.parametrize("quality", (50, 90, 100))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("size", SIZES)
def test_streams_of_the_gpus_own_blocks(hip, size, B, chroma, quality):
    """the second half, bit for bit against the reference's coder on the first half's output; and both halves in one call equal the two calls"""
    H, W = size
    x = _dev(_frames(B, H, W))
    kw = dict(jpeg_quality=quality, jpeg_chroma=chroma)
    coef = hip.jpeg_blocks_tensor(x, **kw)
    kw["jpeg_cap"] = _bound(H, W, chroma)
    got = _streams(hip, *hip.jpeg_entropy_tensor(coef, (H, W), **kw))
    c = _np(hip, coef)
    _assert_streams(got, [R.stream(c[b], H, W, chroma, quality) for b in range(B)], "entropy half")
    _assert_streams(_streams(hip, *hip.encode_jpeg_tensor(x, **kw)), got, "both halves")


def _built_blocks(kind, mcus, bpm, chroma):
    """coefficient blocks [mcus][bpm][64] that drive the coder into its corners"""
    c = np.zeros((mcus, bpm, 64), np.int16)
    if kind == "zero":
        pass
    elif kind == "dc_jumps":          # difference category 11, both signs
        flat = c.reshape(-1, 64)
        flat[::2, 0], flat[1::2, 0] = -1024, 1016
    elif kind == "ac_extremes":       # the longest codes and dense 0xFF stuffing
        c[..., 1:] = 1023
        c[:, ::2, 1::2] = -1023
    elif kind == "only_63":           # three ZRLs, no EOB
        c[..., 63] = 5
        c[1::2, :, 63] = -1
    elif kind == "runs":              # zero runs of exactly 15, 16 and 32
        for i, run in enumerate((15, 16, 32)):
            c[i::3, :, 1 + run] = 3 + i
            c[i::3, :, 0] = 7 * i
    elif kind == "ends_at_62":        # a non-zero at 62, then EOB
        c[..., 62] = -2
        c[..., 5] = 100
    elif kind == "ff_tail":           # interval 0's padded last byte is 0xFF: searched on the reference
        for dc in range(64):
            for k in range(1, 11):
                c[:] = 0
                c[0, 0, 0] = dc
                c[:, -1, 63] = (1 << k) - 1
                pending, tail = R.interval_tail(c[:1], chroma)
                if pending and tail == b"\xff\x00":
                    return c
        raise AssertionError("no block with an all-ones tail found")
    return c


BUILT = ("zero", "dc_jumps", "ac_extremes", "only_63", "runs", "ends_at_62", "ff_tail")


@pytest.mark.parametrize("restart", (1, 4, "row"))
@pytest.mark.parametrize("kind", BUILT)
@pytest.mark.parametrize("chroma", ("420", "444"))
def test_streams_of_built_blocks(hip, chroma, kind, restart):
    """15 MCUs (5 x 3), so at restart 1 the RST counter wraps; bit for bit against the reference's coder"""
    H, W = (48, 80) if chroma == "420" else (24, 40)
    p = R.plan(H, W, chroma)
    assert p["mcu_cols"] * p["mcu_rows"] == 15
    bpm = p["blocks"] // 15
    r = p["mcu_cols"] if restart == "row" else restart
    c = _built_blocks(kind, 15, bpm, chroma)
    coef = np.stack([c.reshape(-1, 64), c.reshape(-1, 64)[::-1]])      # a second frame, the blocks in reverse
    bound = F.jpeg_plan(H, W, chroma, r)["bound"]
    got = _streams(hip, *hip.jpeg_entropy_tensor(_dev(coef), (H, W), jpeg_quality=75, jpeg_chroma=chroma, jpeg_restart=r, jpeg_cap=bound))
    want = [R.stream(coef[b], H, W, chroma, 75, r) for b in range(2)]
    _assert_streams(got, want, kind)
    assert max(len(w) for w in want) <= bound
    if kind == "ff_tail" and r == 1:
        assert b"\xff\x00\xff\xd0" in want[0]


# ---- the streams decode
def _decode_error(stream, x):
    from PIL import Image
    im = Image.open(io.BytesIO(stream))
    im.load()
    assert im.mode == "RGB" and im.size == (x.shape[1], x.shape[0])
    return float(np.abs(np.asarray(im).astype(np.float64)[..., ::-1] - np.clip(x, 0, 255)).mean())


@pytest.mark.parametrize("chroma", CHROMAS)
def test_pillow_decodes_the_streams(hip, chroma):
    from PIL import Image
    x = R.bgr_frames(5, 3, 48, 80, "smooth")
    streams = _streams(hip, *hip.encode_jpeg_tensor(_dev(x), jpeg_quality=90, jpeg_chroma=chroma, jpeg_restart=4))
    for b, s in enumerate(streams):
        buf = io.BytesIO()
        Image.fromarray(np.clip(np.rint(x[b][..., ::-1]), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90, subsampling=PIL_SUB[chroma])
        ours, pillows = _decode_error(s, x[b]), _decode_error(buf.getvalue(), x[b])
        print("%s frame %d: mean absolute decode error %.4f, Pillow's own encode %.4f" % (chroma, b, ours, pillows))
        assert ours <= DECODE_MARGIN * pillows


def test_a_frames_bytes_do_not_depend_on_the_batch(hip):
    x = _frames(5, 17, 23)
    cap = _bound(17, 23)
    all5 = _streams(hip, *hip.encode_jpeg_tensor(_dev(x), jpeg_cap=cap))
    for b in (0, 4):
        assert _streams(hip, *hip.encode_jpeg_tensor(_dev(x[b:b + 1]), jpeg_cap=cap))[0] == all5[b]
    assert _streams(hip, *hip.encode_jpeg_tensor(_dev(x[::-1].copy()), jpeg_cap=cap))[::-1] == all5


# ---- capacity
def test_a_cap_one_byte_short(hip):
    """the frame that does not fit reports -needed, nothing is written beyond a frame's size or its slot, and the neighbours are what they were"""
    H, W, B = 17, 23, 3
    x = _dev(_frames(B, H, W))
    roomy = _streams(hip, *hip.encode_jpeg_tensor(x, jpeg_cap=_bound(H, W)))
    need = [len(s) for s in roomy]
    big = max(range(B), key=lambda b: need[b])
    assert sum(n == need[big] for n in need) == 1
    cap = need[big] - 1
    torch = _torch()
    guard = 64
    buf = torch.full((B * cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
    j = L.Jpeg(90, 420, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = hip._lib.rrv_jpeg_encode_device(hip._h, C.c_void_p(x.data_ptr()), B, H, W, C.byref(j), C.c_void_p(buf.data_ptr()), cap, C.c_void_p(sizes.data_ptr()), stream)
    assert rc == RRV_OK
    got, sz = _np(hip, buf), _np(hip, sizes)
    assert sz.tolist() == [(-n if b == big else n) for b, n in enumerate(need)]
    for b in range(B):
        slot = got[b * cap:(b + 1) * cap]
        if b != big:
            assert slot[:need[b]].tobytes() == roomy[b]
            assert np.all(slot[need[b]:] == 0xA5)
    assert np.all(got[B * cap:] == 0xA5)
    with pytest.raises(ValueError, match="jpeg_cap"):
        F.jpeg_frames(got[:B * cap].reshape(B, cap), sz)


# ---- stale scratch, failure paths
def test_stale_scratch_does_not_show(hip, pkg, weights):
    big, small = _dev(_frames(3, 48, 80)), _dev(_frames(2, 17, 23, seed=9))
    kw = dict(jpeg_chroma="444", jpeg_restart=1)
    hip.encode_jpeg_tensor(big, jpeg_quality=100, jpeg_cap=_bound(48, 80, "444", 1), **kw)
    kw["jpeg_cap"] = _bound(17, 23, "444", 1)
    got = _streams(hip, *hip.encode_jpeg_tensor(small, **kw))
    fresh = pkg.Stylization(weights, cuda=True)
    try:
        want = _streams(fresh, *fresh.encode_jpeg_tensor(small, **kw))
    finally:
        fresh.close()
    assert got == want


def test_stale_slot_scratch_does_not_show(pkg, weights):
    """the same through the transfer entry, whose coefficient blocks and interval index live in the workspace slot: a 48 x 80 batch, then a
    24 x 40 one on the same slot (one slot, so that both calls use it), against a fresh handle"""
    big, small = _dev(_u8_frames(3, 48, 80)), _dev(_u8_frames(2, 24, 40, seed=9))
    kw = dict(layout="nhwc", out_layout="jpeg", jpeg_chroma="444", jpeg_restart=1)
    state = load_golden("global_a")["state"]
    got = want = None
    with fixed_kernels():
        for stale in (True, False):
            s = pkg.Stylization(weights, cuda=True)
            try:
                s.set_state(state)
                s._chk(s._lib.rrv_set_pipeline(s._h, 1))
                if stale:
                    s.transfer_tensor(big, jpeg_quality=100, jpeg_cap=_bound(48, 80, "444", 1), **kw)
                res = _streams(s, *s.transfer_tensor(small, jpeg_cap=_bound(24, 40, "444", 1), **kw))
            finally:
                s.close()
            got, want = (res, want) if stale else (got, res)
    assert got == want and len(got) == 2


def test_out_of_memory_leaves_the_handle_usable(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    try:
        x = _dev(_frames(2, 17, 23))
        for nth in (1, 2):      # the coefficient blocks, the interval index
            s.debug_fail_alloc(nth)
            with pytest.raises(pkg.RRVError) as e:
                s.encode_jpeg_tensor(x)
            assert e.value.code == RRV_E_NOMEM
            s.debug_fail_alloc(0)
        got = _streams(s, *s.encode_jpeg_tensor(x, jpeg_cap=_bound(17, 23)))
        c = _np(s, s.jpeg_blocks_tensor(x))
        assert got == [R.stream(c[b], 17, 23, "420", 90) for b in range(2)]
    finally:
        s.close()


def test_debug_mode_runs_the_stage(pkg, weights):
    """RRV_DEBUG=2 verifies after every launch; the stage's buffers are plain allocations outside the guard-band table"""
    s = pkg.Stylization(weights, cuda=True)
    try:
        x = _dev(_frames(2, 17, 23))
        want = _streams(s, *s.encode_jpeg_tensor(x, jpeg_cap=_bound(17, 23)))
        s.set_debug(2)
        assert _streams(s, *s.encode_jpeg_tensor(x, jpeg_cap=_bound(17, 23))) == want
    finally:
        s.close()


def test_the_entries_refuse_in_words(hip):
    torch = _torch()
    x = _dev(_frames(1, 17, 23))
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(1, dtype=torch.int32, device="cuda")
    coef = torch.zeros(6 * 64 * 4 + 8, dtype=torch.int16, device="cuda")

    def call(j, B=1, H=17, W=23, cap=4096, o=out):
        rc = hip._lib.rrv_jpeg_encode_device(hip._h, C.c_void_p(x.data_ptr()), B, H, W, C.byref(j) if j else None, C.c_void_p(o.data_ptr()) if o is not None else None,
                                             cap, C.c_void_p(sizes.data_ptr()), None)
        return rc, (hip._lib.rrv_last_error(hip._h) or b"").decode()

    for j, kw, word in ((L.Jpeg(0, 420, 0), {}, "quality"), (L.Jpeg(101, 420, 0), {}, "quality"), (L.Jpeg(90, 411, 0), {}, "chroma"),
                        (L.Jpeg(90, 420, 65536), {}, "restart"), (L.Jpeg(90, 420, -1), {}, "restart"), (L.Jpeg(90, 420, 0), {"B": 65}, "batch"),
                        (L.Jpeg(90, 420, 0), {"B": 0}, "batch"), (L.Jpeg(90, 420, 0), {"H": 0}, "H, W"), (L.Jpeg(90, 420, 0), {"W": 65536}, "H, W"),
                        (L.Jpeg(90, 420, 0), {"cap": 630}, "cap"), (L.Jpeg(90, 420, 0), {"o": None}, "null"), (None, {}, "null")):
        rc, msg = call(j, **kw)
        assert rc == RRV_E_ARG and word in msg, (kw, rc, msg)
    rc = hip._lib.rrv_jpeg_blocks_device(hip._h, C.c_void_p(x.data_ptr()), 1, 17, 23, C.byref(L.Jpeg(90, 420, 0)), C.c_void_p(coef.data_ptr() + 2), None)
    assert rc == RRV_E_ARG and "aligned" in hip._lib.rrv_last_error(hip._h).decode()
    # the handle is as usable as before
    c = _np(hip, hip.jpeg_blocks_tensor(x))
    assert _streams(hip, *hip.encode_jpeg_tensor(x, jpeg_cap=_bound(17, 23))) == [R.stream(c[0], 17, 23, "420", 90)]


# ---- end to end
@pytest.fixture(scope="module")
def frame_model(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, use_Global=False)
    s.prepare_style(pkg.synth_style(64, 64, kind="smooth", seed=7))
    yield s
    s.close()


def _u8_frames(B, H, W, seed=21):
    return np.clip(np.rint(np.concatenate([R.bgr_frames(seed + b, 1, H, W, "smooth") for b in range(B)])), 0, 255).astype(np.uint8)


E2E = {"plain": dict(), "staged": dict(work_size=(32, 48), out_size="source", guide="source", strength=0.6)}


@pytest.mark.parametrize("how", sorted(E2E))
@pytest.mark.parametrize("model,B", (("global", 3), ("frame", 3), ("frame", 17)))
def test_transfer_with_jpeg_output(hip, frame_model, model, B, how):
    """transfer_batch(out_format="jpeg") == rrv_transfer_jpeg (it is that call) == rrv_transfer_jpeg_view_device (transfer_tensor) == the float32
    call followed by rrv_jpeg_encode_device, bit for bit in a fixed kernel mode; Pillow decodes every frame as well as its own encode of the
    float32 result; a frame's bytes do not depend on B or on its position"""
    from PIL import Image
    s = hip if model == "global" else frame_model
    kw = E2E[how]
    x = _u8_frames(B, 40, 56)
    jk = dict(jpeg_quality=85, jpeg_chroma="422", jpeg_restart=3)
    with fixed_kernels(s):
        host = s.transfer_batch(x, out_format="jpeg", **jk, **kw)
        xt = _dev(x)
        view = _streams(s, *s.transfer_tensor(xt, layout="nhwc", out_layout="jpeg", **jk, **kw))
        y = s.transfer_tensor(xt, layout="nhwc", out_dtype=_torch().float32, **kw)
        chain = _streams(s, *s.encode_jpeg_tensor(y, **jk))
        alone = s.transfer_batch(x[B - 1:], out_format="jpeg", **jk, **({k: v for k, v in kw.items()}))
    assert isinstance(host, list) and all(isinstance(b, bytes) for b in host)
    _assert_streams(view, chain, "view entry against the chain")
    _assert_streams(host, chain, "host twin against the chain")
    assert alone[0] == host[B - 1]
    yn = _np(s, y)
    for b in range(B):
        buf = io.BytesIO()
        Image.fromarray(np.clip(np.rint(yn[b][..., ::-1]), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=85, subsampling=PIL_SUB["422"])
        assert _decode_error(host[b], yn[b]) <= DECODE_MARGIN * _decode_error(buf.getvalue(), yn[b])


def test_transfer_jpeg_overflow_names_the_cap(hip):
    x = _u8_frames(2, 40, 56)
    with pytest.raises(ValueError, match="jpeg_cap"):
        hip.transfer_batch(x, out_format="jpeg", jpeg_cap=700)
    assert len(hip.transfer_batch(x, out_format="jpeg")) == 2


def test_driver_gpu_jpeg_writes_the_gpus_bytes(pkg, weights, tmp_path):
    """--gpu-jpeg --video x.avi --no-frames on five 48 x 80 frames: the AVI's chunks decode and are transfer_frames(out_format="jpeg") of the frames"""
    import struct
    from PIL import Image
    D = importlib.import_module("rerevst-code_amd.driver")
    frames = _u8_frames(5, 48, 80, seed=40)
    for i, f in enumerate(frames):
        Image.fromarray(f[..., ::-1].copy()).save(str(tmp_path / ("f%03d.png" % i)))
    style = tmp_path / "style.png"
    Image.fromarray(pkg.synth_style(64, 64, kind="smooth", seed=7)[..., ::-1].copy()).save(str(style))
    models = []

    def factory(args, device):
        models.append(pkg.Stylization(weights, cuda=True, device=device))
        models[0].close_for_real, models[0].close = models[0].close, lambda: None
        return models[0]

    avi = tmp_path / "x.avi"
    with fixed_kernels():
        rc = D.main(["--style", str(style), "--frames", str(tmp_path / "f*.png"), "--checkpoint", "synthetic", "--out", str(tmp_path / "out"),
                     "--video", str(avi), "--no-frames", "--gpu-jpeg", "--jpeg-quality", "90"], model_factory=factory)
        assert rc == 0
        want = models[0].transfer_frames(frames, out_format="jpeg", jpeg_quality=90)
    models[0].close_for_real()
    assert not (tmp_path / "out").exists()
    data = avi.read_bytes()
    at = data.index(b"movi") + 4
    chunks = []
    while data[at:at + 4] == b"00dc":
        n = struct.unpack("<I", data[at + 4:at + 8])[0]
        chunks.append(data[at + 8:at + 8 + n])
        at += 8 + n + (n & 1)
    assert chunks == want
    for c in chunks:
        im = Image.open(io.BytesIO(c))
        im.load()
        assert im.size == (80, 48)


def test_out_of_memory_in_the_slot_reservation(pkg, weights):
    """a plain JPEG transfer reserves the slot's working frame, coefficient blocks and interval index before its first launch (reserve_stages):
    each allocation failing is RRV_E_NOMEM, and the next call works"""
    s = pkg.Stylization(weights, cuda=True)
    try:
        s.set_state(load_golden("global_a")["state"])
        x = _dev(_u8_frames(2, 40, 56))
        with fixed_kernels(s):
            for nth in (1, 2, 3):
                s.debug_fail_alloc(nth)
                with pytest.raises(pkg.RRVError) as e:
                    s.transfer_tensor(x, layout="nhwc", out_layout="jpeg")
                assert e.value.code == RRV_E_NOMEM and "rrv_debug_fail_alloc" in str(e.value)
                s.debug_fail_alloc(0)
            got = _streams(s, *s.transfer_tensor(x, layout="nhwc", out_layout="jpeg"))
            want = _streams(s, *s.encode_jpeg_tensor(s.transfer_tensor(x, layout="nhwc", out_dtype=_torch().float32)))
        assert got == want
    finally:
        s.close()


def test_host_twin_over_several_sub_batches(hip):
    """130 small frames: more than one sub-batch of the host twin, on alternating slots and staging sets; every frame's bytes are those of the
    view entry, which takes 64 frames per call"""
    x = np.concatenate([_u8_frames(13, 24, 40, seed=60 + i) for i in range(10)])
    with fixed_kernels(hip):
        host = hip.transfer_batch(x, out_format="jpeg", jpeg_chroma="444", strength=np.linspace(0.2, 1.0, 130).tolist())
        view = _streams(hip, *hip.transfer_tensor(_dev(x), layout="nhwc", out_layout="jpeg", jpeg_chroma="444", strength=np.linspace(0.2, 1.0, 130).tolist()))
    _assert_streams(host, view, "host twin against the view entry")
    assert len(set(host)) > 100

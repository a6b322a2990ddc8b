"""The JPEG input stage on the GPU (include/rerevst_hip.h "JPEG input"), each half against a reference of its own (tests/jpeg_dec_ref.py): the
coefficient blocks bit for bit on the project's own streams, on built blocks that reach the ends of the code and on Pillow's streams; the planes
against the rounding of the reference's float64 values; corrupt frames as results, not faults; the entries' refusals and failure paths.  Tiny
frames."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import jpeg_dec_ref as D
import jpeg_ref as R

pytestmark = pytest.mark.gpu

RRV_OK, RRV_E_ARG, RRV_E_NOMEM = 0, -1, -5
L = importlib.import_module("rerevst-code_amd._lib")
F = importlib.import_module("rerevst-code_amd.framework")
# one block, below one 4:2:0 MCU; odd with ragged MCUs; several workgroups and MCU rows; more than 64 intervals per frame at restart 1 (the
# marker numbering crosses a wave: 5 x 17 = 85 MCUs at 4:4:4, 3 x 9 = 27 at 4:2:0, where jpeg_planes_k<2, 2> takes six workgroups)
SIZES = ((8, 8), (17, 23), (48, 80), (33, 130))
CHROMAS = ("420", "422", "444")
FORMATS = CHROMAS + ("grey",)
PILLOW = ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1})      # no markers at all: the first two
TIE_CAP = 0.02


def _torch():
    import torch
    return torch


def _np(s, t):
    _torch().cuda.synchronize()
    s.sync()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def hip(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    yield s
    s.close()


def _frames(B, H, W, kind, seed=3):
    return np.concatenate([R.bgr_frames(seed + b, 1, H, W, kind) for b in range(B)])


def _coef(s, streams):
    coef, status = s.jpeg_coefficients_tensor(streams, return_status=True)
    return _np(s, coef), _np(s, status)


def _planes(s, streams):
    planes, layout, status = s.decode_jpeg_tensor(streams, return_status=True)
    return _np(s, planes), layout, _np(s, status)


# ---- entropy half, the project's own streams
@pytest.mark.parametrize("restart", (1, 4, None))
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("size", SIZES)
def test_coefficients_of_own_streams(hip, size, chroma, restart):
    H, W = size
    for kind in ("noise", "smooth"):
        want = R.coefficients(_frames(3, H, W, kind), chroma, 90)
        streams = [R.stream(want[b], H, W, chroma, 90, restart) for b in range(3)]
        got, status = _coef(hip, streams)
        assert not status.any(), status
        assert got.dtype == np.int16 and np.array_equal(got, want)
        one, status = _coef(hip, streams[1:2])      # B = 1, and another position in the batch
        assert not status.any() and np.array_equal(one[0], want[1])
    if (H, W) == (33, 130) and chroma == "444" and restart == 1:
        assert F.jpeg_info(streams[0])["intervals"] == 85


@pytest.mark.parametrize("restart", (1, 4, "row"))
@pytest.mark.parametrize("chroma", ("420", "444"))
def test_coefficients_of_built_blocks(hip, chroma, restart):
    """15 MCUs (5 x 3), so at restart 1 the RST counter wraps: DC differences of category 11 in both signs, AC +-1023, one, two and three ZRL,
    coefficient 63 set (no EOB), all-zero blocks, and intervals whose last byte is a stuffed FF"""
    H, W = (48, 80) if chroma == "420" else (24, 40)
    p = R.plan(H, W, chroma)
    assert p["mcu_cols"] * p["mcu_rows"] == 15
    r = p["mcu_cols"] if restart == "row" else restart
    built = D.built_blocks(chroma, 15)
    coef = [built, built[::-1].copy(), D.ff_tail_blocks(chroma, 15)]
    if r >= 3:
        y = built[::p["blocks"] // 15, 0].astype(int)
        assert 2047 in np.diff(y[:r]) and -2047 in np.diff(y[:r])
    streams = [R.stream(c, H, W, chroma, 75, r) for c in coef]
    if r == 1:
        assert b"\xff\x00\xff\xd0" in streams[2]
    got, status = _coef(hip, streams)
    assert not status.any(), status
    for b in range(3):
        assert np.array_equal(got[b], coef[b]), b


def test_the_loop_closes_on_the_gpus_own_bytes(hip):
    """rrv_jpeg_entropy_device, then rrv_jpeg_scan_device on what it wrote"""
    torch = _torch()
    for chroma, restart in (("420", None), ("422", 1), ("444", 3)):
        x = torch.from_numpy(_frames(3, 17, 23, "noise")).cuda()
        coef = hip.jpeg_blocks_tensor(x, jpeg_quality=90, jpeg_chroma=chroma, jpeg_restart=restart)
        cap = F.jpeg_plan(17, 23, chroma, restart)["bound"]
        streams = F.jpeg_frames(*(_np(hip, t) for t in hip.jpeg_entropy_tensor(coef, (17, 23), jpeg_quality=90, jpeg_chroma=chroma, jpeg_restart=restart, jpeg_cap=cap)))
        got, status = _coef(hip, streams)
        assert not status.any() and np.array_equal(got, _np(hip, coef))


# ---- foreign streams: both halves
def _pillow_streams(H, W, fmt, kind):
    """fifteen streams of one size and chroma format: qualities 50 / 90 / 100 x default tables, optimised tables (neither has restart markers),
    restart blocks 1, restart rows 1, and the default tables with the DHT segments cut out; every stream from another frame"""
    out = []
    for qi, q in enumerate((50, 90, 100)):
        for vi, kw in enumerate(PILLOW + ("bare",)):
            frame = R.bgr_frames(100 + 5 * qi + vi, 1, H, W, kind)[0]
            s = D.pillow_stream(frame, q, fmt if fmt != "grey" else "444", grey=fmt == "grey", **({} if kw == "bare" else kw))
            out.append(D.without_dht(s) if kw == "bare" else s)
    return out


@pytest.fixture(scope="module")
def pillow_cases():
    """the streams of a (size, format, kind) and the reference's decode of them, computed once for the two tests that use them"""
    cache = {}

    def get(size, fmt, kind):
        key = (size, fmt, kind)
        if key not in cache:
            streams = _pillow_streams(size[0], size[1], fmt, kind)
            cache[key] = (streams, [D.coefficients(s) for s in streams])
        return cache[key]
    return get


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES)
def test_coefficients_of_pillow_streams(hip, pillow_cases, size, fmt):
    for kind in ("noise", "smooth"):
        streams, ref = pillow_cases(size, fmt, kind)
        got, status = _coef(hip, streams)
        assert not status.any(), status
        for b, (info, want) in enumerate(ref):
            assert np.array_equal(got[b], want), (kind, b)
        three, status = _coef(hip, streams[4:7])      # B = 3 at other positions; tables and intervals differ frame by frame
        assert not status.any() and np.array_equal(three, got[4:7])
    assert F.jpeg_info(streams[0])["chroma"] == (400 if fmt == "grey" else int(fmt))


def _check_planes(info, coef, frame, what):
    """the rule of the issue: equal to rint of the exact value outside the tie zone; inside it either neighbour.  The zone's half-width is 4 x the
    largest |float32 numpy separable inverse DCT - float64| on the same blocks.  Exact ties (within 1e-9 of a half-integer) are common where a
    block has only a DC coefficient: either neighbour is right there, and they are set aside before the share of near-ties is capped."""
    err = D.f32_error(info, coef)
    y, cb, cr = D.exact_planes(info, coef)
    gy, gcb, gcr = D.split_planes(frame, info)
    if cb is None:
        assert np.all(gcb == 128) and np.all(gcr == 128), what
    near = total = 0
    for exact, got in ((y, gy), (cb, gcb), (cr, gcr)) if cb is not None else ((y, gy),):
        v = np.clip(exact, 0.0, 255.0)
        g = got.astype(np.float64)
        d = np.abs(v - np.floor(v) - 0.5)
        tie = d < 1e-9
        zone = (d <= 4.0 * err) & ~tie
        sure = ~tie & ~zone
        assert np.array_equal(g[sure], np.rint(v[sure])), (what, int((g[sure] != np.rint(v[sure])).sum()))
        loose = tie | zone
        assert np.all((g[loose] == np.floor(v[loose])) | (g[loose] == np.ceil(v[loose]))), what
        near += int(zone.sum())
        total += int((~tie).sum())
    share = near / max(total, 1)
    print("%s: float32 error %.2e, %.3f %% of the samples are near-ties" % (what, err, 100 * share))
    assert share <= TIE_CAP, (what, share)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES)
def test_planes_against_the_float64_values(hip, pillow_cases, size, fmt):
    for kind in ("noise", "smooth"):
        streams, ref = pillow_cases(size, fmt, kind)
        got, layout, status = _planes(hip, streams)
        assert not status.any() and layout == D.LAYOUT[ref[0][0]["chroma"]]
        assert got.shape == (len(streams), D.frame_bytes(ref[0][0])) and got.dtype == np.uint8
        for b, (info, coef) in enumerate(ref):
            _check_planes(info, coef, got[b], "%s %s %s frame %d" % (size, fmt, kind, b))
        one, _, status = _planes(hip, streams[7:8])      # B = 1
        assert not status.any() and np.array_equal(one[0], got[7])
        # the two halves called one after the other are the decode entry, bit for bit
        coef = hip.jpeg_coefficients_tensor(streams)
        halves, layout2 = hip.jpeg_planes_tensor(coef, streams)
        assert layout2 == layout and np.array_equal(_np(hip, halves), got)


def test_planes_of_own_streams_and_built_blocks(hip):
    """the pixel half on DC coefficients at both ends of their range (the clamp to 0 and to 255) and on the project's own streams"""
    H, W = 48, 80
    ends = np.zeros((90, 64), np.int16)
    ends[::2, 0], ends[1::2, 0] = -1024, 1016
    coef = [ends, R.coefficients(_frames(1, H, W, "noise"), "420", 100)[0], R.coefficients(_frames(1, H, W, "smooth"), "420", 50)[0]]
    streams = [R.stream(c, H, W, "420", q, None) for c, q in zip(coef, (75, 100, 50))]
    got, layout, status = _planes(hip, streams)
    assert layout == "i420" and not status.any()
    for b, s in enumerate(streams):
        info, c = D.coefficients(s)
        assert np.array_equal(c, coef[b])
        _check_planes(info, c, got[b], "own stream %d" % b)
    assert got[0].min() == 0 and got[0].max() == 255


# ---- bad data is a result, not a fault
def _raw_decode(s, streams, canary=512):
    """rrv_jpeg_scan_device and rrv_jpeg_planes_device straight through the C ABI, on buffers with canary bytes behind them"""
    torch = _torch()
    infos, host, cap = F._jpeg_streams(streams)
    B, f = len(streams), infos[0]
    fb = D.frame_bytes(dict(H=f.H, W=f.W, chroma=f.chroma))
    d = torch.from_numpy(host).cuda()
    coef = torch.full((B * f.blocks * 64 + canary,), 0x5A5A, dtype=torch.int16, device="cuda")
    planes = torch.full((B * fb + canary,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((B + canary,), -77, dtype=torch.int32, device="cuda")
    s._chk(s._lib.rrv_jpeg_scan_device(s._h, C.c_void_p(d.data_ptr()), cap, infos, B, C.c_void_p(coef.data_ptr()), C.c_void_p(status.data_ptr()), None))
    s._chk(s._lib.rrv_jpeg_planes_device(s._h, C.c_void_p(coef.data_ptr()), infos, B, C.c_void_p(planes.data_ptr()), None))
    coef, planes, status = _np(s, coef), _np(s, planes), _np(s, status)
    assert np.all(coef[B * f.blocks * 64:] == 0x5A5A) and np.all(planes[B * fb:] == 0xA5) and np.all(status[B:] == -77), "a canary is gone"
    return coef[:B * f.blocks * 64].reshape(B, f.blocks, 64), planes[:B * fb].reshape(B, fb), status[:B]


def test_a_corrupt_frame_is_a_status(hip):
    """a batch of three, the middle frame damaged in four ways, after a larger batch has left its data in the scratch.  Safe by construction:
    jpeg_huff_k's loops run over block and coefficient counts, its stores are indexed by those counters, and jpeg_marks_k writes interval
    starts only at indices below the plan's count (csrc/jpeg_dec_k.h)."""
    H, W = 48, 80
    big = [R.stream(c, 64, 96, "444", 100, 1) for c in R.coefficients(_frames(5, 64, 96, "noise"), "444", 100)]
    _raw_decode(hip, big)
    want = R.coefficients(_frames(3, H, W, "noise", seed=9), "420", 90)
    clean = [R.stream(want[b], H, W, "420", 90, 2) for b in range(3)]      # 15 MCUs: 8 intervals
    c0, p0, st0 = _raw_decode(hip, clean)
    assert not st0.any() and np.array_equal(c0, want)
    pillow = [D.pillow_stream(f, 90, "420") for f in _frames(3, H, W, "noise", seed=9)]      # no restart markers: one lane per frame
    cp, pp, stp = _raw_decode(hip, pillow)
    assert not stp.any()
    cases = [(clean, c0, p0, how) for how in ("truncate", "drop", "swap", "ones")] + [(pillow, cp, pp, "truncate")]
    for streams, c_ok, p_ok, how in cases:
        bad = D.corrupted(streams[1], how) if how != "truncate" else streams[1][:len(streams[1]) // 2]
        with pytest.raises(ValueError):
            D.coefficients(bad)      # (the reference calls it corrupt too)
        mixed = [streams[0], bad, streams[2]]
        c, p, st = _raw_decode(hip, mixed)
        assert st[0] == 0 and st[2] == 0 and 1 <= st[1] <= 7, (how, st)
        if how == "swap":
            assert st[1] == 6, st
        for b in (0, 2):
            assert np.array_equal(c[b], c_ok[b]) and np.array_equal(p[b], p_ok[b]), (how, b)
        with pytest.raises(ValueError, match="frame 1 is corrupt"):
            hip.decode_jpeg_tensor(mixed)
    # the handle decodes as before
    c, p, st = _raw_decode(hip, clean)
    assert not st.any() and np.array_equal(c, c0) and np.array_equal(p, p0)


# ---- refusals and failure paths
def test_the_entries_refuse_in_words(hip):
    torch = _torch()
    a = [D.pillow_stream(f, 90, "420") for f in _frames(2, 17, 23, "smooth")]
    other = D.pillow_stream(_frames(1, 24, 23, "smooth")[0], 90, "420")
    other_chroma = D.pillow_stream(_frames(1, 17, 23, "smooth")[0], 90, "444")
    infos, host, cap = F._jpeg_streams(a)
    d = torch.from_numpy(host).cuda()
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    status = torch.zeros(64, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def decode(infos=infos, B=2, cap=cap, st=status, dst=out):
        rc = hip._lib.rrv_jpeg_decode_device(hip._h, ptr(d), cap, infos, B, ptr(dst) if dst is not None else None, ptr(st) if st is not None else None, None)
        return rc, (hip._lib.rrv_last_error(hip._h) or b"").decode()

    mixed = (L.JpegInfo * 2)(infos[0], F._jpeg_parse(other))
    mixed_chroma = (L.JpegInfo * 2)(infos[0], F._jpeg_parse(other_chroma))
    bent = (L.JpegInfo * 2)(infos[0], infos[1])
    bent[1].blocks += 1
    for kw, word in ((dict(B=0), "batch"), (dict(B=65), "batch"), (dict(st=None), "d_status"), (dict(dst=None), "null"), (dict(infos=None), "null"),
                     (dict(cap=len(a[0]) - 1), "cap"), (dict(infos=mixed), "share H, W"), (dict(infos=mixed_chroma), "share H, W"), (dict(infos=bent), "info 1")):
        rc, msg = decode(**kw)
        assert rc == RRV_E_ARG and word in msg, (kw.keys(), rc, msg)
    rc = hip._lib.rrv_jpeg_scan_device(hip._h, ptr(d), cap, infos, 2, C.c_void_p(out.data_ptr() + 2), ptr(status), None)
    assert rc == RRV_E_ARG and "aligned" in hip._lib.rrv_last_error(hip._h).decode()
    for bad, word in (([a[0], other], "share H, W"), ([a[0], b"nope"], "stream 1"), ([], "non-empty"), (a[0], "list of bytes")):
        with pytest.raises(ValueError, match=word):
            hip.decode_jpeg_tensor(bad)
    with pytest.raises(ValueError, match="progressive"):
        hip.decode_jpeg_tensor([D.pillow_stream(_frames(1, 17, 23, "smooth")[0], 90, "420", progressive=True)])
    # the handle is as usable as before
    rc, msg = decode()
    assert rc == RRV_OK, msg
    got = _np(hip, out)[:2 * D.frame_bytes(D.parse(a[0]))].reshape(2, -1)
    assert np.array_equal(got, _planes(hip, a)[0])


def test_out_of_memory_leaves_the_handle_usable(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    try:
        streams = [D.pillow_stream(f, 90, "420", restart_marker_blocks=2) for f in _frames(2, 17, 23, "noise")]
        # the frame descriptors; then the interval starts; then, the descriptors now in place (grow-only), the coefficient blocks behind the interval starts
        for nth in (1, 2, 2):
            s.debug_fail_alloc(nth)
            with pytest.raises(pkg.RRVError) as e:
                s.decode_jpeg_tensor(streams)
            assert e.value.code == RRV_E_NOMEM
            s.debug_fail_alloc(0)
        got, layout, status = _planes(s, streams)
        assert not status.any()
        for b, data in enumerate(streams):
            info, coef = D.coefficients(data)
            _check_planes(info, coef, got[b], "after the failed allocations, frame %d" % b)
    finally:
        s.close()


def test_several_calls_per_batch_and_debug_mode(pkg, weights):
    """70 streams run as two calls of the entry (64 + 6); RRV_DEBUG=2 verifies after every launch and changes nothing"""
    s = pkg.Stylization(weights, cuda=True)
    try:
        base = [D.pillow_stream(f, 90, "422", restart_marker_rows=1) for f in _frames(5, 17, 23, "noise")]
        streams = [base[b % 5] for b in range(70)]
        got, layout, status = _planes(s, streams)
        assert layout == "i422" and not status.any()
        assert all(np.array_equal(got[b], got[b % 5]) for b in range(70))
        s.set_debug(2)
        again, _, status = _planes(s, base)
        assert not status.any() and np.array_equal(again, got[:5])
    finally:
        s.close()


# ---- JPEG as the input form of a transfer
from conftest import load_golden, fixed_kernels      # noqa: E402


@pytest.fixture(scope="module")
def global_model(pkg, weights):
    s = pkg.Stylization(weights, cuda=True)
    s.set_state(load_golden("global_a")["state"])
    yield s
    s.close()


@pytest.fixture(scope="module")
def frame_model(pkg, weights):
    s = pkg.Stylization(weights, cuda=True, use_Global=False)
    s.prepare_style(pkg.synth_style(64, 64, kind="smooth", seed=7))
    yield s
    s.close()


E2E = {"plain": dict(), "staged": dict(work_size=(32, 48), out_size="source", guide="source", strength=0.6)}


def _e2e_streams(B, H=40, W=56):
    """B Pillow streams of one size, 4:2:0; tables, restart intervals and quality differ frame by frame"""
    kws = ({}, {"optimize": True}, {"restart_marker_blocks": 2}, {"restart_marker_rows": 1})
    return [D.pillow_stream(R.bgr_frames(40 + b, 1, H, W, "smooth")[0], (90, 75, 95)[b % 3], "420", **kws[b % 4]) for b in range(B)]


def _chain(s, streams, H, W, **kw):
    """decode, then the transfer from those planes with JFIF's matrix installed (and the default put back): float32 [B][Ho][Wo][3] on the GPU"""
    torch = _torch()
    planes, name = s.decode_jpeg_tensor(streams)
    s.set_yuv_input_matrix("bt601", True)
    try:
        return s.transfer_tensor(planes, layout=name, size=(H, W), out_layout="nhwc", out_dtype=torch.float32, **kw)
    finally:
        s.set_yuv_input_matrix(None)


@pytest.mark.parametrize("how", sorted(E2E))
@pytest.mark.parametrize("model,B", (("global", 3), ("frame", 3), ("global", 17)))
def test_transfer_from_jpeg_equals_decode_then_transfer(global_model, frame_model, model, B, how):
    """transfer_batch(in_format="jpeg") (rrv_transfer_from_jpeg, which runs rrv_transfer_from_jpeg_view_device per sub-batch of sixteen) ==
    decode_jpeg_tensor followed by transfer_tensor from those planes with the BT.601 full-range input matrix, bit for bit in a fixed kernel mode,
    while the handle holds another matrix (its default, BT.601 limited range) and keeps it; a frame does not depend on B or its position; JPEG
    in with JPEG out == the chain followed by encode_jpeg_tensor"""
    s = global_model if model == "global" else frame_model
    kw, streams = E2E[how], _e2e_streams(B)
    jk = dict(jpeg_quality=85, jpeg_chroma="422", jpeg_restart=3)
    with fixed_kernels(s):
        host = s.transfer_batch(streams, in_format="jpeg", **kw)
        y = _chain(s, streams, 40, 56, **kw)
        want = _np(s, y)
        alone = s.transfer_batch(streams[B - 1:], in_format="jpeg", **kw)
        both = s.transfer_batch(streams, in_format="jpeg", out_format="jpeg", **jk, **kw)
        enc = F.jpeg_frames(*(_np(s, t) for t in s.encode_jpeg_tensor(y, **jk)))
        # the handle's own input matrix is what it was: an I420 call gives what it gave before
        planes, name = s.decode_jpeg_tensor(streams[:1])
        limited = _np(s, s.transfer_tensor(planes, layout=name, size=(40, 56), out_layout="nhwc", out_dtype=_torch().float32, **kw))
    assert host.dtype == np.float32 and host.shape == want.shape
    assert np.array_equal(host, want)
    assert np.array_equal(alone[0], host[B - 1])
    assert both == enc
    assert not np.array_equal(limited[0], want[0])      # (limited range reads the same planes differently: the override mattered)


def test_transfer_from_jpeg_uint8_and_frames_geometry(global_model):
    """uint8 output and the pad / crop geometry of transfer_frames through the same entry"""
    streams = _e2e_streams(3, 41, 57)
    with fixed_kernels(global_model):
        got = global_model.transfer_frames(streams, in_format="jpeg", dtype=np.uint8)
        planes, name = global_model.decode_jpeg_tensor(streams)
        global_model.set_yuv_input_matrix("bt601", True)
        try:
            want = _np(global_model, global_model.transfer_tensor(planes, layout=name, size=(41, 57), out_layout="nhwc", out_dtype=_torch().uint8, pad_crop=True))
        finally:
            global_model.set_yuv_input_matrix(None)
    assert got.shape == (3, 41, 57, 3) and got.dtype == np.uint8 and np.array_equal(got, want)


def test_transfer_from_jpeg_bad_frames_raise_with_the_index(global_model):
    streams = _e2e_streams(18)
    want = global_model.transfer_batch(streams[:2], in_format="jpeg")
    bad = list(streams)
    bad[17] = bad[17][:len(bad[17]) // 2]      # in the second sub-batch
    with pytest.raises(ValueError, match="frame 17 is corrupt"):
        global_model.transfer_batch(bad, in_format="jpeg")
    bad[5] = D.pillow_stream(R.bgr_frames(1, 1, 40, 56, "smooth")[0], 90, "420", progressive=True)
    with pytest.raises(ValueError, match="frame 5.*progressive"):
        global_model.transfer_batch(bad, in_format="jpeg")
    with pytest.raises(ValueError, match="share H, W"):
        global_model.transfer_batch([streams[0], D.pillow_stream(R.bgr_frames(1, 1, 48, 56, "smooth")[0], 90, "420")], in_format="jpeg")
    with pytest.raises(ValueError, match="size="):
        global_model.transfer_batch(streams, in_format="jpeg", size=(40, 56))
    with pytest.raises(ValueError, match="list of bytes"):
        global_model.transfer_batch(np.zeros((2, 40, 56, 3), np.uint8), in_format="jpeg")
    assert np.array_equal(global_model.transfer_batch(streams[:2], in_format="jpeg"), want)      # the handle is as usable as before


def test_add_from_jpeg_gives_the_state_of_the_decoded_planes(pkg, weights):
    """add(in_format="jpeg") + compute, in a fixed kernel mode, gives BIT FOR BIT the state of add from the decoded planes through the same arithmetic:
    the scaled add entry at the planes' own size (work_size=(H, W): every tap weight is 1) with the BT.601 full-range input matrix installed.
    Against the deferred add of the planes (in_format "i420", converted in the first kernel) the states agree within the parity tests' bound on a
    state (tests/state_bounds.py): a second check, on another path."""
    from state_bounds import state_worst
    H, W = 64, 48
    streams = [D.pillow_stream(R.bgr_frames(60 + b, 1, H, W, "smooth")[0], 90, "420", **({"restart_marker_rows": 1} if b else {})) for b in range(3)]
    style = pkg.synth_style(64, 64, kind="smooth", seed=7)
    states = {}
    with fixed_kernels():
        for how in ("jpeg", "scaled", "deferred"):
            s = pkg.Stylization(weights, cuda=True)
            try:
                s.prepare_style(style)
                s.clean()
                if how == "jpeg":
                    s.add(streams[0], in_format="jpeg")
                    s.add(streams[1:], in_format="jpeg")
                else:
                    planes, name = s.decode_jpeg_tensor(streams)
                    assert name == "i420"
                    host = _np(s, planes)
                    s.set_yuv_input_matrix("bt601", True)
                    if how == "scaled":
                        for b in range(3):
                            s.add(host[b], in_format=name, size=(H, W), work_size=(H, W))
                    else:
                        s.add(host, in_format=name, size=(H, W))
                s.compute()
                states[how] = s.get_state()
            finally:
                s.close()
    assert np.array_equal(states["jpeg"], states["scaled"]), int((states["jpeg"] != states["scaled"]).sum())
    worst, where = state_worst(states["jpeg"], states["deferred"])
    print("add from JPEG against the deferred add from the planes: worst state entry at %.1f %% of its bound (%s)" % (100 * worst, where))
    assert worst <= 1.0, where
    s2 = pkg.Stylization(weights, cuda=True)
    try:
        with pytest.raises(ValueError, match="progressive"):
            s2.add(D.pillow_stream(R.bgr_frames(1, 1, H, W, "smooth")[0], 90, "420", progressive=True), in_format="jpeg")
    finally:
        s2.close()


def test_the_device_entries_called_directly(global_model):
    """rrv_transfer_from_jpeg_view_device at B = 20 (above the host twin's sub-batch) on a stream of the caller's, against the host twin; and
    rrv_transfer_jpeg_from_jpeg_view_device with a matte, which only the device entry takes, against decode -> transfer_tensor(matte=,
    out_layout="jpeg") with the BT.601 full-range matrix installed; a refused request queues nothing"""
    torch = _torch()
    s, B, H, W = global_model, 20, 40, 56
    streams = _e2e_streams(B, H, W)
    infos, host, cap = F._jpeg_streams(streams)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    jk = dict(jpeg_quality=85, jpeg_chroma="422", jpeg_restart=3)
    matte = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (1, H, W), dtype=np.uint8)).cuda()
    with fixed_kernels(s):
        want = s.transfer_batch(streams, in_format="jpeg")
        side = torch.cuda.Stream()
        d = torch.from_numpy(host).cuda()
        out = torch.zeros((B, H, W, 3), dtype=torch.float32, device="cuda")
        status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        vo = L.ImageView()
        assert s._lib.rrv_image_view_contiguous(L.ImageDesc(L.DT_F32, L.LAY_HWC_BGR, L.SP_PIXEL), H, W, C.byref(vo)) == 0
        torch.cuda.synchronize()
        # a refused request (an unknown flag) queues nothing: the status words stay what they were
        rc = s._lib.rrv_transfer_from_jpeg_view_device(s._h, ptr(d), cap, infos, B, 0, 0, 0, 0, 0, 0.0, None, ptr(out), C.byref(vo), ptr(status), 1 << 20,
                                                        C.c_void_p(side.cuda_stream))
        assert rc == RRV_E_ARG and "flags" in s._lib.rrv_last_error(s._h).decode()
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == -1).all()
        s._chk(s._lib.rrv_transfer_from_jpeg_view_device(s._h, ptr(d), cap, infos, B, 0, 0, 0, 0, 0, 0.0, None, ptr(out), C.byref(vo), ptr(status), 0,
                                                         C.c_void_p(side.cuda_stream)))
        side.synchronize()
        got = _np(s, out)
        assert not _np(s, status).any()
        # JPEG in, JPEG out, with a matte (one for every frame), three frames on the null stream
        nb = 3
        ocap = F.jpeg_plan(H, W, "422", 3)["bound"]
        data = torch.zeros((nb, ocap), dtype=torch.uint8, device="cuda")
        sizes = torch.zeros((nb,), dtype=torch.int32, device="cuda")
        req = L.Composite(None, matte.data_ptr(), L.DT_U8, 1, L.KEEP_NONE)
        j = F.jpeg_args(85, "422", 3)
        sub = (L.JpegInfo * nb)(*infos[:nb])
        s._chk(s._lib.rrv_transfer_jpeg_from_jpeg_view_device(s._h, ptr(d), cap, sub, nb, 0, 0, 0, 0, 0, 0.0, C.byref(req), C.byref(j), ptr(data), ocap, ptr(sizes),
                                                              ptr(status), 0, None))
        twin = F.jpeg_frames(_np(s, data), _np(s, sizes))
        planes, name = s.decode_jpeg_tensor(streams[:nb])
        s.set_yuv_input_matrix("bt601", True)
        try:
            chain = F.jpeg_frames(*(_np(s, t) for t in s.transfer_tensor(planes, layout=name, size=(H, W), out_layout="jpeg", matte=matte, jpeg_cap=ocap, **jk)))
        finally:
            s.set_yuv_input_matrix(None)
    assert np.array_equal(got, want)
    assert twin == chain


def _driver_model(pkg, weights, models):
    def factory(args, device):
        models.append(pkg.Stylization(weights, cuda=True, device=device))
        models[0].close_for_real, models[0].close = models[0].close, lambda: None
        return models[0]
    return factory


def _avi_chunks(path):
    import struct
    data = open(path, "rb").read()
    at = data.index(b"movi") + 4
    chunks = []
    while data[at:at + 4] == b"00dc":
        n = struct.unpack("<I", data[at + 4:at + 8])[0]
        chunks.append(data[at + 8:at + 8 + n])
        at += 8 + n + (n & 1)
    return chunks


def test_driver_gpu_decode_of_jpg_files(pkg, weights, tmp_path):
    """five 48 x 80 Pillow .jpg files with --gpu-decode: the frames written are transfer_frames(in_format="jpeg") of the files' bytes"""
    from PIL import Image
    DRV = importlib.import_module("rerevst-code_amd.driver")
    streams = [D.pillow_stream(R.bgr_frames(70 + i, 1, 48, 80, "smooth")[0], 90, "420") for i in range(5)]
    for i, data in enumerate(streams):
        (tmp_path / ("f%03d.jpg" % i)).write_bytes(data)
    style = tmp_path / "style.png"
    Image.fromarray(pkg.synth_style(64, 64, kind="smooth", seed=7)[..., ::-1].copy()).save(str(style))
    models = []
    with fixed_kernels():
        rc = DRV.main(["--style", str(style), "--frames", str(tmp_path / "f*.jpg"), "--checkpoint", "synthetic", "--out", str(tmp_path / "out"), "--gpu-decode"],
                      model_factory=_driver_model(pkg, weights, models))
        assert rc == 0
        want = models[0].transfer_frames(streams, in_format="jpeg", dtype=np.uint8)
    models[0].close_for_real()
    # the frame files keep their names, so they are .jpg, written by Pillow from the uint8 frame: the bytes are Pillow's for that frame
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["f%03d.jpg" % i for i in range(5)]
    for i in range(5):
        ref = str(tmp_path / ("ref%03d.jpg" % i))
        DRV.write_image_bgr(ref, want[i])
        assert (tmp_path / "out" / ("f%03d.jpg" % i)).read_bytes() == open(ref, "rb").read(), i
        assert Image.open(ref).size == (80, 48)


def test_driver_avi_to_avi_touches_no_pixel(pkg, weights, tmp_path):
    """an .avi written by MJPGWriter to an .avi with --gpu-jpeg --no-frames: the output chunks are transfer_frames(in_format="jpeg",
    out_format="jpeg") of the input chunks, and no output directory appears"""
    from PIL import Image
    DRV = importlib.import_module("rerevst-code_amd.driver")
    streams = [D.without_dht(D.pillow_stream(R.bgr_frames(80 + i, 1, 48, 80, "smooth")[0], 90, "420")) for i in range(5)]
    src = str(tmp_path / "in.avi")
    w = DRV.MJPGWriter(src, 25, 80, 48)
    for data in streams:
        w.write_jpeg(data, (48, 80))
    w.release()
    style = tmp_path / "style.png"
    Image.fromarray(pkg.synth_style(64, 64, kind="smooth", seed=7)[..., ::-1].copy()).save(str(style))
    models = []
    dst = str(tmp_path / "x.avi")
    with fixed_kernels():
        rc = DRV.main(["--style", str(style), "--frames", src, "--checkpoint", "synthetic", "--out", str(tmp_path / "out"), "--video", dst, "--no-frames",
                       "--gpu-jpeg", "--jpeg-quality", "90"], model_factory=_driver_model(pkg, weights, models))
        assert rc == 0
        want = models[0].transfer_frames(streams, in_format="jpeg", out_format="jpeg", jpeg_quality=90)
    models[0].close_for_real()
    assert not (tmp_path / "out").exists()
    assert _avi_chunks(dst) == want
    assert abs(DRV.MJPGReader(dst).fps - 25) < 1e-9

"""YUV 4:2:2 and 4:4:4 without a GPU: the layout values against the header, rrv_image_view_contiguous / rrv_image_view_check against
tests/chroma_ref.py's formulas (a wrong plane size stops here, before any kernel addresses through it), the numpy converters of
video.py against the same reference, the Y4M writer / reader pair, and the ValueErrors of the Python argument checks."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import chroma_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("rerevst-code_amd._lib")
V = importlib.import_module("rerevst-code_amd.video")
D = importlib.import_module("rerevst-code_amd.driver")
RRV_OK, RRV_E_ARG = 0, -1
H, W = 37, 51
DT_U8, DT_F32, DT_U16 = 0, 1, 2
NEW_LAYOUTS = sorted(R.LAYOUTS.values())
BAD_LAYOUTS = (4, 5, 6, 7, 10, 16, 17, 32, 33, 48, 50, -1)


def layout_info(lay):
    """(dtype, planar, chroma) of a layout value, from the issue's table: base = value & ~0x30, flag = value & 0x30"""
    base, flag = lay & ~0x30, lay & 0x30
    return DT_U16 if base in (8, 9) else DT_U8, base in (2, 8), {0: "420", 0x10: "422", 0x20: "444"}[flag]


@pytest.fixture(scope="module")
def lib():
    importlib.import_module("rerevst-code_amd.build").build_lib(verbose=False)
    return L.load()


def test_enum_values_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "rerevst_hip.h")).read()
    assert re.search(r"RRV_LAY_422\s*=\s*0x10\b", hdr) and re.search(r"RRV_LAY_444\s*=\s*0x20\b", hdr)
    assert (L.LAY_422, L.LAY_444) == (0x10, 0x20)
    for name, value in R.LAYOUTS.items():
        assert getattr(L, name[4:]) == value, name
        assert re.search(r"\b%s\s*=" % name, hdr), name
    assert [L.LAY_I422, L.LAY_NV16, L.LAY_I422_16, L.LAY_P216, L.LAY_I444, L.LAY_NV24, L.LAY_I444_16, L.LAY_P416] == [18, 19, 24, 25, 34, 35, 40, 41]
    for name in R.NEW_FORMATS:                      # the sixteen names, with the values and fields of the reference table
        lay, planar, chroma, bits = R.FORMATS[name]
        f = V.YUV_FORMATS[name]
        assert (f.layout, f.planar, f.chroma, f.bits, f.dtype) == (lay, planar, chroma, bits, np.dtype(np.uint8 if bits == 8 else np.uint16)), name
    assert len(R.NEW_FORMATS) == 16 and all(V.YUV_FORMATS[n].chroma == "420" for n in ("i420", "nv12", "i420p10", "p016"))


def test_bad_layout_values_are_refused(lib):
    v = L.ImageView()
    for lay in BAD_LAYOUTS:
        for dt in (DT_U8, DT_U16, DT_F32):
            assert lib.rrv_image_view_contiguous(L.ImageDesc(dt, lay, 0), H, W, C.byref(v)) == RRV_E_ARG, (lay, dt)
    for lay in NEW_LAYOUTS:                         # the new layouts with the wrong dtype or space
        dt = layout_info(lay)[0]
        assert lib.rrv_image_view_contiguous(L.ImageDesc(DT_U16 if dt == DT_U8 else DT_U8, lay, 0), H, W, C.byref(v)) == RRV_E_ARG
        assert lib.rrv_image_view_contiguous(L.ImageDesc(DT_F32, lay, 0), H, W, C.byref(v)) == RRV_E_ARG
        assert lib.rrv_image_view_contiguous(L.ImageDesc(dt, lay, 1), H, W, C.byref(v)) == RRV_E_ARG


@pytest.mark.parametrize("lay", NEW_LAYOUTS)
def test_contiguous_view_equals_the_reference_formulas(lib, lay):
    dt, planar, chroma = layout_info(lay)
    v = L.ImageView()
    assert lib.rrv_image_view_contiguous(L.ImageDesc(dt, lay, 0), H, W, C.byref(v)) == RRV_OK
    fs, off, pitch = R.contiguous_view(H, W, planar, chroma)
    table = R.plane_table(H, W, planar, chroma)
    n = len(table)
    assert (v.desc.dtype, v.desc.layout, v.desc.space) == (dt, lay, 0)
    assert v.frame_stride == fs == R.frame_samples(H, W, chroma)
    assert list(v.plane_offset)[:n] == off and list(v.pitch)[:n] == pitch
    # the largest element any plane row reaches is the frame's last: no plane is sized for another chroma format
    reach = max(v.plane_offset[k] + (rows - 1) * v.pitch[k] + ln - 1 for k, (ln, rows) in enumerate(table))
    assert reach == fs - 1
    # and the planes tile the frame: sorted by offset, each starts where the previous one ends
    ends = sorted((v.plane_offset[k], v.plane_offset[k] + rows * ln) for k, (ln, rows) in enumerate(table))
    assert ends[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] == fs
    assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 1) == RRV_OK
    assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 0) == RRV_OK


def test_frame_sizes_by_hand():
    # 37 x 51: 4:2:2 has CH = 37, CW = 26; 4:4:4 CH = 37, CW = 51
    assert R.frame_samples(H, W, "422") == 37 * 51 + 2 * 37 * 26 == 3811
    assert R.frame_samples(H, W, "444") == 3 * 37 * 51 == 5661
    assert R.frame_samples(H, W, "420") == 37 * 51 + 2 * 19 * 26
    assert V.yuv_frame_bytes(H, W, chroma="422") == 3811 and V.yuv_frame_bytes(H, W, 10, "444") == 2 * 5661
    assert V.yuv_frame_bytes(H, W) == 37 * 51 + 2 * 19 * 26 and V.chroma_plane_size(H, W, "422") == (37, 26)


def _view(dt, lay, fs, off, pitch):
    v = L.ImageView()
    v.desc, v.frame_stride = L.ImageDesc(dt, lay, 0), fs
    for k in range(len(off)):
        v.plane_offset[k], v.pitch[k] = off[k], pitch[k]
    return v


def test_view_check_on_pitched_surfaces(lib):
    for dt, lay in ((DT_U8, L.LAY_NV16), (DT_U16, L.LAY_P216)):       # a capture card's surface: pitch 64, the chroma plane at its own offset
        v = _view(dt, lay, 64 * 40 * 2 + 128, [0, 64 * 40], [64, 64])
        assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 0) == RRV_OK
        assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 1) == RRV_OK
        v.plane_offset[1] = 64 * 36                                     # the chroma plane starts inside the last luma row
        assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 0) == RRV_OK
        assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 1) == RRV_E_ARG
        v.plane_offset[1] = 64 * 40
        v.frame_stride = 64 * 40 + 64 * 36                             # 4:2:2 chroma has H = 37 rows, not 19: the next frame would start inside it
        assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 1) == RRV_E_ARG
        v.pitch[1] = 51                                                  # 2 CW = 52 elements per chroma row
        assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 0) == RRV_E_ARG
    for dt, lay in ((DT_U8, L.LAY_NV24), (DT_U16, L.LAY_P416)):       # 4:4:4 semi-planar: a chroma row is 2W elements
        good = _view(dt, lay, 0, [0, 64 * 40], [64, 2 * W])
        assert lib.rrv_image_view_check(C.byref(good), 1, H, W, 1) == RRV_OK
        short = _view(dt, lay, 0, [0, 64 * 40], [64, 2 * W - 1])
        assert lib.rrv_image_view_check(C.byref(short), 1, H, W, 0) == RRV_E_ARG
        half = _view(dt, lay, 0, [0, 64 * 40], [64, 2 * ((W + 1) // 2)])   # the 4:2:2 row length
        assert lib.rrv_image_view_check(C.byref(half), 1, H, W, 0) == RRV_E_ARG
    planar = _view(DT_U8, L.LAY_I444, 0, [0, 64 * 40, 64 * 40 + 10], [64, 64, 64])      # Cb and Cr overlap
    assert lib.rrv_image_view_check(C.byref(planar), 1, H, W, 0) == RRV_OK
    assert lib.rrv_image_view_check(C.byref(planar), 1, H, W, 1) == RRV_E_ARG


@pytest.mark.parametrize("fmt", R.NEW_FORMATS)
def test_video_converters_equal_the_reference(fmt):
    lay, planar, chroma, bits = R.FORMATS[fmt]
    rng = np.random.default_rng(bits + lay)
    img = (rng.random((2, H, W, 3)) * 300 - 20).astype(np.float32)       # beyond 0..255: both clamps of the output conversion fire
    got = V.bgr_to_yuv420(img, R.M(fmt), "i420" if planar else "nv12", bits=bits, chroma=chroma)
    want = R.yuv_ref(img, fmt)
    assert got.dtype == want.dtype and got.shape == (2, R.frame_samples(H, W, chroma))
    np.testing.assert_array_equal(got, want)
    buf = R.random_samples(7 + lay, 2, H, W, fmt)
    back = V.yuv420_to_bgr(buf, H, W, R.N(fmt), "i420" if planar else "nv12", bits=bits, chroma=chroma)
    ref = R.bgr_ref(buf, H, W, fmt)
    assert back.dtype == np.float32 and ref.min() == 0.0 and ref.max() == 255.0
    np.testing.assert_array_equal(back, ref)
    np.testing.assert_array_equal(V.yuv_matrix(bits=bits), R.M(fmt))
    np.testing.assert_array_equal(V.yuv_input_matrix(bits=bits), R.N(fmt))


def test_pair_mean_by_hand():
    """4:2:2: (l + r) * 0.5f per row, the last odd column paired with itself; 4:4:4: the pixel's own value"""
    m = np.zeros((3, 4), np.float32)
    m[0, 1] = m[1, 2] = m[2, 0] = 1.0                 # Y = G, Cb = B, Cr = R
    img = np.zeros((1, 2, 3, 3), np.float32)            # BGR
    img[0, :, :, 0] = [[10, 21, 7], [0, 255, 200]]
    img[0, :, :, 2] = [[1, 2, 3], [4, 5, 6]]
    got = R.yuv_ref(img, "i422", m)[0]
    np.testing.assert_array_equal(got[6:10], [16, 7, 128, 200])      # rint(15.5) = 16 (half to even), 7; rint(127.5) = 128, 200
    np.testing.assert_array_equal(got[10:14], [2, 3, 4, 6])          # rint(1.5) = 2, 3; rint(4.5) = 4, 6
    got = R.yuv_ref(img, "nv24", m)[0]
    np.testing.assert_array_equal(got[6:12], [10, 1, 21, 2, 7, 3])


@pytest.mark.parametrize("tag,chroma,bits", [("422", "422", 8), ("444", "444", 8), ("422p10", "422", 10), ("444p12", "444", 12)])
def test_y4m_round_trip(tmp_path, tag, chroma, bits):
    h, w = 10, 15
    fmt = "i" + chroma + ("" if bits == 8 else "p%d" % bits)
    frames = R.random_samples(3, 3, h, w, fmt)
    path = str(tmp_path / "t.y4m")
    wr = D.Y4MWriter(path, (30000, 1001), w, h, full_range=True, bits=bits, chroma=chroma)
    assert wr.frame_bytes == R.frame_samples(h, w, chroma) * (1 if bits == 8 else 2)
    for fr in frames:
        wr.append(fr, (h, w))
    with pytest.raises(ValueError):
        wr.append(frames[0][:-1], (h, w))
    wr.release()
    head = open(path, "rb").readline()
    assert head == b"YUV4MPEG2 W15 H10 F30000:1001 Ip A1:1 C%s XCOLORRANGE=FULL\n" % tag.encode()
    with D.Y4MReader(path, high_depth=True, chroma=True) as r:
        assert (r.width, r.height, r.fps, r.colorspace, r.chroma, r.bits, r.full_range, len(r)) == (w, h, (30000, 1001), tag, chroma, bits, True, 3)
        assert r.frame_samples == R.frame_samples(h, w, chroma) and r.frame_bytes == wr.frame_bytes
        got = np.stack([r.read(i) for i in (2, 0, 1)])
        np.testing.assert_array_equal(got, frames[[2, 0, 1]])
        run = np.empty((2, r.frame_samples), frames.dtype)
        r.read_run(1, run)
        np.testing.assert_array_equal(run, frames[1:])
    fields, raw = D.read_y4m(path, high_depth=True, chroma=True)
    assert b"C" + tag.encode() in fields and [len(x) for x in raw] == [wr.frame_bytes] * 3
    np.testing.assert_array_equal(np.frombuffer(raw[1], frames.dtype if bits == 8 else "<u2"), frames[1])
    # the defaults refuse the file by its tag, as before; each option alone opens only its own half
    for kw in ({}, {"high_depth": True}) + (({"chroma": True},) if bits > 8 else ()):
        with pytest.raises(ValueError, match="C" + tag):
            D.Y4MReader(path, **kw)


def test_y4m_420_tags_are_unchanged(tmp_path):
    for bits, tag in ((8, b"C420jpeg"), (10, b"C420p10")):
        path = str(tmp_path / ("a%d.y4m" % bits))
        D.Y4MWriter(path, 24, 16, 8, bits=bits).release()
        assert open(path, "rb").readline() == b"YUV4MPEG2 W16 H8 F24:1 Ip A1:1 " + tag + b" XCOLORRANGE=LIMITED\n"
        with D.Y4MReader(path, high_depth=True, chroma=True) as r:
            assert r.chroma == "420" and r.bits == bits


def test_python_argument_checks(tmp_path):
    F = importlib.import_module("rerevst-code_amd.framework")
    with pytest.raises(ValueError):
        V.yuv_frame_bytes(H, W, chroma="411")
    with pytest.raises(ValueError):
        V.bgr_to_yuv420(np.zeros((2, 2, 3), np.float32), R.M("i422"), chroma="440")
    with pytest.raises(ValueError):
        V.yuv420_to_bgr(np.zeros(R.frame_samples(H, W, "420"), np.uint8), H, W, R.N("i422"), chroma="422")      # a 4:2:0 sample count
    with pytest.raises(ValueError):
        D.Y4MWriter(str(tmp_path / "x.y4m"), 24, 16, 8, chroma="4:2:2")
    assert "i422p14" not in V.YUV_FORMATS
    with pytest.raises(ValueError, match="i422p14"):
        F.yuv_frames_args(np.zeros((1, 10), np.uint16), "i422p14", (H, W))
    with pytest.raises(ValueError):
        F.yuv_planes(np.zeros(10, np.uint8), H, W, "i422p14")
    n = R.frame_samples(H, W, "422")
    with pytest.raises(ValueError):
        F.yuv_frames_args(np.zeros((2, n), np.uint8), "p210", (H, W))               # a uint8 array for a uint16 format
    with pytest.raises(ValueError):
        F.yuv_frames_args(np.zeros((2, R.frame_samples(H, W, "420")), np.uint16), "p210", (H, W))      # the 4:2:0 sample count
    with pytest.raises(ValueError):
        F.yuv_frames_args(np.zeros((2, n), np.uint16), "p210", None)                # no size
    a, h, w = F.yuv_frames_args(np.zeros((2, n), np.uint16), "p210", (H, W))
    assert a.shape == (2, n) and (h, w) == (H, W)
    y, cb, cr = F.yuv_planes(np.arange(R.frame_samples(4, 6, "444"), dtype=np.uint8), 4, 6, "nv24")
    assert y.shape == (4, 6) and cb.shape == cr.shape == (4, 6) and cb[0, 1] == 26 and cr[0, 1] == 27
    y, cb, cr = F.yuv_planes(np.zeros((2, n), np.uint16), H, W, "i422p10")
    assert cb.shape == (2, 37, 26)
    with pytest.raises(ValueError):
        D.check_chroma("422", False)                  # 4:2:2 with PNG-only output: no .y4m to carry it
    with pytest.raises(ValueError):
        D.stylize_files(None, "s.png", ["a.png"], str(tmp_path / "o"), video_path=None, chroma="422")
    with pytest.raises(ValueError):
        D.stylize_files(None, "s.png", ["a.png"], str(tmp_path / "o"), video_path=str(tmp_path / "v.avi"), chroma="444")
    with pytest.raises(SystemExit):                   # the command line says the same before any model exists
        D.main(["--style", __file__, "--frames", "*.png", "--checkpoint", "synthetic", "--out", str(tmp_path / "o"), "--chroma", "422"])
    assert D.check_chroma("444", True) == "444" and D.y4m_format("422", 10) == "i422p10" and D.y4m_format("420", 8) == "i420"


torch = pytest.importorskip("torch")


def test_image_view_of_yuv_tensors(lib):
    F = importlib.import_module("rerevst-code_amd.framework")
    n = R.frame_samples(H, W, "422")
    big = torch.zeros((6, n + 9), dtype=torch.int16)
    t = big[::2, :n]                                   # every second frame of a pitched buffer
    v = F.image_view_of(t, "p210", size=(H, W))
    fs, off, pitch = R.contiguous_view(H, W, False, "422")
    assert v is not None and v.frame_stride == 2 * (n + 9) and list(v.plane_offset)[:2] == off and list(v.pitch)[:2] == pitch
    assert (v.desc.dtype, v.desc.layout) == (DT_U16, L.LAY_P216)
    assert lib.rrv_image_view_check(C.byref(v), 3, H, W, 1) == RRV_OK
    assert F.image_view_of(t[:, ::2], "p210", size=(H, W)) is None                    # sample stride 2
    assert F.image_view_of(t.to(torch.uint8), "p210", size=(H, W)) is None           # bytes for a uint16 format
    assert F.image_view_of(big[:, :n - 1], "p210", size=(H, W)) is None              # not a frame's sample count
    with pytest.raises(ValueError):
        F.image_view_of(t, "p210")                     # a YUV name needs the size
    with pytest.raises(ValueError):
        F.image_view_of(t, "i422p14", size=(H, W))

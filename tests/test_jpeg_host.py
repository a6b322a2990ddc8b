"""JPEG output (include/rerevst_hip.h "JPEG output") without a GPU: the reference (tests/jpeg_ref.py) against Pillow, the table, bound and
plan functions against Pillow and the reference, the ledger of librerevst_jpeg.so, and the Python and driver surface.  What needs a handle is
in tests/test_gpu_jpeg.py."""
import ctypes as C
import importlib
import io
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as R
import kernel_ledger

L = importlib.import_module("rerevst-code_amd._lib")
assert "rrv_jpeg_encode_device" in L.SYMBOLS

F = importlib.import_module("rerevst-code_amd.framework")
D = importlib.import_module("rerevst-code_amd.driver")
BUILD = importlib.import_module("rerevst-code_amd.build")

RRV_OK, RRV_E_ARG = 0, -1
GJ = "tests/test_gpu_jpeg.py::"
# kernel symbol of librerevst_jpeg.so -> the GPU test that holds THAT instantiation to the reference
JPEG_LEDGER = {
    "jpeg_blocks_k<2, 2>": GJ + "test_blocks_against_the_float64_transform",      # [*-420-*]
    "jpeg_blocks_k<2, 1>": GJ + "test_blocks_against_the_float64_transform",      # [*-422-*]
    "jpeg_blocks_k<1, 1>": GJ + "test_blocks_against_the_float64_transform",      # [*-444-*]
    "jpeg_entropy_k<0>": GJ + "test_streams_of_built_blocks",                     # the lengths place every interval: a wrong one moves the bytes behind it
    "jpeg_entropy_k<1>": GJ + "test_streams_of_built_blocks",
    "jpeg_place_k": GJ + "test_a_cap_one_byte_short",                             # offsets, sizes against cap, header and EOI
}
SIZES = ((1, 1), (8, 8), (17, 23), (16, 16), (48, 80))
PIL_SUB = {"444": 0, "422": 1, "420": 2}
DECODE_MARGIN = 1.05      # of Pillow's own decode error; the reference alone is measured against it below


def test_jpeg_ledger_matches_the_library():
    """the fourth library's kernels are exactly the ledger's keys, every cited test exists and is parametrised over the chroma formats, and the
    other three libraries hold no kernel of it"""
    BUILD.build_lib(verbose=False)
    mine = kernel_ledger.symbols(BUILD.JPEG_LIB)
    assert len(mine) == len(set(mine))
    assert set(mine) == set(JPEG_LEDGER), (sorted(set(mine) - set(JPEG_LEDGER)), sorted(set(JPEG_LEDGER) - set(mine)))
    for key, ref in JPEG_LEDGER.items():
        path, name = ref.split("::")
        assert os.path.isfile(os.path.join(kernel_ledger.ROOT, path)), (key, ref)
        mod = importlib.import_module(os.path.splitext(os.path.basename(path))[0])
        assert callable(getattr(mod, name, None)), (key, ref)
    gpu = importlib.import_module("test_gpu_jpeg")
    assert {R.FACTORS[c] for c in gpu.CHROMAS} == {(2, 2), (2, 1), (1, 1)}
    for lib in (BUILD.LIB, BUILD.STAGES_LIB, BUILD.COMPOSE_LIB):
        assert not [s for s in kernel_ledger.symbols(lib) if "jpeg" in s]


# ---- the reference against Pillow
def _decode(stream):
    im = Image.open(io.BytesIO(stream))
    im.load()
    return im


def _pil_tables(im):
    """Pillow's two quantisation tables as it reports them: natural order in current versions, zigzag order in old ones (the callers accept both)"""
    return [np.array(im.quantization[i]) for i in (0, 1)]


@pytest.mark.parametrize("restart", (1, 4, "row", None))
@pytest.mark.parametrize("chroma", ("420", "422", "444"))
@pytest.mark.parametrize("size", SIZES)
def test_pillow_opens_the_references_streams(size, chroma, restart):
    H, W = size
    r = R.plan(H, W, chroma)["mcu_cols"] if restart == "row" else restart
    x = R.bgr_frames(2, 1, H, W, "smooth")
    s = R.encode(x, chroma, 90, r)[0]
    assert s[:2] == b"\xff\xd8" and s[-2:] == b"\xff\xd9" and len(s) <= F.jpeg_plan(H, W, chroma, r)["bound"]
    im = _decode(s)
    assert im.size == (W, H) and im.mode == "RGB"
    lu, ch = R.tables(90)
    got = _pil_tables(im)
    assert any(np.array_equal(got[0], t) and np.array_equal(got[1], u) for t, u in ((lu, ch), (lu[R.ZIGZAG], ch[R.ZIGZAG])))
    err = np.abs(np.asarray(im).astype(np.float64)[..., ::-1] - np.clip(x[0], 0, 255)).mean()
    assert err < 12.0, err      # a picture of the source, not noise (a smooth frame; the tight comparison is below)


def _errors(kind, chroma, quality, H=48, W=80):
    x = R.bgr_frames(7, 1, H, W, kind)[0]
    src = np.clip(x, 0, 255)
    ours = np.abs(np.asarray(_decode(R.encode(x[None], chroma, quality)[0])).astype(np.float64)[..., ::-1] - src).mean()
    buf = io.BytesIO()
    Image.fromarray(np.clip(np.rint(x[..., ::-1]), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=quality, subsampling=PIL_SUB[chroma])
    pil = np.abs(np.asarray(_decode(buf.getvalue())).astype(np.float64)[..., ::-1] - src).mean()
    return float(ours), float(pil)


@pytest.mark.parametrize("quality", (50, 90))
@pytest.mark.parametrize("chroma", ("420", "422", "444"))
@pytest.mark.parametrize("kind", ("noise", "smooth"))
def test_reference_decodes_as_well_as_pillows_encode(kind, chroma, quality):
    """the two encoders share tables and subsampling and differ in sample rounding and in float64 against libjpeg's integer DCT: the decoded
    picture's mean absolute error stays within 5 % of that of Pillow's own encode (profiles/jpeg.txt holds the figures)"""
    ours, pil = _errors(kind, chroma, quality)
    print("%s %s q%d: reference %.4f, Pillow %.4f, ratio %.4f" % (kind, chroma, quality, ours, pil, ours / pil))
    assert ours <= DECODE_MARGIN * pil


# ---- tables, bound, plan
@pytest.mark.parametrize("quality", (1, 10, 50, 75, 90, 100))
def test_tables_are_pillows(quality):
    lu, ch = F.jpeg_tables(quality)
    rl, rc = R.tables(quality)
    assert np.array_equal(lu, rl) and np.array_equal(ch, rc)
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", quality=quality)
    got = _pil_tables(_decode(buf.getvalue()))
    assert any(np.array_equal(got[0], t) and np.array_equal(got[1], u) for t, u in ((lu, ch), (lu[R.ZIGZAG], ch[R.ZIGZAG])))


def test_huffman_tables_are_pillows():
    """Pillow writes the Annex K tables into every non-optimised file: the DHT segments of the reference's header are those"""
    def dht(data):
        out, i = {}, 2
        while data[i + 1] != 0xDA:
            n = data[i + 2] << 8 | data[i + 3]
            if data[i + 1] == 0xC4:
                body = data[i + 4:i + 2 + n]
                while body:
                    k = sum(body[1:17])
                    out[body[0]] = bytes(body[1:17 + k])
                    body = body[17 + k:]
            i += 2 + n
        return out
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (32, 32, 3)).astype(np.uint8)).save(buf, "JPEG", quality=90)
    assert dht(buf.getvalue()) == dht(R.header(32, 32, "420", 90, 2)) and len(dht(buf.getvalue())) == 4


@pytest.mark.parametrize("restart", (None, 1, 7, 65535))
@pytest.mark.parametrize("chroma", ("420", "422", "444"))
@pytest.mark.parametrize("size", SIZES + ((2160, 3840), (65535, 9)))
def test_plan_and_bound_are_the_references_counts(size, chroma, restart):
    H, W = size
    got, want = F.jpeg_plan(H, W, chroma, restart), R.plan(H, W, chroma, restart)
    assert {k: got[k] for k in ("mcu_cols", "mcu_rows", "interval", "blocks", "header_bytes")} == {k: want[k] for k in ("mcu_cols", "mcu_rows", "interval", "blocks", "header_bytes")}
    # every block at its longest code (9 + 11 + 63 x 26 bits), every byte stuffed, padding and RST per interval, header and EOI
    assert got["bound"] >= want["header_bytes"] + 2 * -(-want["blocks"] * 1658 // 8) + 4 * want["intervals"] + 2


def test_bound_holds_for_the_longest_codes():
    """every AC at +-1023 and the DC jumping: the reference's stream stays below the bound, and is most of it"""
    H, W = 24, 40
    for chroma in ("420", "444"):
        for r in (1, None):
            p = R.plan(H, W, chroma, r)
            c = np.full((p["blocks"], 64), 1023, np.int16)
            c[::2, 1::2] = -1023
            c[::2, 0], c[1::2, 0] = -1024, 1016
            n = len(R.stream(c, H, W, chroma, 90, r))
            bound = F.jpeg_plan(H, W, chroma, r)["bound"]
            assert bound // 3 < n <= bound, (chroma, r, n, bound)


def test_the_handle_free_entries_refuse_bad_arguments():
    lib = L.load()
    lu, ch = (C.c_uint16 * 64)(), (C.c_uint16 * 64)()
    n, v = C.c_size_t(0), [C.c_int(0) for _ in range(5)]
    assert lib.rrv_jpeg_tables(90, lu, ch) == RRV_OK
    for q in (0, 101, -5):
        assert lib.rrv_jpeg_tables(q, lu, ch) == RRV_E_ARG
    assert lib.rrv_jpeg_tables(90, None, ch) == RRV_E_ARG
    for H, W, chroma, restart in ((0, 8, 420, 0), (8, 0, 420, 0), (65536, 8, 420, 0), (8, 8, 411, 0), (8, 8, 420, -1), (8, 8, 420, 65536)):
        assert lib.rrv_jpeg_bound(H, W, chroma, restart, C.byref(n)) == RRV_E_ARG
        assert lib.rrv_jpeg_plan(H, W, chroma, restart, *(C.byref(x) for x in v)) == RRV_E_ARG
    assert lib.rrv_jpeg_bound(8, 8, 420, 0, None) == RRV_E_ARG
    assert lib.rrv_jpeg_bound(8, 8, 444, 0, C.byref(n)) == RRV_OK and n.value > 629


def test_the_request_struct_is_the_headers():
    assert [f[0] for f in L.Jpeg._fields_] == ["quality", "chroma", "restart"] and C.sizeof(L.Jpeg) == 12
    header = open(os.path.join(kernel_ledger.ROOT, "include", "rerevst_hip.h")).read()
    body = header[header.index("typedef struct rrv_jpeg {"):header.index("} rrv_jpeg;")]
    assert [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln] == ["quality", "chroma", "restart"]


# ---- the Python surface refuses in words, before any GPU work
@pytest.mark.parametrize("kw,word", (({"quality": 0}, "jpeg_quality"), ({"quality": 101}, "jpeg_quality"), ({"quality": 90.5}, "jpeg_quality"),
                                     ({"chroma": "411"}, "jpeg_chroma"), ({"restart": 0}, "jpeg_restart"), ({"restart": 65536}, "jpeg_restart")))
def test_jpeg_args_refuse(kw, word):
    with pytest.raises(ValueError, match=word):
        F.jpeg_args(**kw)


def test_jpeg_args_and_cap_defaults():
    j = F.jpeg_args()
    assert (j.quality, j.chroma, j.restart) == (90, 420, 0)
    assert F.jpeg_args(75, 444, 12).chroma == 444 and F.jpeg_args(75, "422", 12).restart == 12
    assert F.jpeg_slot_bytes(480, 640) == 2 * 480 * 640 + 629 + 2      # two bytes per delivered pixel plus the header (and EOI)
    assert F.jpeg_slot_bytes(8, 8, "444") == 2 * 64 + 631 <= F.jpeg_plan(8, 8, "444")["bound"]
    with pytest.raises(ValueError, match="jpeg_cap"):
        F.jpeg_slot_bytes(480, 640, cap=600)      # too small for the header
    assert F.jpeg_slot_bytes(480, 640, cap=631) == 631


def test_jpeg_frames_names_the_cap():
    data = np.zeros((2, 700), np.uint8)
    assert F.jpeg_frames(data, np.array([650, 640], np.int32)) == [bytes(650), bytes(640)]
    with pytest.raises(ValueError, match="jpeg_cap.*frame 1 needs 900"):
        F.jpeg_frames(data, np.array([650, -900], np.int32))


class _NoGpu(F.Stylization):
    """the keyword checks of the transfer calls run before the library is asked for anything"""
    def __init__(self):
        self.use_Global, self.style_num, self.device = True, 1, 0


def test_transfer_calls_refuse_jpeg_combinations():
    s = _NoGpu()
    x = np.zeros((2, 16, 16, 3), np.uint8)
    for kw, word in ((dict(style_weights=[1.0]), "style_weights"), (dict(style_masks=np.ones((1, 16, 16), np.float32)), "style_masks"),
                     (dict(dtype=np.uint8), "dtype="), (dict(out=np.zeros((2, 16, 16, 3), np.float32)), "out="),
                     (dict(jpeg_quality=0), "jpeg_quality"), (dict(jpeg_quality=101), "jpeg_quality"), (dict(jpeg_chroma="411"), "jpeg_chroma")):
        for call in (s.transfer_batch, s.transfer_frames):
            with pytest.raises(ValueError, match=word):
                call(x, out_format="jpeg", **kw)
    with pytest.raises(ValueError, match="jpeg_cap"):
        s.transfer_batch(x, out_format="jpeg", jpeg_cap=100)


# ---- driver flags
def test_driver_flags_reach_the_flow(tmp_path, monkeypatch):
    seen = {}

    def fake(model, style, frames, out, video, fps, **kw):
        seen.update(kw, video=video)
        return []
    monkeypatch.setattr(D, "stylize_files", fake)
    monkeypatch.setattr(D, "list_frames", lambda pattern: ["a.png"])
    style = tmp_path / "s.png"
    Image.new("RGB", (8, 8)).save(str(style))
    base = ["--style", str(style), "--frames", "x*.png", "--checkpoint", "synthetic", "--out", str(tmp_path / "o")]
    factory = lambda args, device: object()
    assert D.main(base + ["--video", str(tmp_path / "v.avi"), "--no-frames", "--gpu-jpeg"], model_factory=factory) == 0
    assert seen["gpu_jpeg"] == dict(quality=95, chroma="420") and seen["write_frames"] is False
    seen.clear()
    assert D.main(base + ["--gpu-jpeg", "--jpeg-quality", "80", "--jpeg-chroma", "444"], model_factory=factory) == 0
    assert seen["gpu_jpeg"] == dict(quality=80, chroma="444") and seen["write_frames"] is True
    seen.clear()
    assert D.main(base + ["--video", str(tmp_path / "v.avi")], model_factory=factory) == 0
    assert "gpu_jpeg" not in seen      # without the flag the driver is what it was
    for bad in (["--gpu-jpeg", "--video", str(tmp_path / "v.y4m")], ["--gpu-jpeg", "--jpeg-quality", "0"], ["--gpu-jpeg", "--gpus", "2"]):
        with pytest.raises(SystemExit):
            D.main(base + bad, model_factory=factory)


def test_stylize_files_refuses_gpu_jpeg_without_the_model(tmp_path):
    class Plain:
        use_Global = True
    with pytest.raises(ValueError, match="gpu_jpeg"):
        D.stylize_files(Plain(), "s.png", ["a.png"], str(tmp_path), gpu_jpeg=dict(quality=90))
    with pytest.raises(ValueError, match="y4m"):
        D.stylize_files(Plain(), "s.png", ["a.png"], str(tmp_path), video_path=str(tmp_path / "v.y4m"), gpu_jpeg=dict(quality=90))

"""Shots (include/rerevst_hip.h "Shots", INTEGRATION.md "Shots") without a GPU: the ledger of librerevst_shots.so, the thumbnail plan,
video.shot_signature on inputs with known answers, the distance and the cut rule on a synthetic video, the shots file, and the driver's
control flow with a model that only records its calls.  The kernel and the entries are held to these in tests/test_gpu_shots.py."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import kernel_ledger

L = importlib.import_module("rerevst-code_amd._lib")
F = importlib.import_module("rerevst-code_amd.framework")
V = importlib.import_module("rerevst-code_amd.video")
D = importlib.import_module("rerevst-code_amd.driver")
BUILD = importlib.import_module("rerevst-code_amd.build")

GS = "tests/test_gpu_shots.py::"
# kernel symbol of librerevst_shots.so -> the GPU test that holds it to video.shot_signature, word for word
SHOTS_LEDGER = {
    "shot_sig_k": GS + "test_kernel_equals_the_numpy_restatement",
}

PLANS = {(512, 512): (512, 512), (1080, 1920): (270, 480), (2160, 3840): (270, 480), (4320, 7680): (540, 960)}
SHOT_LENGTHS = (11, 9, 13, 1)
CUTS = [0, 11, 20, 33]
SIZES = ((48, 64), (37, 53))


def synthetic_video(H, W):
    """Four shots of 11, 9, 13 and 1 uint8 BGR frames of H x W: shot k is a 9 x 9 box-blurred default_rng(100 + k) field stretched to a
    brightness range, [0, 100] and [150, 255] in turn, and each frame is the field one pixel further along x than the frame before."""
    frames = []
    for k, n in enumerate(SHOT_LENGTHS):
        f = np.random.default_rng(100 + k).random((H + 8, W + n - 1 + 8, 3))
        c = np.pad(np.cumsum(np.cumsum(f, 0), 1), ((1, 0), (1, 0), (0, 0)))
        blur = (c[9:, 9:] - c[:-9, 9:] - c[9:, :-9] + c[:-9, :-9]) / 81.0      # [H][W + n - 1][3]
        lo, hi = (0.0, 100.0) if k % 2 == 0 else (150.0, 255.0)
        u8 = np.rint(lo + (blur - blur.min()) / (blur.max() - blur.min()) * (hi - lo)).astype(np.uint8)
        frames += [np.ascontiguousarray(u8[:, j:j + W]) for j in range(n)]
    return frames


_VIDEOS = {}


def video_and_signatures(H, W):
    """the synthetic video and its numpy signatures, computed once per size"""
    if (H, W) not in _VIDEOS:
        frames = synthetic_video(H, W)
        _VIDEOS[H, W] = (frames, np.stack([V.shot_signature(f) for f in frames]))
    return _VIDEOS[H, W]


def cell_pixels(H, W):
    """[16] pixel counts of the cells: cell row cy holds the rows ceil(cy H / 4) .. ceil((cy + 1) H / 4) - 1"""
    ys = [-(-c * H // 4) for c in range(5)]
    xs = [-(-c * W // 4) for c in range(5)]
    return np.array([(ys[cy + 1] - ys[cy]) * (xs[cx + 1] - xs[cx]) for cy in range(4) for cx in range(4)])


# ---- ledger and plan
def test_shots_ledger_matches_the_library():
    """the sixth library's kernel set is exactly shot_sig_k, the cited GPU test exists, and no other library holds a kernel of the stage"""
    BUILD.build_lib(verbose=False)
    mine = kernel_ledger.symbols(BUILD.SHOTS_LIB)
    assert sorted(mine) == sorted(SHOTS_LEDGER), mine
    gpu = importlib.import_module("test_gpu_shots")
    for key, ref in SHOTS_LEDGER.items():
        path, name = ref.split("::")
        assert path == "tests/test_gpu_shots.py" and os.path.isfile(os.path.join(kernel_ledger.ROOT, path)) and callable(getattr(gpu, name, None)), (key, ref)
    for lib in (BUILD.LIB, BUILD.STAGES_LIB, BUILD.COMPOSE_LIB, BUILD.JPEG_LIB, BUILD.JPEG_IN_LIB):
        assert not [s for s in kernel_ledger.symbols(lib) if "shot" in s]
    assert len(kernel_ledger.symbols(BUILD.LIB)) == 85      # the main library's kernel set stays what tests/kernel_ledger.py pins


def _lib_plan(H, W):
    th, tw = C.c_int(), C.c_int()
    assert L.load().rrv_shot_plan(H, W, C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


def test_plan_equals_the_library_and_keeps_the_resampler_ratio():
    for size, thumb in PLANS.items():
        assert F.shot_plan(*size) == thumb == _lib_plan(*size)
    for size in ((8, 8), (513, 4), (4097, 16), (4, 4), (1, 1), (511, 513), (3840, 2160), (65535, 7), (7, 65535)):
        th, tw = F.shot_plan(*size)
        assert (th, tw) == _lib_plan(*size)
        assert th >= 1 and tw >= 1 and size[0] <= 8 * th and size[1] <= 8 * tw      # never above 8: the resampler's limit
    assert F.shot_plan(8, 8) == (8, 8) and F.shot_plan(513, 4) == (257, 2) and F.shot_plan(4097, 16) == (513, 2)
    lib = L.load()
    th, tw = C.c_int(), C.c_int()
    assert lib.rrv_shot_plan(0, 8, C.byref(th), C.byref(tw)) == -1 and lib.rrv_shot_plan(8, 8, None, C.byref(tw)) == -1
    with pytest.raises(ValueError):
        F.shot_plan(0, 8)
    assert F.Stylization.shot_detection is True


# ---- video.shot_signature on inputs with known answers
@pytest.mark.parametrize("H,W", [(4, 4), (5, 7), (37, 53)])
def test_every_cell_sums_to_its_pixel_count(H, W):
    frame = np.random.default_rng(H * W).uniform(-20, 280, (H, W, 3)).astype(np.float32)
    sig = V.shot_signature(frame)
    assert sig.shape == (16, 32) and sig.dtype == np.uint32
    np.testing.assert_array_equal(sig.sum(axis=1), cell_pixels(H, W))
    assert cell_pixels(H, W).sum() == H * W and cell_pixels(H, W).min() >= 1


def _bin(b8, g8, r8):
    return ((29 * b8 + 150 * g8 + 77 * r8 + 128) >> 8) >> 3


def test_ties_and_specials_round_as_stated():
    """0.5 -> 0, 1.5 -> 2, 254.5 -> 254, 255.5 -> 255, -3 -> 0, 300 -> 255, NaN -> 0, +inf -> 255, -inf -> 0.  A bin is 8 luma levels wide, so
    the value goes into the green channel of a pixel whose blue and red put the two candidate roundings into different bins."""
    for v, c8, other in ((0.5, 0, 1), (1.5, 2, 1), (254.5, 254, 255), (255.5, 255, 254), (-3.0, 0, 1), (300.0, 255, 254), (np.nan, 0, 1), (np.nan, 0, 255),
                         (np.inf, 255, 0), (np.inf, 255, 254), (-np.inf, 0, 255), (-np.inf, 0, 1), (-0.0, 0, 1)):
        b8, r8 = next((b, r) for b in range(256) for r in range(256) if _bin(b, c8, r) != _bin(b, other, r))
        frame = np.zeros((4, 4, 3), np.float32)
        frame[1, 2] = (b8, v, r8)      # cell 1 * 4 + 2
        sig = V.shot_signature(frame)
        assert sig[6, _bin(b8, c8, r8)] == 1 and sig[6].sum() == 1 and sig.sum() == 16 and sig[:, 0].sum() >= 15, (v, b8, r8)


def test_signature_equals_a_pixel_by_pixel_count():
    """the vectorised restatement against the definition, one pixel at a time in Python integers (round() is half to even)"""
    rng = np.random.default_rng(7)
    frame = rng.uniform(-20, 280, (9, 11, 3)).astype(np.float32)
    frame[rng.integers(0, 9, 12), rng.integers(0, 11, 12), rng.integers(0, 3, 12)] = [0.5, 1.5, 2.5, 254.5, 255.5, -3, 300, np.nan, np.inf, -np.inf, 7.5, 8.5]
    want = np.zeros((16, 32), np.uint32)
    for y in range(9):
        for x in range(11):
            c = [0 if not v > 0 else 255 if v >= 255 else round(float(v)) for v in frame[y, x]]
            want[(4 * y) // 9 * 4 + (4 * x) // 11, _bin(*c)] += 1
    np.testing.assert_array_equal(V.shot_signature(frame), want)


def test_primaries_land_in_their_bins():
    for bgr, b in (((255, 0, 0), 3), ((0, 255, 0), 18), ((0, 0, 255), 9), ((255, 255, 255), 31)):
        sig = V.shot_signature(np.full((8, 12, 3), bgr, np.uint8))
        np.testing.assert_array_equal(sig[:, b], cell_pixels(8, 12))
        assert sig.sum() == 96
    with pytest.raises(ValueError):
        V.shot_signature(np.zeros((3, 8, 3), np.float32))


# ---- the synthetic video
@pytest.mark.parametrize("H,W", SIZES)
def test_distances_and_cuts_of_the_synthetic_video(H, W):
    frames, sigs = video_and_signatures(H, W)
    assert len(frames) == 34
    Dn = V.shot_distances(sigs)
    assert Dn.dtype == np.float64 and Dn.shape == (34,) and Dn[0] == 0
    inside = [f for f in range(1, 34) if f not in CUTS]
    print("inside max %.4f, at the cuts %s" % (Dn[inside].max(), Dn[CUTS[1:]]))
    assert Dn[inside].max() < 0.06
    assert Dn[CUTS[1:]].min() >= 0.96
    np.testing.assert_array_equal(Dn, V.shot_distances(sigs, [(H, W)] * 34))
    # the formula, once by hand
    n = cell_pixels(H, W)
    by_hand = np.mean([np.abs(sigs[5, c].astype(np.int64) - sigs[4, c].astype(np.int64)).sum() / (2.0 * n[c]) for c in range(16)])
    assert Dn[5] == pytest.approx(by_hand, abs=1e-15)
    assert V.detect_cuts(Dn) == CUTS
    assert V.detect_cuts(Dn, min_len=10) == [0, 11, 33]
    assert V.detect_cuts(Dn, threshold=1.1) == [0]
    assert V.shots_from_cuts(CUTS, 34) == [(0, 11), (11, 20), (20, 33), (33, 34)]
    assert V.check_shots([(0, 11), (11, 34)], 34) == [(0, 11), (11, 34)]
    for bad in ([], [(1, 34)], [(0, 11), (12, 34)], [(0, 11), (11, 33)], [(0, 0), (0, 34)]):
        with pytest.raises(ValueError):
            V.check_shots(bad, 34)


def test_a_size_change_is_always_a_cut():
    a, b = synthetic_video(48, 64)[:6], synthetic_video(37, 53)[6:11]      # one shot, two sizes
    sigs = np.stack([V.shot_signature(f) for f in a + b])
    sizes = [f.shape[:2] for f in a + b]
    Dn = V.shot_distances(sigs, sizes)
    assert Dn[6] == 1.0 and V.shot_distances(sigs)[6] == 1.0 and Dn[[1, 2, 3, 4, 5, 7, 8, 9, 10]].max() < 0.06
    # equal pixel counts per cell, another shape: only `sizes` can tell
    t = np.stack([V.shot_signature(np.zeros((8, 16, 3))), V.shot_signature(np.zeros((16, 8, 3)))])
    assert V.shot_distances(t)[1] == 0.0 and V.shot_distances(t, [(8, 16), (16, 8)])[1] == 1.0
    assert V.size_changes(sizes) == [6]
    assert V.detect_cuts(Dn, forced=V.size_changes(sizes)) == [0, 6]
    assert V.detect_cuts(Dn, threshold=1.1, min_len=100, forced=V.size_changes(sizes)) == [0, 6]      # whatever the rule says


# ---- the shots file
def test_shots_file_round_trip_and_refusals(tmp_path):
    p = str(tmp_path / "shots.txt")
    V.write_shots(p, CUTS)
    assert V.read_shots(p, 34) == CUTS
    with open(p, "w") as f:
        f.write("# a comment\n0\n\n 11  # the second shot\n20\n")
    assert V.read_shots(p, 21) == [0, 11, 20]
    for text, word in (("0\n20\n11\n", "not sorted"), ("0\n11\n11\n", "twice"), ("0\n34\n", "out of range"), ("0\n-1\n", "not sorted"), ("-1\n0\n", "out of range"),
                       ("11\n20\n", "missing"), ("", "missing"), ("0\nabc\n", "not a frame index")):
        with open(p, "w") as f:
            f.write(text)
        with pytest.raises(ValueError, match=word):
            V.read_shots(p, 34)


# ---- the driver's control flow, with a model that records its calls
class _Recorder:
    """The call surface stylize_files / stylize_y4m use, recording (name, frame numbers): a frame carries its number in its first pixel (B, G)"""
    use_Global = True
    shot_detection = True
    yuv_input = True

    def __init__(self):
        self.calls = []

    @staticmethod
    def _number(f):
        f = np.asarray(f).reshape(-1)
        return int(f[0])

    def prepare_style(self, style):
        self.calls.append(("prepare_style",))

    def set_yuv_input_matrix(self, *a, **k):
        pass

    set_yuv_matrix = set_yuv_input_matrix

    def clean(self):
        self.calls.append(("clean",))

    def add(self, f, **kw):
        self.calls.append(("add", self._number(f)))

    def compute(self):
        self.calls.append(("compute",))

    def shot_signatures(self, frames, in_format="bgr", size=None):
        self.calls.append(("shot_signatures", len(frames)))
        if in_format == "bgr":
            return np.stack([V.shot_signature(f) for f in frames])
        H, W = size
        return np.stack([V.shot_signature(np.repeat(np.asarray(f)[:H * W].reshape(H, W, 1), 3, axis=2)) for f in frames])      # the luma plane

    def transfer_frames(self, frames, out=None, in_format="bgr", size=None, **kw):
        self.calls.append(("transfer_frames", [self._number(f) for f in frames]))
        if out is None:
            out = np.zeros(np.asarray(frames).shape, np.float32)
        out[...] = 0
        return out


def _numbered_pngs(tmp_path, frames):
    src = tmp_path / "in"
    src.mkdir()
    for i, f in enumerate(frames):
        f = f.copy()
        f[0, 0, 0] = i      # blue of the first pixel: the frame's number (PNG is lossless)
        D.write_image_bgr(str(src / ("f%03d.png" % i)), f)
    D.write_image_bgr(str(tmp_path / "style.png"), np.zeros((16, 16, 3), np.uint8))
    return D.list_frames(str(src / "*.png"))


def _expected(shots, chunk):
    calls = [("prepare_style",)]
    for lo, hi in shots:
        calls += [("clean",)] + [("add", lo + i) for i in V.sample_indices(hi - lo)] + [("compute",)]
        calls += [("transfer_frames", list(range(c0, min(c0 + chunk, hi)))) for c0 in range(lo, hi, chunk)]
    return calls


def test_driver_runs_one_preparation_per_shot_and_no_chunk_straddles(tmp_path):
    frames, _ = video_and_signatures(37, 53)
    paths = _numbered_pngs(tmp_path, frames)
    kw = dict(chunk=4, io_threads=2, log=lambda *_: None)
    shots = [(0, 11), (11, 20), (20, 33), (33, 34)]
    m = _Recorder()
    D.stylize_files(m, str(tmp_path / "style.png"), paths, str(tmp_path / "o1"), shots=shots, **kw)
    assert m.calls == _expected(shots, 4)
    assert [c[1] for c in m.calls if c[0] == "add"] == [0, 10, 11, 19, 20, 32, 33]      # lo + sample_indices(hi - lo), spelled out
    # without shots: today's sequence, call for call
    m = _Recorder()
    D.stylize_files(m, str(tmp_path / "style.png"), paths, str(tmp_path / "o2"), **kw)
    assert m.calls == _expected([(0, 34)], 4)
    # one shot that is the whole video: the same calls as none
    m = _Recorder()
    D.stylize_files(m, str(tmp_path / "style.png"), paths, str(tmp_path / "o3"), shots=[(0, 34)], **kw)
    assert m.calls == _expected([(0, 34)], 4)
    # "auto": the detection pass first (every frame, in chunks), then the shots it found
    m = _Recorder()
    stats = {}
    D.stylize_files(m, str(tmp_path / "style.png"), paths, str(tmp_path / "o4"), shots="auto", write_shots=str(tmp_path / "w.txt"), stats=stats, **kw)
    assert m.calls[:9] == [("shot_signatures", 4)] * 8 + [("shot_signatures", 2)]
    assert m.calls[9:] == _expected(shots, 4) and stats["shots"] == 4
    assert V.read_shots(str(tmp_path / "w.txt"), 34) == CUTS
    # the refusals, in words
    with pytest.raises(ValueError, match="one rank"):
        D.stylize_files(_Recorder(), str(tmp_path / "style.png"), paths, str(tmp_path / "o5"), shots=shots, world=2, rank=0, **kw)
    fm = _Recorder()
    fm.use_Global = False
    with pytest.raises(ValueError, match="frame mode"):
        D.stylize_files(fm, str(tmp_path / "style.png"), paths, str(tmp_path / "o5"), shots=shots, **kw)
    with pytest.raises(ValueError, match="tile"):
        D.stylize_files(_Recorder(), str(tmp_path / "style.png"), paths, str(tmp_path / "o5"), shots=[(0, 11), (12, 34)], **kw)
    assert not fm.calls


def test_command_line_shots_file_round_trip_and_refusals(tmp_path, capsys):
    frames, _ = video_and_signatures(37, 53)
    _numbered_pngs(tmp_path, frames)
    made = []

    def factory(args, device):
        made.append(_Recorder())
        return made[-1]
    base = ["--style", str(tmp_path / "style.png"), "--frames", str(tmp_path / "in" / "*.png"), "--checkpoint", "synthetic", "--io-threads", "2", "--chunk", "5"]
    w = str(tmp_path / "cuts.txt")
    assert D.main(base + ["--out", str(tmp_path / "a"), "--shots", "auto", "--write-shots", w], model_factory=factory) == 0
    assert V.read_shots(w, 34) == CUTS
    assert D.main(base + ["--out", str(tmp_path / "b"), "--shots", w], model_factory=factory) == 0
    auto, from_file = made[0].calls, made[1].calls
    assert [c for c in auto if c[0] != "shot_signatures"] == from_file == _expected(V.shots_from_cuts(CUTS, 34), 5)
    assert D.main(base + ["--out", str(tmp_path / "c"), "--shots", "auto", "--shot-min-len", "10"], model_factory=factory) == 0
    assert [c for c in made[2].calls if c[0] != "shot_signatures"] == _expected([(0, 11), (11, 33), (33, 34)], 5)
    assert D.main(base + ["--out", str(tmp_path / "d"), "--shots", "auto", "--shot-threshold", "1.1"], model_factory=factory) == 0
    assert [c for c in made[3].calls if c[0] != "shot_signatures"] == _expected([(0, 34)], 5)
    capsys.readouterr()
    n = len(made)
    for extra, word in ((["--gpus", "2"], "one GPU"), (["--style", str(tmp_path / "style.png"), str(tmp_path / "style.png")], "single-style"), (["--no-global"], "frame mode"),
                        (["--shots", str(tmp_path / "nowhere.txt")], "no such file")):
        with pytest.raises(SystemExit) as e:
            D.main(base + ["--out", str(tmp_path / "e"), "--shots", "auto"] + extra, model_factory=factory)
        assert e.value.code == 2 and word in capsys.readouterr().err, word
    for extra in (["--shots", w, "--shot-min-len", "10"], ["--shot-threshold", "0.5"]):      # the rule's knobs without the detector
        with pytest.raises(SystemExit):
            D.main(base + ["--out", str(tmp_path / "e")] + extra, model_factory=factory)
        assert "belong to --shots auto" in capsys.readouterr().err
    with open(str(tmp_path / "bad.txt"), "w") as f:
        f.write("0\n20\n11\n")
    with pytest.raises(SystemExit):
        D.main(base + ["--out", str(tmp_path / "e"), "--shots", str(tmp_path / "bad.txt")], model_factory=factory)
    assert "not sorted" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        D.main(base + ["--out", str(tmp_path / "e"), "--write-shots", w], model_factory=factory)
    assert "--write-shots needs --shots" in capsys.readouterr().err
    assert len(made) == n      # refused before a model exists


def test_y4m_chunks_start_over_at_every_shot(tmp_path):
    H, W, n = 8, 16, 21
    w = D.Y4MWriter(str(tmp_path / "in.y4m"), 24, W, H)
    for i in range(n):
        fr = np.full(H * W * 3 // 2, 33 if i < 9 else 220, np.uint8)      # (+ 0..2 below: inside one bin)
        fr[0] = i      # the first luma sample: the frame's number
        fr[1:H * W] += np.uint8(i % 3)
        w.append(fr, (H, W))
    w.release()
    D.write_image_bgr(str(tmp_path / "style.png"), np.zeros((16, 16, 3), np.uint8))
    kw = dict(video_path=str(tmp_path / "out.y4m"), write_frames=False, chunk=4, io_threads=2, log=lambda *_: None)
    m = _Recorder()
    m.transfer_frames = lambda frames, out=None, **k: (m.calls.append(("transfer_frames", [int(f[0]) for f in frames])), out.__setitem__(Ellipsis, 0), out)[2]
    D.stylize_y4m(m, str(tmp_path / "style.png"), str(tmp_path / "in.y4m"), str(tmp_path / "o"), shots=[(0, 9), (9, 21)], **kw)
    assert m.calls == _expected([(0, 9), (9, 21)], 4)
    m.calls.clear()
    D.stylize_y4m(m, str(tmp_path / "style.png"), str(tmp_path / "in.y4m"), str(tmp_path / "o"), **kw)
    assert m.calls == _expected([(0, 21)], 4)
    m.calls.clear()
    D.stylize_y4m(m, str(tmp_path / "style.png"), str(tmp_path / "in.y4m"), str(tmp_path / "o"), shots="auto", write_shots=str(tmp_path / "w.txt"), **kw)
    assert m.calls[:6] == [("shot_signatures", 4)] * 5 + [("shot_signatures", 1)]
    assert m.calls[6:] == _expected([(0, 9), (9, 21)], 4) and V.read_shots(str(tmp_path / "w.txt"), n) == [0, 9]
    m.use_Global = False
    with pytest.raises(ValueError, match="frame mode"):
        D.stylize_y4m(m, str(tmp_path / "style.png"), str(tmp_path / "in.y4m"), str(tmp_path / "o"), shots="auto", **kw)

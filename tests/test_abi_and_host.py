"""CPU-side checks: the C-ABI library loads and exports every symbol the header declares
(no compute calls without a GPU), host-side driver logic, weight table."""
import os
import re
import importlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "rerevst_hip.h")).read()
    return sorted(set(re.findall(r"\b(rrv_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    b = importlib.import_module("rerevst-code_amd.build")
    b.build_lib(verbose=False)
    L = importlib.import_module("rerevst-code_amd._lib")
    lib = L.load()
    names = _declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "librerevst_hip.so lacks %s" % n
        assert n in L.SYMBOLS, "ctypes table lacks %s" % n
    assert sorted(L.SYMBOLS) == names


def test_state_layout_constants_agree(oracle):
    L = importlib.import_module("rerevst-code_amd._lib")
    D = importlib.import_module("rerevst-code_amd.dist")
    hdr = open(os.path.join(ROOT, "include", "rerevst_hip.h")).read()
    n = int(re.search(r"#define RRV_STATE_FLOATS (\d+)", hdr).group(1))
    assert n == L.STATE_FLOATS == D.STATE_FLOATS == oracle.STATE_FLOATS == 17536


def test_weight_table_and_generator(pkg):
    t = pkg.weight_table()
    # 107 reference keys minus the 18 Vgg19.* keys the reference deletes itself; Encoder 3.5M + EncoderStyle 3.5M + Decoder 4.66M
    assert len(t) == 89 and sum(int(np.prod(s)) for s in t.values()) == 11_679_203
    w1, w2 = pkg.synthetic_weights(0), pkg.synthetic_weights(0)
    for k, shape in t.items():
        assert w1[k].shape == tuple(shape) and w1[k].dtype == np.float32
        np.testing.assert_array_equal(w1[k], w2[k])
    assert not np.array_equal(pkg.synthetic_weights(1)["Decoder.slice1.weight"], w1["Decoder.slice1.weight"])


def test_video_helpers_match_oracle_restatement(oracle):
    V = importlib.import_module("rerevst-code_amd.video")
    for n in (1, 2, 8, 9, 17, 100, 300, 1200):
        assert V.sample_indices(n) == oracle.sample_indices(n)
    assert len(V.sample_indices(300)) == 38 and len(V.sample_indices(1200)) == 150
    for n in (48, 64, 256, 436, 512, 1024):
        assert V.padded_size(n) == oracle.padded_size(n)
    img = np.random.default_rng(0).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    tool = V.ReshapeTool()
    p = tool.process(img)
    assert p.shape == (192, 256, 3) and (p == oracle.reflect_pad(img, 192, 256)).all()
    assert (p[64:114, 64:134] == img).all()
    # shards tile the frame range exactly
    for n, w in ((300, 8), (1200, 8), (7, 2), (5, 4)):
        spans = [V.shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))


def test_stylization_without_gpu_fails_loudly(pkg, weights):
    """No CPU fallback: constructing the HIP Stylization on a box without a GPU raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg.RRVError):
        pkg.Stylization(weights, cuda=True)
    with pytest.raises(pkg.RRVError):
        pkg.Stylization(weights, cuda=False)


def test_bench_kernel_name_mapping_and_traffic_lookup():
    """bench.py labels -> rocprofv3 kernel names (used to attach the measured HBM traffic to the roofline)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.rocprof_name("conv_wino<E_LRELU | E_NORM1 | E_RES_UPS | E_NORM2>") == "void conv_wino_split_k<54, 0>(ConvP)"
    assert b.rocprof_name("conv_wino<E_RELU | E_POOL>") == "void conv_wino_split_k<65, 0>(ConvP)"
    assert b.rocprof_name("conv_upw<E_LRELU>") == "void conv_wino_k<2, 0, 4, 1, 0, 0>(ConvP)"
    assert b.rocprof_name("conv_upw_sc<E_LRELU | E_NORM1>") == "void conv_wino_k<6, 0, 4, 1, 1, 0>(ConvP)"
    assert b.rocprof_name("conv_mfma<128,1,0>") == "void conv_mfma_k<128, 1, 0, 0, 0, 1>(ConvP)"
    for size, ms in ((512, 0), (256, 0), (1024, 0), (1024, 4)):        # every configuration has a committed counter pass: never null
        t = b.measured_traffic("conv_upw_sc<E_LRELU | E_NORM1>", size, ms)
        assert t is not None and t > 1e8, (size, ms, t)
    assert b.measured_traffic("conv_wino<E_RELU>") > 1e6
    assert b.measured_traffic("no_such_kernel<1>") is None


def test_bench_dump_sample_is_seeded_and_bounded():
    """bench.py --dump-outputs: an output within the budget is dumped whole; a larger one as whole frames, or as single
    elements when one frame is over the budget — the same indices every run, and never more bytes than the budget."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    a = np.random.default_rng(3).random((10, 8, 8, 3), dtype=np.float32)
    s, idx = b.dump_sample(a, a.nbytes)
    assert idx is None and np.array_equal(s, a) and s.dtype == np.float32
    s, idx = b.dump_sample(a, 3 * a[0].nbytes + 5)
    assert s.shape == (3, 8, 8, 3) and list(idx) == sorted(set(idx)) and np.array_equal(s, a[idx])
    s2, idx2 = b.dump_sample(a, 3 * a[0].nbytes + 5)
    assert np.array_equal(idx, idx2) and np.array_equal(s, s2)
    s, idx = b.dump_sample(a, 100)
    assert s.shape == (25,) and s.nbytes <= 100 and np.array_equal(s, a.reshape(-1)[idx])
    assert b.DUMP_BYTES + 16 * 128 <= 64 * 1000 * 1000


def test_checkpoint_pth_branch_strict_load(tmp_path, pkg):
    """The reference loads its 107-key .pth with a strict load_state_dict (test/framework.py:74-75).  Write the seeded
    weights as a torch.save'd state_dict WITH the Vgg19.* keys the reference's checkpoint also carries, read it back
    through the product's .pth branch; a missing key or a wrong shape must raise."""
    import torch
    W = importlib.import_module("rerevst-code_amd.weights")
    w = pkg.synthetic_weights(0)
    sd = {k: torch.from_numpy(v.copy()) for k, v in w.items()}
    for i, (idx, cin, cout) in enumerate(W.VGG_CONVS):                    # the unused perceptual-loss VGG (deleted by the reference itself)
        sd["Vgg19.slice.%d.weight" % idx] = torch.zeros(cout, cin, 3, 3)
        sd["Vgg19.slice.%d.bias" % idx] = torch.zeros(cout)
    assert len(sd) == 107
    path = str(tmp_path / "style_net-TIP-final.pth")
    torch.save(sd, path)
    got = W.load_checkpoint(path)
    assert sorted(got) == sorted(w)
    for k in w:
        assert got[k].dtype == np.float32 and got[k].flags.c_contiguous
        np.testing.assert_array_equal(got[k], w[k])
    bad = dict(sd)
    del bad["Decoder.Filter2.F1.FC.bias"]
    torch.save(bad, path)
    with pytest.raises(KeyError, match="Decoder.Filter2.F1.FC.bias"):
        W.load_checkpoint(path)
    bad = dict(sd)
    bad["Decoder.slice1.weight"] = torch.zeros(3, 64, 1, 1)
    torch.save(bad, path)
    with pytest.raises(ValueError, match="Decoder.slice1.weight"):
        W.load_checkpoint(path)
    # half-precision / double checkpoints are converted to fp32
    torch.save({k: v.double() for k, v in sd.items()}, path)
    assert W.load_checkpoint(path)["Decoder.slice1.bias"].dtype == np.float32


def test_multistyle_driver_helpers(oracle):
    V = importlib.import_module("rerevst-code_amd.video")
    for n in (2, 16, 17, 33, 300):
        assert V.sample_indices_multistyle(n) == oracle.sample_indices_multistyle(n)
    assert V.sample_indices_multistyle(33) == [0, 16, 32, 32]          # the last frame AGAIN ("Multi-style Interpolation/test.py":72-85)
    assert len(V.sample_indices_multistyle(300)) == 20
    # two styles: exactly the reference ramp [i/(n-1), 1 - i/(n-1)] (test.py:127-131)
    for i in (0, 1, 150, 299):
        w = V.ramp_weights(i, 300, 2)
        assert w == [i / 299.0, 1 - i / 299.0]
    for S in (3, 4):
        assert V.ramp_weights(0, 300, S) == [0.0] * (S - 1) + [1.0]    # starts on the last style ...
        assert V.ramp_weights(299, 300, S) == [1.0] + [0.0] * (S - 1)   # ... ends on style 0
        for i in range(0, 300, 7):
            w = V.ramp_weights(i, 300, S)
            assert abs(sum(w) - 1) < 1e-12 and min(w) >= 0 and sum(1 for v in w if v > 0) <= 2
    img = np.random.default_rng(1).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    r = V.resize_bilinear(img, (384, 384))
    assert r.shape == (384, 384, 3) and r.dtype == np.uint8
    np.testing.assert_array_equal(V.resize_bilinear(img, (70, 50)), img)       # identity geometry
    flat = np.full((9, 9, 3), 77, np.uint8)
    assert (V.resize_bilinear(flat, (384, 384)) == 77).all()


def test_multistyle_driver_flow_with_oracle_model(oracle, pkg, weights):
    """video.stylize_video_multistyle (the product's restatement of "Multi-style Interpolation/test.py":40-131) driven
    with the oracle as the model: padding before encoding, every 16th + last feature sampled, per-frame ramp, crop."""
    V = importlib.import_module("rerevst-code_amd.video")
    frames = [pkg.synth_frame(i, 24, 32, kind="smooth") for i in range(3)]
    styles = [pkg.synth_style(20, 28, kind="smooth", seed=5), pkg.synth_style(28, 20, kind="smooth", seed=6)]
    m = oracle.MultiStylization(weights, 2)
    out = V.stylize_video_multistyle(m, frames, styles, style_size=(32, 32))
    assert sorted(out) == [0, 1, 2] and all(v.shape == (24, 32, 3) and v.dtype == np.float32 for v in out.values())
    # the same by hand
    o = oracle.MultiStylization(weights, 2)
    o.prepare_style([V.resize_bilinear(s, (32, 32)) for s in styles])
    feats = [o.generate_content_features(oracle.reflect_pad(f, 192, 192)) for f in frames]
    o.clean()
    for i in (0, 2):                    # sample_indices_multistyle(3) = [0] + [last]
        o.add_patch(feats[i])
    o.compute_norm()
    for i in range(3):
        ref = o.transfer(feats[i], [i / 2.0, 1 - i / 2.0])[64:88, 64:96]
        np.testing.assert_allclose(out[i], ref, atol=1e-3)


def test_oracle_torch_conv_backend_agrees(oracle):
    """bench.py times the oracle with its 3x3 convolutions on torch's CPU conv2d (the reference's primitive); same result."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 21, 17, 32), dtype=np.float32)
    w = (rng.standard_normal((48, 32, 3, 3), dtype=np.float32) * 0.05).astype(np.float32)
    b = rng.standard_normal(48).astype(np.float32)
    a = oracle.conv3x3(x, w, b)
    oracle.set_conv_backend("torch")
    try:
        c = oracle.conv3x3(x, w, b)
        c0 = oracle.conv3x3(x, w)
    finally:
        oracle.set_conv_backend("numpy")
    assert c.shape == a.shape and c.dtype == np.float32
    np.testing.assert_allclose(c, a, atol=2e-5)
    np.testing.assert_allclose(c0 + b, a, atol=2e-5)


def test_bench_roofline_fields_from_event_rows():
    """bench.py's roofline object: `achieved` / `frac` are the EXECUTED FLOPs of the dominant kernel over its HIP-event
    time (never above 1), the reference's direct-form FLOPs are reported next to them; HBM-bound kernels carry a
    fraction of the HBM peak instead."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    rows = []
    for _ in range(8):        # (name, ms, algorithmic flops, algorithmic bytes, executed flops)
        rows.append(("conv_upw_sc<E_LRELU | E_NORM1>@128x64@640x640", 1.0, 4.0e11, 8.0e8, 1.2e11))
        rows.append(("conv_wino<E_RELU>@256x256@160x160", 0.5, 1.0e11, 3.0e8, 4.4e10))
        rows.append(("conv_last", 0.25, 1.0e10, 8.0e8, 1.0e10))
    roof, kern, layers = b.roofline_and_kernels(rows, 1, 64, 512)
    assert roof["kernel"] == "conv_upw_sc<E_LRELU | E_NORM1>" and roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s"
    assert abs(roof["achieved"] - 120.0) < 1e-6 and abs(roof["frac"] - 120.0 / 157.3) < 1e-3 and roof["frac"] < 1.0
    assert abs(roof["algorithmic_tflops"] - 400.0) < 1e-6 and abs(roof["algorithmic_speedup"] - 4.0 / 1.2) < 1e-2
    assert roof["algorithmic_bytes_per_launch"] == 800000000 and abs(roof["avg_launch_ms"] - 1.0) < 1e-9
    k = {r["kernel"]: r for r in kern}
    assert k["conv_last"]["bound"] == "hbm" and abs(k["conv_last"]["frac_of_hbm_peak"] - 3200.0 / 8000.0) < 1e-3
    assert k["conv_wino<E_RELU>"]["bound"] == "mfma" and abs(k["conv_wino<E_RELU>"]["frac_of_mfma_peak"] - 88.0 / 157.3) < 1e-3
    assert abs(k["conv_last"]["ms_per_frame"] - 8 * 0.25 / 64) < 1e-4
    assert b.roofline_and_kernels([], 0, 64, 512)[0] is None


def test_tools_hold_no_copies_of_the_library_kernels():
    """microbenchmarks are built from the library headers (ablation hooks behind WSPLIT_ABL / F43_ABL, empty
    in the product build), never from hand-kept copies of a kernel that drift from it."""
    tools = os.path.join(ROOT, "tools")
    lib_kernels = set()
    for f in os.listdir(os.path.join(ROOT, "rerevst-code_amd", "csrc")):
        lib_kernels |= set(re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", open(os.path.join(ROOT, "rerevst-code_amd", "csrc", f)).read()))
    assert {"conv_wino_split_k", "conv_f43_k", "conv_wino_k"} <= lib_kernels
    for f in os.listdir(tools):
        if not f.endswith((".h", ".hip")):
            continue
        src = open(os.path.join(tools, f)).read()
        defined = set(re.findall(r"__global__.*?\bvoid\s+(\w+)\s*\(", src))
        assert not (defined & lib_kernels), "%s defines its own %s" % (f, sorted(defined & lib_kernels))
        assert not re.search(r"conv_wino\w*_ab", src), "%s refers to a kernel copy" % f
    # the hooks are compiled out of the product: the library build defines neither macro
    b = importlib.import_module("rerevst-code_amd.build")
    import inspect
    assert "WSPLIT_ABL" not in inspect.getsource(b) and "F43_ABL" not in inspect.getsource(b)


@pytest.mark.parametrize("cfg", ["256", "512", "1024", "ms4"])
def test_pmc_read_traffic_is_not_below_the_compulsory_input(cfg):
    """profiles/hbm_traffic_<cfg>.json turns rocprofv3's FETCH_SIZE into bytes with a per-kernel factor F (the counter tallies
    64 B per L2 request whatever its width: tools/pmc_traffic_json.py, profiles/r05_fetch_calib.txt, r06_fetch_calib.txt).  A wrong factor shows up
    as a kernel that "reads" less than it must (round 4: conv_f43_k at F = 0.5 reported half its input).  For every kernel whose
    compulsory read per launch is far beyond what the caches can hold (>= 256 MB: 32 MB of L2, and the producer's output of
    the previous launch cannot all sit in the memory-side cache) the read bytes must reach 0.8 x that compulsory read = the
    algorithmic bytes of the same configuration's bench line (profiles/r06_bench_<cfg>.json: input + output + residual +
    weights, each once) minus the bytes it measurably wrote.  (Measured: 0.83 - 1.56; the 128-byte residual rows of
    conv_f43_k<54> and what still sits in the caches account for the values below 1.)"""
    import json
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    with open(os.path.join(root, "profiles", "hbm_traffic_%s.json" % cfg)) as f:
        traffic = json.load(f)["kernels"]
    with open(os.path.join(root, "profiles", "r06_bench_%s.json" % cfg)) as f:
        line = json.loads(f.read().strip().splitlines()[-1])
    checked = 0
    for row in line["kernels"]:
        alg = row.get("algorithmic_bytes_per_launch")
        if not alg:
            continue
        name = bench.rocprof_name(row["kernel"])
        ent = next((v for k, v in traffic.items() if k == name or k.startswith(name + "(") or k == name.replace(", 0>(ConvP)", ", 1>(ConvP)")), None)
        if ent is None:
            continue
        compulsory = alg - ent["write_bytes"]
        if compulsory < (256 << 20):
            continue
        assert ent["read_bytes"] >= 0.8 * compulsory, "%s: %d read bytes per launch (F = %s) against %d compulsory" % (row["kernel"], ent["read_bytes"], ent["fetch_factor"], compulsory)
        checked += 1
    assert checked >= (1 if cfg == "ms4" else 4)

#!/usr/bin/env python
"""What scaling costs: the resample kernel next to the first kernel and the whole launch sequence, and the host -> host rate of a scaled
call.  Writes one JSON object (with --out: to that file, e.g. profiles/resample.json).  Needs an MI355X; a leg that did not run is
recorded as "not measured", never estimated.

  kernel legs  16 frames per call through transfer_tensor(work_size=, pad_crop=True), 3840 x 2160 -> 1920 x 1080 and 1920 x 1080 ->
               960 x 540, NV12 and uint8 BGR input.  Each leg runs in a process of its own under `rocprofv3 --kernel-trace --stats`; its
               kernel trace is cut into calls at every dispatch of resample_k, the first (warm-up) call is dropped, and the medians over
               the others are recorded: the resample kernel, conv_first_k, and the sum of all kernels of the call, in ms per 16 frames.
               Algorithmic bytes come from the shapes (source samples read once, 12 bytes per working pixel written), algorithmic
               operations from the tap tables (two per tap, channel and pass); the share of peak is the larger of bytes / 8 TB/s and
               operations / 157.3 TFLOP/s over the kernel time, and the larger one names the bound.
  host legs    transfer_frames over 300 uint8 BGR frames per call, page-locked buffers, profiler off, three repeats after a warm-up call,
               each leg in a process of its own: 1920 x 1080 frames with work_size=(540, 960) on this tree's library; 960 x 540 frames,
               not scaled, on this tree's library and -- with --parent-lib -- on a library built from the parent commit, the two taking
               turns.  The plain path is held to the parent's: its median may fall below the parent's by the parent's own max - min.
    python tools/resample_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/resample.json] [--skip-kernel-legs]
Every leg is a process in a session of its own.  The first leg that exits non-zero or runs past --leg-timeout ends the measurement: its
whole process group is killed, nothing more is started on the GPU, what was measured so far is written with "not measured" for the rest,
and the tool exits non-zero.
`--leg NAME` runs one leg (what the child processes do; RRV_LIB_PATH names the library).  FORM_CASES adds a 1920 x 1080 -> 960 x 540
`trace:` leg for each input form the measured cases do not read (uint8 planar, float32 HWC and planar, I420, ten-bit planar and P010):
not part of the JSON, they let a comparison of two builds time every resample_k<IN> (profiles/stages.txt)."""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_CASES = {"2160_nv12": ((2160, 3840), (1080, 1920), "nv12"), "2160_bgr": ((2160, 3840), (1080, 1920), "bgr"),
                "1080_nv12": ((1080, 1920), (540, 960), "nv12"), "1080_bgr": ((1080, 1920), (540, 960), "bgr")}
# one leg for each input form the four above do not read (every resample_k<IN> then has one); main() measures the four, `--leg trace:<case>` any
FORM_CASES = {"1080_" + f: ((1080, 1920), (540, 960), f) for f in ("u8_chw", "f32", "f32_chw", "i420", "i420p10", "p010")}
KERNEL_CASES.update(FORM_CASES)
MEASURED = [c for c in KERNEL_CASES if c not in FORM_CASES]
SOURCE_BYTES = {"bgr": 3.0, "u8_chw": 3.0, "f32": 12.0, "f32_chw": 12.0, "nv12": 1.5, "i420": 1.5, "i420p10": 3.0, "p010": 3.0}      # per source pixel
FRAMES_PER_CALL = 16
PEAK_BYTES_S, PEAK_FP32_S = 8.0e12, 157.3e12


def _stat(v, digits):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits), "runs": [round(x, digits) for x in v]}


def _load_pkg():
    """the package on the library RRV_LIB_PATH names; a library built from the parent commit has no scaled entries, so they leave the
    symbol table before it is loaded"""
    sys.path.insert(0, HERE)
    L = importlib.import_module("rerevst-code_amd._lib")
    if os.environ.get("RRV_LIB_PATH"):
        import ctypes
        L._share_torch_hip_runtime()      # as L.load() does first: both libraries' legs then run on the same HIP runtime
        lib = ctypes.CDLL(L.LIB_PATH)
        for name in [n for n in L.SYMBOLS if not hasattr(lib, n)]:
            del L.SYMBOLS[name]
    return importlib.import_module("rerevst-code_amd")


def _model(pkg, H, W):
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    m.prepare_style(pkg.synth_style(512, 512, kind="noise", seed=7))
    m.clean()
    for i in (0, 8, 16):
        m.add(pkg.synth_frame(i, H, W, kind="noise"))
    m.compute()
    return m


def _source(fmt, n, H, W, seed=3):
    """n random source frames: uint8 BGR [n][H][W][3] ("f32": float32; "_chw": planar [n][3][H][W]), or 4:2:0 samples [n][H*W*3/2] (even
    H, W): bytes, or ten-bit codes as int16 (the bits of uint16; "p010" keeps them in the high bits)"""
    rng = np.random.default_rng(seed)
    if fmt in ("i420p10", "p010"):
        base = (rng.integers(0, 1024, (4, H * W * 3 // 2), dtype=np.uint16) << (6 if fmt == "p010" else 0)).view(np.int16)
    elif fmt in ("nv12", "i420"):
        base = rng.integers(0, 256, (4, H * W * 3 // 2), dtype=np.uint8)
    else:
        base = rng.integers(0, 256, (4, 3, H, W) if fmt.endswith("_chw") else (4, H, W, 3), dtype=np.uint8).astype(np.float32 if fmt.startswith("f32") else np.uint8)
    return base[np.arange(n) % 4]


def leg_trace(pkg, case, repeats):
    """the work a profiler run traces: preparation at the working size, then 1 + repeats identical scaled calls of 16 frames"""
    import torch
    (SH, SW), (H, W), fmt = KERNEL_CASES[case]
    m = _model(pkg, H, W)
    x = torch.from_numpy(_source(fmt, FRAMES_PER_CALL, SH, SW)).cuda()
    kw = dict(layout="nchw" if fmt.endswith("_chw") else "nhwc") if fmt in ("bgr", "u8_chw", "f32", "f32_chw") else dict(layout=fmt, size=(SH, SW))
    torch.cuda.synchronize()
    for _ in range(repeats + 1):
        m.transfer_tensor(x, pad_crop=True, out_layout="nhwc", work_size=(H, W), **kw)
        m.sync()
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "calls": repeats + 1}


def algorithmic(case):
    """bytes and float operations of one resample launch of 16 frames, from the shapes and the tap tables"""
    (SH, SW), (H, W), fmt = KERNEL_CASES[case]
    sys.path.insert(0, HERE)
    taps = importlib.import_module("rerevst-code_amd.framework").resample_taps
    ny, nx = taps(SH, H)[1].astype(np.int64), taps(SW, W)[1].astype(np.int64)
    bytes_ = (SOURCE_BYTES[fmt] * SH * SW + 12.0 * H * W) * FRAMES_PER_CALL
    ops = 2.0 * 3 * (float(nx.sum()) * SH + float(ny.sum()) * W) * FRAMES_PER_CALL      # horizontal pass over the source rows, vertical over the columns
    return bytes_, ops


def parse_trace(path):
    """per-call kernel times (ms) of a rocprofv3 kernel trace: calls start at each resample_k dispatch, the first one is the warm-up"""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    starts = [i for i, r in enumerate(rows) if "resample_k" in r[0]]
    if len(starts) < 2:
        raise ValueError("%s holds %d resample_k dispatches: nothing to cut calls at" % (path, len(starts)))
    calls = []
    for a, b in zip(starts[1:], starts[2:] + [len(rows)]):
        seg = rows[a:b]
        ms = lambda pred: sum(e - s for n, s, e in seg if pred(n)) / 1e6
        calls.append((ms(lambda n: "resample_k" in n), ms(lambda n: "conv_first_k" in n), ms(lambda n: True), len(seg)))
    return calls


def _run(cmd, env, timeout, stdout):
    """One leg's process, in a session of its own.  A time limit kills the whole group (under rocprofv3 the program that has the GPU open is
    a grandchild) and raises, as a non-zero exit status does: the caller then starts nothing more on the GPU."""
    p = subprocess.Popen(cmd, stdout=stdout, env=env, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=timeout)
    except BaseException:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.wait()
        raise
    if p.returncode != 0:
        raise subprocess.CalledProcessError(p.returncode, cmd)
    return out


def kernel_leg(case, a):
    out_dir = tempfile.mkdtemp(prefix="resample_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", case, "--",
           sys.executable, os.path.abspath(__file__), "--leg", "trace:" + case, "--repeats", str(a.kernel_repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    print("kernel leg %s under rocprofv3" % case, file=sys.stderr, flush=True)
    try:
        _run(cmd, env, a.leg_timeout, subprocess.DEVNULL)
        traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise ValueError("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
        calls = parse_trace(traces[0])
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    (SH, SW), (H, W), fmt = KERNEL_CASES[case]
    bytes_, ops = algorithmic(case)
    rs = _stat([c[0] for c in calls], 4)
    t = rs["median"] * 1e-3
    t_bytes, t_ops = bytes_ / PEAK_BYTES_S, ops / PEAK_FP32_S
    return {"source": [SH, SW], "work_size": [H, W], "input": fmt, "frames_per_call": FRAMES_PER_CALL, "calls": len(calls),
            "kernels_per_call": calls[0][3], "resample_k_ms": rs, "conv_first_k_ms": _stat([c[1] for c in calls], 4),
            "all_kernels_ms": _stat([c[2] for c in calls], 3), "algorithmic_bytes": int(bytes_), "algorithmic_flop": int(ops),
            "achieved_TB_s": round(bytes_ / t / 1e12, 3), "bound": "HBM bandwidth" if t_bytes >= t_ops else "fp32 vector rate",
            "share_of_peak": round(max(t_bytes, t_ops) / t, 4)}


def leg_host(pkg, scaled, n, repeats):
    """frames/s host -> host of transfer_frames over n uint8 BGR frames: 1080p with work_size=(540, 960), or 540p as they are"""
    (SH, SW), work = ((1080, 1920), (540, 960)) if scaled else ((540, 960), None)
    m = _model(pkg, 540, 960)
    src = pkg.pinned_empty((n, SH, SW, 3), np.uint8)
    src[...] = _source("bgr", n, SH, SW)
    out = pkg.pinned_empty((n, 540, 960, 3), np.float32)
    kw = {"work_size": work} if scaled else {}
    rates = []
    for k in range(repeats + 1):            # call 0 warms up (workspaces, staging)
        t0 = time.perf_counter()
        m.transfer_frames(src, out=out, **kw)
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    return dict(_stat(rates, 1), unit="frames/s host -> host", frames_per_call=n, source=[SH, SW], delivered=[540, 960], scaled=scaled)


def _child(lib, leg, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(a.frames), "--repeats", str(a.repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    if lib:
        env["RRV_LIB_PATH"] = os.path.abspath(lib)
    print("leg %s on %s" % (leg, lib or "this tree's library"), file=sys.stderr, flush=True)
    return json.loads(_run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().strip().splitlines()[-1])


def measure(a, res):
    """Every leg in order, each in a process of its own; the first one that fails ends the measurement (the exception leaves here)."""
    if not a.skip_kernel_legs:
        if shutil.which("rocprofv3") is None:
            for case in MEASURED:
                res["kernel_" + case] = "not measured (rocprofv3 not found)"
        else:
            for case in MEASURED:
                res["kernel_" + case] = kernel_leg(case, a)
    if a.skip_host_legs:
        return
    plain, parent = [], []
    for turn in range(2):                    # the two libraries take turns
        if a.parent_lib:
            parent.append(_child(a.parent_lib, "host:plain", a))
        plain.append(_child(None, "host:plain", a))
    res["host_scaled_1080_to_540"] = dict(_child(None, "host:scaled", a), library="this commit")
    merge = lambda legs: dict(legs[0], **_stat([r for l in legs for r in l["runs"]], 1))
    res["host_plain_540"] = dict(merge(plain), library="this commit")
    if a.parent_lib:
        res["host_plain_540_parent"] = dict(merge(parent), library="parent commit")
        p, t = res["host_plain_540_parent"], res["host_plain_540"]
        spread = p["max"] - p["min"]
        res["plain_path_vs_parent"] = {"parent_median": p["median"], "parent_spread": round(spread, 1), "this_median": t["median"],
                                       "ratio": round(t["median"] / p["median"], 4), "inside_parent_spread": t["median"] >= p["median"] - spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", type=str, default=None, help="librerevst_hip.so built from the parent commit: the plain host leg is measured on it too")
    ap.add_argument("--skip-kernel-legs", action="store_true")
    ap.add_argument("--skip-host-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<case>, host:scaled or host:plain")
    a = ap.parse_args()
    if a.leg:
        pkg = _load_pkg()
        kind, what = a.leg.split(":")
        res = leg_trace(pkg, what, a.repeats) if kind == "trace" else leg_host(pkg, what == "scaled", a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 frames per call, pad / crop, float32 BGR out; rocprofv3 --kernel-trace --stats, one run per leg; ms per call, medians over "
                          "%d calls after a warm-up call" % a.kernel_repeats,
           "host_legs": "%d uint8 BGR frames per call, page-locked buffers, staged copies, profiler off, %d repeats" % (a.frames, a.repeats)}
    keys = ["kernel_" + c for c in MEASURED] + ["host_plain_540", "host_plain_540_parent", "host_scaled_1080_to_540"]
    failed = None
    try:
        measure(a, res)
    except (subprocess.SubprocessError, ValueError, KeyError) as e:      # a leg failed, faulted or hung, or left no usable trace: nothing more is started
        failed = "%s: %s" % (type(e).__name__, str(e)[:300])
        res["stopped"] = "a leg did not complete (%s); the legs after it were not run" % failed
    for k in keys:
        res.setdefault(k, "not measured")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if failed:
        sys.exit("resample_rate: " + failed)


if __name__ == "__main__":
    main()

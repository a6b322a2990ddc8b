#!/usr/bin/env python
"""What an output size costs: the delivery kernel next to the last kernel and the whole launch sequence, and the host -> host rate of a
delivering call.  Writes one JSON object (with --out: to that file, e.g. profiles/deliver.json).  Needs an MI355X; a leg that did not
run is recorded as "not measured", never estimated.

  kernel legs  16 uint8 BGR frames per call through transfer_tensor(pad_crop=True, out_size=): a 1920 x 1080 working frame delivered at
               3840 x 2160 as NV12, as uint8 BGR and as P010, and 960 x 540 delivered at 1920 x 1080 as NV12.  Each leg runs in a process
               of its own under `rocprofv3 --kernel-trace --stats` (no counters in the same run); its kernel trace is cut into calls
               behind every dispatch of deliver_k (a call's last kernel), the first segment (preparation and the warm-up call) is
               dropped, and the medians over the others are recorded: deliver_k, conv_last_k, and the sum of all kernels of the call,
               in ms per 16 frames.  Algorithmic bytes come from the shapes (12 bytes per working pixel read, the delivered frame's
               bytes written); the share of peak is bytes / 8 TB/s over the kernel time: HBM bandwidth is the bound that applies.
  host legs    transfer_frames over --frames uint8 BGR frames per call, page-locked buffers, profiler off, --repeats repeats after a
               warm-up call, each leg in a process of its own: 3840 x 2160 frames with work_size=(1080, 1920) delivered at the source's
               size (out_size="source") as uint8 BGR and as NV12, against the same calls delivering the 1080p working frame; and the
               plain 512 x 512 call with no out_size on this tree's library and -- with --parent-lib -- on a library built from the
               parent commit, the two taking turns.  The plain path is held to the parent's: its median may fall below the parent's by
               the parent's own max - min.
    python tools/deliver_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/deliver.json] [--skip-kernel-legs] [--skip-host-legs]
Every leg is a process in a session of its own.  The first leg that exits non-zero or runs past --leg-timeout ends the measurement: its
whole process group is killed, nothing more is started on the GPU, what was measured so far is written with "not measured" for the rest,
and the tool exits non-zero.
`--leg NAME` runs one leg (what the child processes do; RRV_LIB_PATH names the library).  FORM_CASES adds a 960 x 540 -> 1920 x 1080
`trace:` leg for each output form (uint8 and float32, HWC and planar, P010): not part of the JSON, they let a comparison of two builds
time every deliver_k<OUT> at one size (profiles/stages.txt)."""
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
# case: (working frame, delivered frame, output format, bytes per delivered pixel)
KERNEL_CASES = {"1080_to_2160_nv12": ((1080, 1920), (2160, 3840), "nv12", 1.5), "1080_to_2160_u8": ((1080, 1920), (2160, 3840), "bgr", 3.0),
                "1080_to_2160_p010": ((1080, 1920), (2160, 3840), "p010", 3.0), "540_to_1080_nv12": ((540, 960), (1080, 1920), "nv12", 1.5)}
# one leg for each output form at 540 -> 1080 (every deliver_k<OUT> then has one at that size); main() measures the four above, `--leg trace:<case>` any
FORM_CASES = {"540_to_1080_" + f: ((540, 960), (1080, 1920), f, b) for f, b in (("bgr", 3.0), ("u8_chw", 3.0), ("f32", 12.0), ("f32_chw", 12.0), ("p010", 3.0))}
MEASURED = list(KERNEL_CASES)
KERNEL_CASES.update(FORM_CASES)
# host leg: (source frame, work_size or None, out_size or None, out_format)
HOST_CASES = {"4k_u8_deliver": ((2160, 3840), (1080, 1920), "source", "bgr"), "4k_u8_work": ((2160, 3840), (1080, 1920), None, "bgr"),
              "4k_nv12_deliver": ((2160, 3840), (1080, 1920), "source", "nv12"), "4k_nv12_work": ((2160, 3840), (1080, 1920), None, "nv12"),
              "plain": ((512, 512), None, None, "bgr")}
FRAMES_PER_CALL = 16
PEAK_BYTES_S = 8.0e12


def _stat(v, digits):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits), "runs": [round(x, digits) for x in v]}


def _load_pkg():
    """the package on the library RRV_LIB_PATH names; a library built from the parent commit has no delivering entries, so they leave the
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


def _source(n, H, W, seed=3):
    """n random uint8 BGR source frames [n][H][W][3], four different ones in turn"""
    base = np.random.default_rng(seed).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    return base[np.arange(n) % 4]


def leg_trace(pkg, case, repeats):
    """the work a profiler run traces: preparation at the working size, then 1 + repeats identical delivering calls of 16 frames"""
    import torch
    (H, W), (DH, DW), fmt, _ = KERNEL_CASES[case]
    m = _model(pkg, H, W)
    x = torch.from_numpy(_source(FRAMES_PER_CALL, H, W)).cuda()
    if fmt in ("bgr", "u8_chw", "f32", "f32_chw"):
        kw = dict(out_layout="nchw" if fmt.endswith("_chw") else "nhwc", out_dtype=torch.float32 if fmt.startswith("f32") else torch.uint8)
    else:
        kw = dict(out_layout=fmt)
    torch.cuda.synchronize()
    for _ in range(repeats + 1):
        m.transfer_tensor(x, layout="nhwc", pad_crop=True, out_size=(DH, DW), **kw)
        m.sync()
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "calls": repeats + 1}


def algorithmic(case):
    """bytes of one deliver launch of 16 frames, from the shapes"""
    (H, W), (DH, DW), _, out_bpp = KERNEL_CASES[case]
    return (12.0 * H * W + out_bpp * DH * DW) * FRAMES_PER_CALL


def parse_trace(path):
    """per-call kernel times (ms) of a rocprofv3 kernel trace: a call ends with its deliver_k dispatch; the first segment holds the
    preparation and the warm-up call"""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    ends = [i for i, r in enumerate(rows) if "deliver_k" in r[0]]
    if len(ends) < 2:
        raise ValueError("%s holds %d deliver_k dispatches: nothing to cut calls at" % (path, len(ends)))
    calls = []
    for a, b in zip(ends[:-1], ends[1:]):
        seg = rows[a + 1:b + 1]
        ms = lambda pred: sum(e - s for n, s, e in seg if pred(n)) / 1e6
        calls.append((ms(lambda n: "deliver_k" in n), ms(lambda n: "conv_last_k" in n), ms(lambda n: True), len(seg)))
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
    out_dir = tempfile.mkdtemp(prefix="deliver_rate_")
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
    (H, W), (DH, DW), fmt, _ = KERNEL_CASES[case]
    bytes_ = algorithmic(case)
    dl = _stat([c[0] for c in calls], 4)
    t = dl["median"] * 1e-3
    return {"work_size": [H, W], "delivered": [DH, DW], "output": fmt, "frames_per_call": FRAMES_PER_CALL, "calls": len(calls),
            "kernels_per_call": calls[0][3], "deliver_k_ms": dl, "conv_last_k_ms": _stat([c[1] for c in calls], 4),
            "all_kernels_ms": _stat([c[2] for c in calls], 3), "algorithmic_bytes": int(bytes_), "achieved_TB_s": round(bytes_ / t / 1e12, 3),
            "bound": "HBM bandwidth", "share_of_peak": round(bytes_ / PEAK_BYTES_S / t, 4)}


def leg_host(pkg, case, n, repeats):
    """frames/s host -> host of transfer_frames over n uint8 BGR frames of a HOST_CASES entry"""
    (SH, SW), work, out_size, fmt = HOST_CASES[case]
    WH, WW = work or (SH, SW)
    m = _model(pkg, WH, WW)
    OH, OW = (SH, SW) if out_size == "source" else (WH, WW)
    src = pkg.pinned_empty((n, SH, SW, 3), np.uint8)
    src[...] = _source(n, SH, SW)
    out = pkg.pinned_empty((n, OH, OW, 3) if fmt == "bgr" else (n, pkg.yuv_frame_bytes(OH, OW)), np.uint8)
    kw = {}
    if work:
        kw["work_size"] = work
    if out_size:
        kw["out_size"] = out_size
    if fmt != "bgr":
        kw["out_format"] = fmt
    rates = []
    for k in range(repeats + 1):            # call 0 warms up (workspaces, staging)
        t0 = time.perf_counter()
        m.transfer_frames(src, out=out, **kw)
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    return dict(_stat(rates, 1), unit="frames/s host -> host", frames_per_call=n, source=[SH, SW], work_size=[WH, WW], delivered=[OH, OW], output=fmt)


def _child(lib, leg, a, frames):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames), "--repeats", str(a.repeats)]
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
            parent.append(_child(a.parent_lib, "host:plain", a, a.frames))
        plain.append(_child(None, "host:plain", a, a.frames))
    merge = lambda legs: dict(legs[0], **_stat([r for l in legs for r in l["runs"]], 1))
    res["host_plain_512"] = dict(merge(plain), library="this commit")
    if a.parent_lib:
        res["host_plain_512_parent"] = dict(merge(parent), library="parent commit")
        p, t = res["host_plain_512_parent"], res["host_plain_512"]
        spread = p["max"] - p["min"]
        res["plain_path_vs_parent"] = {"parent_median": p["median"], "parent_spread": round(spread, 1), "this_median": t["median"],
                                       "ratio": round(t["median"] / p["median"], 4), "inside_parent_spread": t["median"] >= p["median"] - spread}
    for case in ("4k_u8_work", "4k_u8_deliver", "4k_nv12_work", "4k_nv12_deliver"):
        res["host_" + case] = dict(_child(None, "host:" + case, a, a.frames_4k), library="this commit")
    for fmt in ("u8", "nv12"):
        w, d = res["host_4k_%s_work" % fmt], res["host_4k_%s_deliver" % fmt]
        res["price_of_4k_delivery_" + fmt] = {"ms_per_frame_working_size": round(1e3 / w["median"], 3), "ms_per_frame_delivered": round(1e3 / d["median"], 3),
                                              "difference_ms_per_frame": round(1e3 / d["median"] - 1e3 / w["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300, help="frames per call of the plain 512 x 512 leg")
    ap.add_argument("--frames-4k", type=int, default=300, help="frames per call of the 3840 x 2160 legs (25 MB of page-locked memory per frame and side)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", type=str, default=None, help="librerevst_hip.so built from the parent commit: the plain host leg is measured on it too")
    ap.add_argument("--skip-kernel-legs", action="store_true")
    ap.add_argument("--skip-host-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<case> or host:<case>")
    a = ap.parse_args()
    if a.leg:
        pkg = _load_pkg()
        kind, what = a.leg.split(":")
        res = leg_trace(pkg, what, a.repeats) if kind == "trace" else leg_host(pkg, what, a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 uint8 BGR frames per call, pad / crop, delivered at twice the working size; rocprofv3 --kernel-trace --stats, one run per "
                          "leg; ms per call, medians over %d calls after a warm-up call" % a.kernel_repeats,
           "host_legs": "uint8 BGR frames, %d per call at 512 x 512 and %d at 3840 x 2160, page-locked buffers, staged copies, profiler off, %d repeats"
                        % (a.frames, a.frames_4k, a.repeats)}
    keys = ["kernel_" + c for c in MEASURED] + ["host_plain_512", "host_plain_512_parent"] + ["host_" + c for c in HOST_CASES if c != "plain"]
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
        sys.exit("deliver_rate: " + failed)


if __name__ == "__main__":
    main()

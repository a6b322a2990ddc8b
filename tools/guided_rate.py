#!/usr/bin/env python
"""What guided delivery costs: its kernels next to bilinear delivery and the whole launch sequence, and the host -> host rate of a guided
call.  Writes one JSON object (with --out: to that file, e.g. profiles/guided.json).  Needs an MI355X; a leg that did not run is recorded
as "not measured", never estimated.  The legs' processes, models and frames are those of tools/deliver_rate.py, which this tool imports.

  kernel legs  16 uint8 BGR frames of the DELIVERED size per call through transfer_tensor(pad_crop=True, work_size=, out_size="source",
               out_layout="nv12"), with guide="source" (radius 4, eps 1e-3) and without: 3840 x 2160 worked on at 1920 x 1080, and
               1920 x 1080 worked on at 960 x 540.  Each leg runs in a process of its own under `rocprofv3 --kernel-trace --stats` (no
               counters in the same run); its kernel trace is cut into calls behind every dispatch of deliver_k (a call's last kernel),
               the first segment (preparation and the warm-up call) is dropped, and the medians over the others are recorded, in ms per
               16 frames: gf_coeff_k, gf_apply_k, the equal-size resample_k (the call's second: X_hi) and deliver_k of a guided call,
               the bilinear deliver_k of a plain one, and the sum of all kernels of either call.  Algorithmic bytes come from the shapes
               (below); the share of peak is bytes / 8 TB/s over the kernel time: HBM bandwidth is the bound that applies.
  host legs    transfer_frames over --frames-4k 3840 x 2160 uint8 BGR frames per call, work_size=(1080, 1920), out_size="source", NV12 out,
               page-locked buffers, profiler off, guided against bilinear; and the plain 512 x 512 call with no out_size on this tree's
               library and -- with --parent-lib -- on a library built from the parent commit, the two taking turns.  The plain path is
               held to the parent's: its median may fall below the parent's by the parent's own max - min.
    python tools/guided_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/guided.json] [--skip-kernel-legs] [--skip-host-legs]
Every leg is a process in a session of its own.  The first leg that exits non-zero or runs past --leg-timeout ends the measurement: its
whole process group is killed, nothing more is started on the GPU, what was measured so far is written with "not measured" for the rest,
and the tool exits non-zero.  `--leg NAME` runs one leg (what the child processes do; RRV_LIB_PATH names the library)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deliver_rate as DR      # noqa: E402  (_run, _stat, _load_pkg, _model, _source, leg_host's plain case)

# case: (working frame, delivered frame = source frame)
KERNEL_CASES = {"1080_to_2160": ((1080, 1920), (2160, 3840)), "540_to_1080": ((540, 960), (1080, 1920))}
FRAMES_PER_CALL = DR.FRAMES_PER_CALL
RADIUS, EPS = 4, 1e-3
GUIDE = dict(guide="source", guide_radius=RADIUS, guide_eps=EPS)
# bytes per frame of one launch, from the shapes (w: working pixels, d: delivered pixels; uint8 BGR source, NV12 out)
ALGORITHMIC = {
    "gf_coeff_k": lambda w, d: 48.0 * w,                          # P and X_lo read (12 each), six coefficient planes written (24)
    "gf_apply_k": lambda w, d: 24.0 * w + 24.0 * d,               # the planes read once (halo rows come from cache), X_hi read and Q written (12 each)
    "resample_k_equal_size": lambda w, d: 15.0 * d,               # the uint8 source read (3), X_hi written (12)
    "deliver_k_equal_size": lambda w, d: 13.5 * d,                # Q read (12), NV12 written (1.5)
    "deliver_k_bilinear": lambda w, d: 12.0 * w + 1.5 * d,
}


def leg_trace(pkg, case, guided, repeats):
    import torch
    (H, W), (DH, DW) = KERNEL_CASES[case]
    m = DR._model(pkg, H, W)
    x = torch.from_numpy(DR._source(FRAMES_PER_CALL, DH, DW)).cuda()
    torch.cuda.synchronize()
    for _ in range(repeats + 1):
        m.transfer_tensor(x, layout="nhwc", pad_crop=True, work_size=(H, W), out_size="source", out_layout="nv12", **(GUIDE if guided else {}))
        m.sync()
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "guided": guided, "calls": repeats + 1}


def parse_trace(path):
    """per call {kernel: ms} of a rocprofv3 kernel trace: a call ends with its deliver_k dispatch; the first segment holds the preparation
    and the warm-up call.  resample_k: the call's first dispatch scales the source down, its second (guided) is the equal-size X_hi pass."""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    ends = [i for i, r in enumerate(rows) if "deliver_k" in r[0]]
    if len(ends) < 2:
        raise ValueError("%s holds %d deliver_k dispatches: nothing to cut calls at" % (path, len(ends)))
    calls = []
    for a, b in zip(ends[:-1], ends[1:]):
        seg = rows[a + 1:b + 1]
        ms = lambda name: [(e - s) / 1e6 for n, s, e in seg if name in n]
        rs = ms("resample_k")
        calls.append({"gf_coeff_k": sum(ms("gf_coeff_k")), "gf_apply_k": sum(ms("gf_apply_k")), "resample_k_working_size": rs[0] if rs else 0.0,
                      "resample_k_equal_size": sum(rs[1:]), "deliver_k": sum(ms("deliver_k")), "conv_last_k": sum(ms("conv_last_k")),
                      "all_kernels": sum((e - s) / 1e6 for _, s, e in seg), "kernels": len(seg)})
    return calls


def kernel_leg(case, guided, a):
    tag = case + ("_guided" if guided else "_bilinear")
    out_dir = tempfile.mkdtemp(prefix="guided_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", tag, "--",
           sys.executable, os.path.abspath(__file__), "--leg", "trace:%s:%d" % (case, guided), "--repeats", str(a.kernel_repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    print("kernel leg %s under rocprofv3" % tag, file=sys.stderr, flush=True)
    try:
        DR._run(cmd, env, a.leg_timeout, subprocess.DEVNULL)
        traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise ValueError("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
        calls = parse_trace(traces[0])
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    (H, W), (DH, DW) = KERNEL_CASES[case]
    res = {"work_size": [H, W], "delivered": [DH, DW], "output": "nv12", "frames_per_call": FRAMES_PER_CALL, "calls": len(calls), "kernels_per_call": calls[0]["kernels"],
           "all_kernels_ms": DR._stat([c["all_kernels"] for c in calls], 3), "conv_last_k_ms": DR._stat([c["conv_last_k"] for c in calls], 4),
           "resample_k_working_size_ms": DR._stat([c["resample_k_working_size"] for c in calls], 4)}
    names = {"gf_coeff_k": "gf_coeff_k", "gf_apply_k": "gf_apply_k", "resample_k_equal_size": "resample_k_equal_size", "deliver_k_equal_size": "deliver_k"} if guided \
        else {"deliver_k_bilinear": "deliver_k"}
    for key, col in names.items():
        st = DR._stat([c[col] for c in calls], 4)
        bytes_ = ALGORITHMIC[key](H * W, DH * DW) * FRAMES_PER_CALL
        t = st["median"] * 1e-3
        res[key] = {"ms": st, "algorithmic_bytes": int(bytes_), "achieved_TB_s": round(bytes_ / t / 1e12, 3), "bound": "HBM bandwidth",
                    "share_of_peak": round(bytes_ / DR.PEAK_BYTES_S / t, 4)}
    return res


def leg_host_4k(pkg, guided, n, repeats):
    """frames/s host -> host of transfer_frames over n 3840 x 2160 uint8 BGR frames, worked on at 1080p, delivered as 4K NV12"""
    (SH, SW), (WH, WW) = (2160, 3840), (1080, 1920)
    m = DR._model(pkg, WH, WW)
    src = pkg.pinned_empty((n, SH, SW, 3), np.uint8)
    src[...] = DR._source(n, SH, SW)
    out = pkg.pinned_empty((n, pkg.yuv_frame_bytes(SH, SW)), np.uint8)
    rates = []
    for k in range(repeats + 1):            # call 0 warms up (workspaces, staging)
        t0 = time.perf_counter()
        m.transfer_frames(src, out=out, work_size=(WH, WW), out_size="source", out_format="nv12", **(GUIDE if guided else {}))
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    return dict(DR._stat(rates, 1), unit="frames/s host -> host", frames_per_call=n, source=[SH, SW], work_size=[WH, WW], delivered=[SH, SW], output="nv12",
                delivery="guided r=%d eps=%g" % (RADIUS, EPS) if guided else "bilinear")


def _child(lib, leg, a, frames):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames), "--repeats", str(a.repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    if lib:
        env["RRV_LIB_PATH"] = os.path.abspath(lib)
    print("leg %s on %s" % (leg, lib or "this tree's library"), file=sys.stderr, flush=True)
    return json.loads(DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().strip().splitlines()[-1])


def measure(a, res):
    """Every leg in order, each in a process of its own; the first one that fails ends the measurement (the exception leaves here)."""
    if not a.skip_kernel_legs:
        for case in KERNEL_CASES:
            for guided in (1, 0):
                key = "kernel_%s_%s" % (case, "guided" if guided else "bilinear")
                res[key] = "not measured (rocprofv3 not found)" if shutil.which("rocprofv3") is None else kernel_leg(case, guided, a)
    if a.skip_host_legs:
        return
    plain, parent = [], []
    for turn in range(2):                    # the two libraries take turns
        if a.parent_lib:
            parent.append(_child(a.parent_lib, "host:plain", a, a.frames))
        plain.append(_child(None, "host:plain", a, a.frames))
    merge = lambda legs: dict(legs[0], **DR._stat([r for l in legs for r in l["runs"]], 1))
    res["host_plain_512"] = dict(merge(plain), library="this commit")
    if a.parent_lib:
        res["host_plain_512_parent"] = dict(merge(parent), library="parent commit")
        p, t = res["host_plain_512_parent"], res["host_plain_512"]
        spread = p["max"] - p["min"]
        res["plain_path_vs_parent"] = {"parent_median": p["median"], "parent_spread": round(spread, 1), "this_median": t["median"],
                                       "ratio": round(t["median"] / p["median"], 4), "inside_parent_spread": t["median"] >= p["median"] - spread}
    for guided in (0, 1):
        res["host_4k_nv12_" + ("guided" if guided else "bilinear")] = dict(_child(None, "host4k:%d" % guided, a, a.frames_4k), library="this commit")
    b, g = res["host_4k_nv12_bilinear"], res["host_4k_nv12_guided"]
    res["price_of_guided_4k_delivery"] = {"ms_per_frame_bilinear": round(1e3 / b["median"], 3), "ms_per_frame_guided": round(1e3 / g["median"], 3),
                                          "difference_ms_per_frame": round(1e3 / g["median"] - 1e3 / b["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300, help="frames per call of the plain 512 x 512 leg")
    ap.add_argument("--frames-4k", type=int, default=300, help="frames per call of the 3840 x 2160 legs (25 MB of page-locked memory per source frame)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", type=str, default=None, help="librerevst_hip.so built from the parent commit: the plain host leg is measured on it too")
    ap.add_argument("--skip-kernel-legs", action="store_true")
    ap.add_argument("--skip-host-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<case>:<guided 0|1>, host:plain or host4k:<guided 0|1>")
    a = ap.parse_args()
    if a.leg:
        pkg = DR._load_pkg()
        kind, *what = a.leg.split(":")
        if kind == "trace":
            res = leg_trace(pkg, what[0], bool(int(what[1])), a.repeats)
        elif kind == "host4k":
            res = leg_host_4k(pkg, bool(int(what[0])), a.frames, a.repeats)
        else:
            res = DR.leg_host(pkg, what[0], a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 uint8 BGR frames per call, pad / crop, worked on at half the source's size and delivered at the source's as NV12, guided (r = %d, "
                          "eps = %g) and bilinear; rocprofv3 --kernel-trace --stats, one run per leg; ms per call, medians over %d calls after a warm-up call"
                          % (RADIUS, EPS, a.kernel_repeats),
           "host_legs": "uint8 BGR frames, %d per call at 512 x 512 and %d at 3840 x 2160, page-locked buffers, staged copies, profiler off, %d repeats"
                        % (a.frames, a.frames_4k, a.repeats)}
    keys = ["kernel_%s_%s" % (c, g) for c in KERNEL_CASES for g in ("guided", "bilinear")] + ["host_plain_512", "host_plain_512_parent", "host_4k_nv12_bilinear",
                                                                                              "host_4k_nv12_guided"]
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
        sys.exit("guided_rate: " + failed)


if __name__ == "__main__":
    main()

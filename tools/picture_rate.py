#!/usr/bin/env python
"""What the picture area costs and saves: the line-profile kernels (include/rerevst_hip.h "Picture area") on 1080p and 2160p frames, a
transfer with a window next to the plain call on the whole frame and on frames of the window's size, the detection pass host to host with
and without the profiles, and the plain call of this commit next to the parent's.  Writes one JSON object (with --out: to that file, e.g.
profiles/picture.json).  Needs an MI355X; a leg that did not run is recorded as "not measured", never estimated.  The processes, the traced
legs and the statistics are tools/shots_rate.py's and tools/deliver_rate.py's.

  kernel legs  16 frames per call through picture_profiles_tensor at 1080p NV12 and 2160p NV12, each in a process of its own under
               `rocprofv3 --kernel-trace --stats` (no counters in the same run): the trace is cut into calls behind every picture_cols_k, the
               first call (warm-up) is dropped, and the medians over five are recorded in ms per 16 frames, with the share of the time that
               12 bytes per pixel would take at 8 TB/s, the bound that applies to picture_lines_k.
  window legs  16 frames of 1080p NV12 -> NV12: transfer_tensor(picture=(138, 0, 804, 1920)), the plain pad / crop call on the whole frame, and
               the plain call on 804 x 1920 frames, traced the same way: all kernels of a call, and resample_k / deliver_k by name.  Pixel
               count lets one expect about 0.74 of the whole frame's kernel time; what is found is recorded.
  pass legs    scan_frames over --frames 512 x 512 uint8 frames in chunks of 32, signatures alone and signatures plus profiles, frames/s.
  plain leg    tools/deliver_rate.py's plain 512 x 512 host call on this commit and -- with --parent-lib -- on a library built from the parent
               commit, the two taking turns: its median may fall below the parent's by the parent's own max - min.
    python tools/picture_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/picture.json] [--skip-kernel-legs] [--skip-window-legs]
The first leg that exits non-zero or runs past --leg-timeout ends the measurement: nothing more is started on the GPU, what was measured is
written, and the tool exits non-zero.  It also exits non-zero when the plain call fell outside the parent's spread."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deliver_rate as DR      # noqa: E402  (_run, _stat, _load_pkg, _model, leg_host's plain case)
import shots_rate as SR        # noqa: E402  (_calls: a kernel trace cut into calls)

FRAMES_PER_CALL = DR.FRAMES_PER_CALL
SIZES = {"1080_nv12": (1080, 1920), "2160_nv12": (2160, 3840)}
WINDOW = (138, 0, 804, 1920)      # a 2.39:1 picture in a 1080p frame
WINDOW_LEGS = ("picture", "plain_full", "plain_window")


def _nv12(H, W):
    import torch
    rng = np.random.default_rng(3)
    return torch.from_numpy(rng.integers(0, 256, (FRAMES_PER_CALL, H * W * 3 // 2), dtype=np.uint8)).cuda()


def leg_trace(pkg, case, repeats):
    """the work a profiler run traces for a kernel leg: 1 + repeats profile calls of 16 frames"""
    import torch
    H, W = SIZES[case]
    x = _nv12(H, W)
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    for _ in range(repeats + 1):
        m.picture_profiles_tensor(x, layout="nv12", size=(H, W))
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "calls": repeats + 1}


def leg_window(pkg, which, repeats):
    """... and for a window leg: 1 + repeats transfer_tensor calls of 16 NV12 frames, NV12 out"""
    import torch
    H, W = SIZES["1080_nv12"]
    y0, x0, h, w = WINDOW
    size = (h, w) if which == "plain_window" else (H, W)
    x = _nv12(*size)
    m = DR._model(pkg, *((h, w) if which != "plain_full" else (H, W)))
    kw = dict(picture=WINDOW) if which == "picture" else dict(pad_crop=True)
    for _ in range(repeats + 1):
        m.transfer_tensor(x, layout="nv12", size=size, out_layout="nv12", **kw)
        torch.cuda.synchronize()
    m.close()
    return {"case": which, "calls": repeats + 1}


def leg_pass(pkg, n, repeats, profiles):
    """frames/s host to host of the detection pass over n 512 x 512 uint8 BGR frames, in chunks of 32"""
    import time
    frames = DR._source(n, 512, 512)
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    rates = []
    for k in range(repeats + 1):            # pass 0 warms up
        t0 = time.perf_counter()
        for c0 in range(0, n, 32):
            m.scan_frames(frames[c0:c0 + 32], signatures=True, profiles=profiles)
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    return dict(DR._stat(rates, 1), unit="frames/s host -> host", frames=n, chunk=32, profiles=profiles)


def traced_leg(kind, case, last, a):
    out_dir = tempfile.mkdtemp(prefix="picture_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "leg", "--",
           sys.executable, os.path.abspath(__file__), "--leg", kind + ":" + case, "--repeats", str(a.kernel_repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    print("%s leg %s under rocprofv3" % (kind, case), file=sys.stderr, flush=True)
    try:
        lines = [ln for ln in DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().splitlines() if ln.startswith("{")]
        if not lines:
            raise ValueError("the leg %s:%s printed no result line" % (kind, case))
        leg = json.loads(lines[-1])
        traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise ValueError("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
        calls = SR._calls(traces[0], last)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    return leg, calls


def kernel_leg(case, a):
    leg, calls = traced_leg("trace", case, "picture_cols_k", a)
    H, W = SIZES[case]
    res = dict(leg, size=[H, W], frames_per_call=FRAMES_PER_CALL, calls=len(calls))
    bound_ms = 12.0 * H * W * FRAMES_PER_CALL / DR.PEAK_BYTES_S * 1e3      # 12 bytes per pixel at the HBM peak
    res["bound_ms_12_bytes_per_pixel_at_8TBs"] = float("%.4g" % bound_ms)
    for k in ("picture_lines_k", "picture_cols_k", "resample_k"):
        res[k + "_ms"] = DR._stat([sum(ms for n, ms in c if k in n) for c in calls], 4)
    t = res["picture_lines_k_ms"]["median"] + res["picture_cols_k_ms"]["median"]
    res["profile_kernels_ms"] = float("%.4g" % t)
    res["bound_share_of_profile_kernels"] = float("%.3g" % (bound_ms / t)) if t > 0 else 0.0
    return res


def window_leg(which, a):
    leg, calls = traced_leg("window", which, "deliver_k" if which == "picture" else "conv_last_k", a)
    res = dict(leg, frames_per_call=FRAMES_PER_CALL, calls=len(calls), all_kernels_ms=DR._stat([sum(ms for _, ms in c) for c in calls], 4))
    for k in ("resample_k", "deliver_k", "conv_first_k", "conv_last_k"):
        res[k + "_ms"] = DR._stat([sum(ms for n, ms in c if k in n) for c in calls], 4)
        res[k + "_launches"] = sum(1 for n, _ in calls[0] if k in n)
    return res


def _child(lib, leg, a, frames):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames), "--repeats", str(a.repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    if lib:
        env["RRV_LIB_PATH"] = os.path.abspath(lib)
    print("leg %s on %s" % (leg, lib or "this tree's library"), file=sys.stderr, flush=True)
    lines = DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().strip().splitlines()
    if not lines:
        raise ValueError("the leg %s printed no result line" % leg)
    return json.loads(lines[-1])


def measure(a, res, save):
    have = shutil.which("rocprofv3") is not None
    if not a.skip_kernel_legs:
        for case in SIZES:
            res["kernel_" + case] = kernel_leg(case, a) if have else "not measured (rocprofv3 not found)"
            save()
    if not a.skip_window_legs:
        for which in WINDOW_LEGS:
            res["window_" + which] = window_leg(which, a) if have else "not measured (rocprofv3 not found)"
            save()
        legs = [res["window_" + w] for w in WINDOW_LEGS]
        if all(isinstance(x, dict) for x in legs):
            p, full, win = (x["all_kernels_ms"]["median"] for x in legs)
            res["window_vs_plain"] = {"window": list(WINDOW), "pixel_share": round(WINDOW[2] * WINDOW[3] / (1080.0 * 1920.0), 4), "picture_over_full": round(p / full, 4),
                                      "window_frames_over_full": round(win / full, 4), "picture_minus_window_frames_ms": round(p - win, 4)}
            save()
    res["detection_pass_512_signatures"] = _child(None, "pass:sig", a, a.frames)
    res["detection_pass_512_both"] = _child(None, "pass:both", a, a.frames)
    save()
    plain, parent = [], []
    for turn in range(2):                    # the two libraries take turns
        if a.parent_lib:
            parent.append(_child(a.parent_lib, "dr_host:plain", a, a.frames))
        plain.append(_child(None, "dr_host:plain", a, a.frames))
    merge = lambda legs: dict(legs[0], **DR._stat([r for l in legs for r in l["runs"]], 1))      # noqa: E731, E741
    res["host_plain_512"] = dict(merge(plain), library="this commit")
    if a.parent_lib:
        res["host_plain_512_parent"] = dict(merge(parent), library="parent commit")
        p, t = res["host_plain_512_parent"], res["host_plain_512"]
        spread = p["max"] - p["min"]
        res["plain_path_vs_parent"] = {"parent_median": p["median"], "parent_spread": round(spread, 1), "this_median": t["median"], "this_spread": round(t["max"] - t["min"], 1),
                                       "ratio": round(t["median"] / p["median"], 4), "inside_parent_spread": t["median"] >= p["median"] - spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300, help="frames of the detection pass and per call of the plain host leg")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", type=str, default=None, help="librerevst_hip.so built from the parent commit: the plain host leg is measured on it too")
    ap.add_argument("--skip-kernel-legs", action="store_true")
    ap.add_argument("--skip-window-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<case>, window:<which>, pass:sig, pass:both or dr_host:plain")
    a = ap.parse_args()
    if a.leg:
        pkg = DR._load_pkg()
        kind, what = a.leg.split(":", 1)
        pkg.Stylization      # (loads the framework module)
        if kind == "trace":
            res = leg_trace(pkg, what, a.repeats)
        elif kind == "window":
            res = leg_window(pkg, what, a.repeats)
        elif kind == "pass":
            res = leg_pass(pkg, a.frames, a.repeats, what == "both")
        else:
            res = DR.leg_host(pkg, what, a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 NV12 frames per call through picture_profiles_tensor; rocprofv3 --kernel-trace --stats, one run per leg, no counters; ms per call, medians "
                          "over %d calls after a warm-up call; the bound is 12 bytes per pixel at the 8 TB/s HBM peak" % a.kernel_repeats,
           "window_legs": "16 frames of 1080p NV12 -> NV12 per transfer_tensor call: picture=%r, the plain pad / crop call on the whole frame, the plain call on frames of the "
                          "window's size; traced the same way: all kernels of a call, ms" % (WINDOW,),
           "pass_legs": "%d uint8 BGR frames of 512 x 512 through scan_frames in chunks of 32; profiler off, %d repeats" % (a.frames, a.repeats),
           "host_legs": "%d frames per call at 512 x 512 (uint8 BGR in and out), page-locked input, profiler off, %d repeats" % (a.frames, a.repeats)}

    def save():      # what is measured so far: a run cut short still leaves its legs
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    failed = None
    try:
        measure(a, res, save)
    except (subprocess.SubprocessError, ValueError) as e:      # a leg failed, faulted or hung, or left no usable trace (ValueError): nothing more is started
        failed = "%s: %s" % (type(e).__name__, str(e)[:300])
        res["stopped"] = "a leg did not complete (%s); the legs after it were not run" % failed
    for k in ["kernel_" + c for c in SIZES] + ["window_" + w for w in WINDOW_LEGS] + ["detection_pass_512_signatures", "detection_pass_512_both", "host_plain_512",
                                                                                   "host_plain_512_parent"]:
        res.setdefault(k, "not measured")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if failed:
        sys.exit("picture_rate: " + failed)
    held = res.get("plain_path_vs_parent")
    if isinstance(held, dict) and not held["inside_parent_spread"]:      # the one condition of the measurement
        sys.exit("picture_rate: the plain 512 x 512 call fell below the parent's median by more than the parent's own spread (ratio %.4f)" % held["ratio"])


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What shot detection costs: shot_sig_k and the thumbnail resample_k (include/rerevst_hip.h "Shots") next to a plain transfer of the same
frames, the detection pass host to host, and the plain call of this commit next to the parent's.  Writes one JSON object (with --out: to that
file, e.g. profiles/shots.json).  Needs an MI355X; a leg that did not run is recorded as "not measured", never estimated.  The processes, the
plain host leg and the statistics are tools/deliver_rate.py's.

  kernel legs  16 frames per call through shot_signatures_tensor at 512 x 512 uint8 BGR, 1080p NV12 and 2160p NV12, each in a process of its
               own under `rocprofv3 --kernel-trace --stats` (no counters in the same run): the trace is cut into calls behind every shot_sig_k,
               the first call (warm-up) is dropped, and the medians over five are recorded in ms per 16 frames, with the bytes each kernel moves
               and the share of 8 TB/s that is (reported, not judged).
  transfer legs  one plain transfer_tensor call of the same 16 frames (the 2160p frames worked on at 1920 x 1080, as the other tools' 4K legs
               are: sixteen 4K working frames need more memory than a shared card has free), traced the same way: the sum of all its kernels,
               next to the figures above.
  pass leg     the detection pass of the driver's --shots auto, host to host: shot_signatures over --frames 512 x 512 uint8 frames in chunks
               of 32, then shot_distances and detect_cuts, in frames/s.
  plain leg    tools/deliver_rate.py's plain 512 x 512 host call on this commit and -- with --parent-lib -- on a library built from the parent
               commit, the two taking turns: its median may fall below the parent's by the parent's own max - min.
    python tools/shots_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/shots.json] [--skip-kernel-legs] [--skip-transfer-legs]
The first leg that exits non-zero or runs past --leg-timeout ends the measurement: nothing more is started on the GPU, what was measured is
written, and the tool exits non-zero.  It also exits non-zero when the plain call fell outside the parent's spread."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deliver_rate as DR      # noqa: E402  (_run, _stat, _load_pkg, leg_host's plain case)

FRAMES_PER_CALL = DR.FRAMES_PER_CALL
# case: (frame size, layout of the tensor entries, source bytes per pixel)
CASES = {"512_u8": ((512, 512), "nhwc", 3.0), "1080_nv12": ((1080, 1920), "nv12", 1.5), "2160_nv12": ((2160, 3840), "nv12", 1.5)}
WORK = {"2160_nv12": (1080, 1920)}      # the working size of a transfer leg, where it is not the frame's


def _frames(case):
    import torch
    (H, W), layout, _ = CASES[case]
    rng = np.random.default_rng(3)
    if layout == "nhwc":
        return torch.from_numpy(rng.integers(0, 256, (FRAMES_PER_CALL, H, W, 3), dtype=np.uint8)).cuda(), dict(layout="nhwc")
    return torch.from_numpy(rng.integers(0, 256, (FRAMES_PER_CALL, H * W * 3 // 2), dtype=np.uint8)).cuda(), dict(layout="nv12", size=(H, W))


def leg_trace(pkg, case, repeats):
    """the work a profiler run traces for a kernel leg: 1 + repeats signature calls of 16 frames"""
    import torch
    x, kw = _frames(case)
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    for _ in range(repeats + 1):
        m.shot_signatures_tensor(x, **kw)
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "calls": repeats + 1}


def leg_xfer(pkg, case, repeats):
    """... and for a transfer leg: 1 + repeats plain transfer_tensor calls of the same 16 frames, uint8 NHWC out"""
    import torch
    (H, W), _, _ = CASES[case]
    x, kw = _frames(case)
    m = DR._model(pkg, *WORK.get(case, (H, W)))
    if case in WORK:
        kw = dict(kw, work_size=WORK[case])
    for _ in range(repeats + 1):
        m.transfer_tensor(x, out_dtype=torch.uint8, out_layout="nhwc", pad_crop=True, **kw)
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "calls": repeats + 1}


def leg_pass(pkg, n, repeats):
    """frames/s host to host of the detection pass over n 512 x 512 uint8 BGR frames, in chunks of 32"""
    import importlib
    import time
    V = importlib.import_module("rerevst-code_amd.video")
    frames = DR._source(n, 512, 512)
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    rates = []
    for k in range(repeats + 1):            # pass 0 warms up
        t0 = time.perf_counter()
        sigs = np.concatenate([m.shot_signatures(frames[c0:c0 + 32]) for c0 in range(0, n, 32)])
        cuts = V.detect_cuts(V.shot_distances(sigs))
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    return dict(DR._stat(rates, 1), unit="frames/s host -> host", frames=n, chunk=32, shots_found=len(cuts))


def _calls(path, last):
    """[(kernel name, ms)] per call of a rocprofv3 kernel trace: a call ends with its kernel whose name contains `last`; the first call is the warm-up"""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    calls, cur = [], []
    for name, s, e in rows:
        cur.append((name, (e - s) / 1e6))
        if last in name:
            calls.append(cur)
            cur = []
    if len(calls) < 2:
        raise ValueError("%s holds %d calls" % (path, len(calls)))
    return calls[1:]


def traced_leg(kind, case, last, a):
    out_dir = tempfile.mkdtemp(prefix="shots_rate_")
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
        calls = _calls(traces[0], last)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    return leg, calls


def kernel_leg(case, a):
    leg, calls = traced_leg("trace", case, "shot_sig_k", a)
    (H, W), _, bpp = CASES[case]
    f = next((k for k in range(1, 9) if -(-max(H, W) // k) <= 512), 8)      # rrv_shot_plan, restated: this process loads no library
    th, tw = -(-H // f), -(-W // f)
    res = dict(leg, size=[H, W], thumbnail=[th, tw], frames_per_call=FRAMES_PER_CALL, calls=len(calls))
    moved = {"shot_sig_k": 12.0 * th * tw + 2048, "resample_k": bpp * H * W + 12.0 * th * tw}
    for k in ("shot_sig_k", "resample_k"):
        res[k + "_ms"] = DR._stat([sum(ms for n, ms in c if k in n) for c in calls], 4)
        t = res[k + "_ms"]["median"] * 1e-3
        res[k + "_bytes_per_call"] = int(moved[k] * FRAMES_PER_CALL)
        res[k + "_share_of_hbm_peak"] = float("%.3g" % (moved[k] * FRAMES_PER_CALL / DR.PEAK_BYTES_S / t)) if t > 0 else 0.0
    res["both_ms"] = DR._stat([sum(ms for _, ms in c) for c in calls], 4)
    return res


def transfer_leg(case, a):
    leg, calls = traced_leg("xfer", case, "conv_last_k", a)
    return dict(leg, size=list(CASES[case][0]), work_size=list(WORK.get(case, CASES[case][0])), frames_per_call=FRAMES_PER_CALL, calls=len(calls), all_kernels_ms=DR._stat([sum(ms for _, ms in c) for c in calls], 4))


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
        for case in CASES:
            res["kernel_" + case] = kernel_leg(case, a) if have else "not measured (rocprofv3 not found)"
            save()
    if not a.skip_transfer_legs:
        for case in CASES:
            res["transfer_" + case] = transfer_leg(case, a) if have else "not measured (rocprofv3 not found)"
            k, t = res.get("kernel_" + case), res["transfer_" + case]      # (no kernel leg with --skip-kernel-legs: no share then)
            if isinstance(k, dict) and isinstance(t, dict):
                t["signature_share_of_a_transfer"] = float("%.3g" % (k["both_ms"]["median"] / t["all_kernels_ms"]["median"]))
            save()
    res["detection_pass_512"] = _child(None, "pass:512", a, a.frames)
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
    ap.add_argument("--skip-transfer-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<case>, xfer:<case>, pass:512 or dr_host:plain")
    a = ap.parse_args()
    if a.leg:
        pkg = DR._load_pkg()
        kind, what = a.leg.split(":", 1)
        pkg.Stylization      # (loads the framework module)
        if kind == "trace":
            res = leg_trace(pkg, what, a.repeats)
        elif kind == "xfer":
            res = leg_xfer(pkg, what, a.repeats)
        elif kind == "pass":
            res = leg_pass(pkg, a.frames, a.repeats)
        else:
            res = DR.leg_host(pkg, what, a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 frames per call through shot_signatures_tensor; rocprofv3 --kernel-trace --stats, one run per leg, no counters; ms per call, medians over "
                          "%d calls after a warm-up call; the share of the 8 TB/s HBM peak is reported, not judged" % a.kernel_repeats,
           "transfer_legs": "one plain transfer_tensor call of the same 16 frames (pad / crop, uint8 NHWC out), traced the same way: all its kernels, ms per call",
           "pass_leg": "%d uint8 BGR frames of 512 x 512 through shot_signatures in chunks of 32, then shot_distances and detect_cuts; profiler off, %d repeats" % (a.frames, a.repeats),
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
    for k in ["kernel_" + c for c in CASES] + ["transfer_" + c for c in CASES] + ["detection_pass_512", "host_plain_512", "host_plain_512_parent"]:
        res.setdefault(k, "not measured")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if failed:
        sys.exit("shots_rate: " + failed)
    held = res.get("plain_path_vs_parent")
    if isinstance(held, dict) and not held["inside_parent_spread"]:      # the one condition of the measurement
        sys.exit("shots_rate: the plain 512 x 512 call fell below the parent's median by more than the parent's own spread (ratio %.4f)" % held["ratio"])


if __name__ == "__main__":
    main()

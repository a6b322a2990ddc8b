#!/usr/bin/env python
"""What compositing costs: composite_k and the equal-size passes it adds next to the whole launch sequence, and the host -> host rate of a
compositing call.  Writes one JSON object (with --out: to that file, e.g. profiles/composite.json).  Needs an MI355X; a leg that did not
run is recorded as "not measured", never estimated.  The legs' processes, models and frames are those of tools/deliver_rate.py, which this
tool imports.

  kernel legs  16 frames per call through transfer_tensor, with the compositing keywords and without: 512 x 512 uint8 BGR, plain, strength 0.5
               and a uint8 matte; and 3840 x 2160 NV12 worked on at 1920 x 1080 (pad / crop) and delivered at the source's size as NV12,
               bilinear and guided (radius 4, eps 1e-3), strength 0.5 and a float32 matte.  Each leg runs in a process of its own under
               `rocprofv3 --kernel-trace --stats` (no counters in the same run); its kernel trace is cut into calls behind every call's last
               kernel (a compositing call: the deliver_k behind composite_k; else its last deliver_k or conv_last_k), the first segment
               (preparation and the warm-up call) is dropped, and the medians over the others are recorded, in ms per 16 frames:
               composite_k, the equal-size resample_k and deliver_k the request adds, and the sum of all kernels of either call.
               Algorithmic bytes come from the shapes (below); the share of peak is bytes / 8 TB/s over the kernel time: HBM bandwidth is
               the bound that applies.
  host legs    transfer_frames over --frames 512 x 512 uint8 BGR frames per call with and without compositing, and over --frames-4k
               3840 x 2160 NV12 frames (work_size=(1080, 1920), out_size="source", NV12 out) likewise; page-locked buffers, profiler off.
               The plain 512 x 512 call also runs -- with --parent-lib -- on a library built from the parent commit, the two taking turns:
               the plain path is held to the parent's, its median may fall below the parent's by the parent's own max - min.
    python tools/composite_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/composite.json] [--skip-kernel-legs] [--skip-host-legs]
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

FRAMES_PER_CALL = DR.FRAMES_PER_CALL
RADIUS, EPS = 4, 1e-3
STRENGTH = 0.5
# case: (source frame, working frame or None, guided, matte dtype)
CASES = {"512_plain_u8_matte": ((512, 512), None, False, np.uint8),
         "2160_nv12_bilinear_f32_matte": ((2160, 3840), (1080, 1920), False, np.float32),
         "2160_nv12_guided_f32_matte": ((2160, 3840), (1080, 1920), True, np.float32)}
# bytes per delivered pixel of one launch, from the shapes
ALGORITHMIC = {
    "composite_k": lambda matte: 36.0 + np.dtype(matte).itemsize,      # P and S read (12 each), the result written (12), the matte read
    "resample_k_equal_size": lambda in_bpp: in_bpp + 12.0,             # the source read, S written
    "deliver_k_equal_size": lambda out_bpp: 12.0 + out_bpp,            # the mixed frame read, the output form written
}


def _matte(dtype, H, W):
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, (1, H, W), dtype=np.uint8) if dtype == np.uint8 else rng.random((1, H, W), dtype=np.float32)


def _call_kw(case, composite, torch=None):
    (SH, SW), work, guided, mdt = CASES[case]
    kw = {}
    if work:
        kw.update(work_size=work, out_size="source", pad_crop=True)
        if guided:
            kw.update(guide="source", guide_radius=RADIUS, guide_eps=EPS)
    if composite:
        m = _matte(mdt, SH, SW)
        kw.update(strength=STRENGTH, matte=torch.from_numpy(m).cuda() if torch is not None else m)
    return kw


def leg_trace(pkg, case, composite, repeats):
    import torch
    (SH, SW), work, guided, _ = CASES[case]
    m = DR._model(pkg, *(work or (SH, SW)))
    if work:      # NV12 in and out
        x = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (FRAMES_PER_CALL, pkg.yuv_frame_bytes(SH, SW)), dtype=np.uint8)).cuda()
        io = dict(layout="nv12", size=(SH, SW))
    else:
        x = torch.from_numpy(DR._source(FRAMES_PER_CALL, SH, SW)).cuda()
        io = dict(layout="nhwc", out_dtype=torch.uint8)
    kw = _call_kw(case, composite, torch)
    torch.cuda.synchronize()
    for _ in range(repeats + 1):
        m.transfer_tensor(x, **io, **kw)
        m.sync()
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "composite": composite, "calls": repeats + 1}


def parse_trace(path, composite):
    """per call {kernel: ms} of a rocprofv3 kernel trace.  A compositing call ends with the deliver_k behind its composite_k; another call with its
    last kernel: deliver_k if it has one, else conv_last_k.  The first segment holds the preparation and the warm-up call."""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    if composite:
        ends = [i + 1 for i, r in enumerate(rows) if "composite_k" in r[0] and i + 1 < len(rows) and "deliver_k" in rows[i + 1][0]]
    else:
        last = "deliver_k" if any("deliver_k" in r[0] for r in rows) else "conv_last_k"
        ends = [i for i, r in enumerate(rows) if last in r[0]]
    if len(ends) < 2:
        raise ValueError("%s holds %d call ends: nothing to cut calls at" % (path, len(ends)))
    calls = []
    for a, b in zip(ends[:-1], ends[1:]):
        seg = rows[a + 1:b + 1]
        ms = lambda name: [(e - s) / 1e6 for n, s, e in seg if name in n]
        calls.append({"composite_k": sum(ms("composite_k")), "resample_k": ms("resample_k"), "deliver_k": ms("deliver_k"), "conv_last_k": sum(ms("conv_last_k")),
                      "all_kernels": sum((e - s) / 1e6 for _, s, e in seg), "kernels": len(seg)})
    return calls


def kernel_leg(case, composite, a):
    tag = case + ("_composite" if composite else "_without")
    out_dir = tempfile.mkdtemp(prefix="composite_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", tag, "--",
           sys.executable, os.path.abspath(__file__), "--leg", "trace:%s:%d" % (case, composite), "--repeats", str(a.kernel_repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    print("kernel leg %s under rocprofv3" % tag, file=sys.stderr, flush=True)
    try:
        DR._run(cmd, env, a.leg_timeout, subprocess.DEVNULL)
        traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise ValueError("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
        calls = parse_trace(traces[0], composite)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    (SH, SW), work, guided, mdt = CASES[case]
    res = {"source": [SH, SW], "work_size": list(work or (SH, SW)), "delivered": [SH, SW], "input": "nv12" if work else "uint8 bgr", "output": "nv12" if work else "uint8 bgr",
           "delivery": "none" if not work else "guided r=%d eps=%g" % (RADIUS, EPS) if guided else "bilinear", "frames_per_call": FRAMES_PER_CALL, "calls": len(calls),
           "kernels_per_call": calls[0]["kernels"], "all_kernels_ms": DR._stat([c["all_kernels"] for c in calls], 3),
           "conv_last_k_ms": DR._stat([c["conv_last_k"] for c in calls], 4)}
    if not composite:
        return res
    res["request"] = "strength %g, one %s matte for every frame" % (STRENGTH, np.dtype(mdt).name)
    px = float(SH * SW) * FRAMES_PER_CALL
    io_bpp = 1.5 if work else 3.0
    # the passes the request adds: the equal-size deliver_k is the call's last; the equal-size resample_k its last too, unless the guided stage
    # made X_hi already (then none is added)
    cols = {"composite_k": ([c["composite_k"] for c in calls], ALGORITHMIC["composite_k"](mdt)),
            "deliver_k_equal_size": ([c["deliver_k"][-1] for c in calls], ALGORITHMIC["deliver_k_equal_size"](io_bpp))}
    if not guided:
        cols["resample_k_equal_size"] = ([c["resample_k"][-1] for c in calls], ALGORITHMIC["resample_k_equal_size"](io_bpp))
    if work and not guided:
        res["deliver_k_bilinear_to_float32_ms"] = DR._stat([c["deliver_k"][0] for c in calls], 4)
    for key, (v, bpp) in cols.items():
        st = DR._stat(v, 4)
        t = st["median"] * 1e-3
        res[key] = {"ms": st, "algorithmic_bytes": int(bpp * px), "achieved_TB_s": round(bpp * px / t / 1e12, 3), "bound": "HBM bandwidth",
                    "share_of_peak": round(bpp * px / DR.PEAK_BYTES_S / t, 4), "added_by_the_request": key != "deliver_k_equal_size" or not guided}
    return res


def leg_host(pkg, case, composite, n, repeats):
    """frames/s host -> host of transfer_frames over n frames of a CASES entry"""
    (SH, SW), work, guided, _ = CASES[case]
    m = DR._model(pkg, *(work or (SH, SW)))
    if work:
        src = pkg.pinned_empty((n, pkg.yuv_frame_bytes(SH, SW)), np.uint8)
        src[...] = np.random.default_rng(3).integers(0, 256, (4, src.shape[1]), dtype=np.uint8)[np.arange(n) % 4]
        out = pkg.pinned_empty((n, pkg.yuv_frame_bytes(SH, SW)), np.uint8)
        io = dict(in_format="nv12", size=(SH, SW), out_format="nv12")
        call = m.transfer_frames
    else:
        src = pkg.pinned_empty((n, SH, SW, 3), np.uint8)
        src[...] = DR._source(n, SH, SW)
        out = pkg.pinned_empty((n, SH, SW, 3), np.uint8)
        io = {}
        call = m.transfer_batch
    kw = _call_kw(case, composite)
    kw.pop("pad_crop", None)
    rates = []
    for k in range(repeats + 1):            # call 0 warms up (workspaces, staging)
        t0 = time.perf_counter()
        call(src, out=out, **io, **kw)
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    return dict(DR._stat(rates, 1), unit="frames/s host -> host", frames_per_call=n, case=case, composite=bool(composite))


def _child(lib, leg, a, frames):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames), "--repeats", str(a.repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    if lib:
        env["RRV_LIB_PATH"] = os.path.abspath(lib)
    print("leg %s on %s" % (leg, lib or "this tree's library"), file=sys.stderr, flush=True)
    return json.loads(DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().strip().splitlines()[-1])


HOST_CASES = ("512_plain_u8_matte", "2160_nv12_bilinear_f32_matte")


def measure(a, res):
    """Every leg in order, each in a process of its own; the first one that fails ends the measurement (the exception leaves here)."""
    if not a.skip_kernel_legs:
        for case in CASES:
            for composite in (1, 0):
                key = "kernel_%s_%s" % (case, "composite" if composite else "without")
                res[key] = "not measured (rocprofv3 not found)" if shutil.which("rocprofv3") is None else kernel_leg(case, composite, a)
            c, w = res["kernel_%s_composite" % case], res["kernel_%s_without" % case]
            if isinstance(c, dict) and isinstance(w, dict):
                res["price_%s" % case] = {"all_kernels_ms_without": w["all_kernels_ms"]["median"], "all_kernels_ms_composite": c["all_kernels_ms"]["median"],
                                          "difference_ms_per_16_frames": round(c["all_kernels_ms"]["median"] - w["all_kernels_ms"]["median"], 3)}
    if a.skip_host_legs:
        return
    plain, parent = [], []
    for turn in range(2):                    # the two libraries take turns
        if a.parent_lib:
            parent.append(_child(a.parent_lib, "dr_host:plain", a, a.frames))
        plain.append(_child(None, "dr_host:plain", a, a.frames))
    merge = lambda legs: dict(legs[0], **DR._stat([r for l in legs for r in l["runs"]], 1))
    res["host_plain_512"] = dict(merge(plain), library="this commit")
    if a.parent_lib:
        res["host_plain_512_parent"] = dict(merge(parent), library="parent commit")
        p, t = res["host_plain_512_parent"], res["host_plain_512"]
        spread = p["max"] - p["min"]
        res["plain_path_vs_parent"] = {"parent_median": p["median"], "parent_spread": round(spread, 1), "this_median": t["median"], "this_spread": round(t["max"] - t["min"], 1),
                                       "ratio": round(t["median"] / p["median"], 4), "inside_parent_spread": t["median"] >= p["median"] - spread}
    for case in HOST_CASES:
        n = a.frames_4k if CASES[case][1] else a.frames
        for composite in (0, 1):
            res["host_%s_%s" % (case, "composite" if composite else "without")] = dict(_child(None, "host:%s:%d" % (case, composite), a, n), library="this commit")
        w, c = res["host_%s_without" % case], res["host_%s_composite" % case]
        res["host_price_%s" % case] = {"ms_per_frame_without": round(1e3 / w["median"], 3), "ms_per_frame_composite": round(1e3 / c["median"], 3),
                                       "difference_ms_per_frame": round(1e3 / c["median"] - 1e3 / w["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300, help="frames per call of the 512 x 512 legs")
    ap.add_argument("--frames-4k", type=int, default=300, help="frames per call of the 3840 x 2160 NV12 legs (12 MB of page-locked memory per frame and side)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", type=str, default=None, help="librerevst_hip.so built from the parent commit: the plain host leg is measured on it too")
    ap.add_argument("--skip-kernel-legs", action="store_true")
    ap.add_argument("--skip-host-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<case>:<composite 0|1>, host:<case>:<composite 0|1> or dr_host:plain")
    a = ap.parse_args()
    if a.leg:
        pkg = DR._load_pkg()
        kind, *what = a.leg.split(":")
        if kind == "trace":
            res = leg_trace(pkg, what[0], bool(int(what[1])), a.repeats)
        elif kind == "host":
            res = leg_host(pkg, what[0], bool(int(what[1])), a.frames, a.repeats)
        else:
            res = DR.leg_host(pkg, what[0], a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 frames per call, strength %g and one matte for every frame, with and without the request; rocprofv3 --kernel-trace --stats, one run per "
                          "leg; ms per call, medians over %d calls after a warm-up call" % (STRENGTH, a.kernel_repeats),
           "host_legs": "%d frames per call at 512 x 512 (uint8 BGR) and %d at 3840 x 2160 (NV12 in and out, worked on at 1920 x 1080), page-locked buffers, staged "
                        "copies, profiler off, %d repeats" % (a.frames, a.frames_4k, a.repeats)}
    keys = ["kernel_%s_%s" % (c, g) for c in CASES for g in ("composite", "without")] + ["host_plain_512", "host_plain_512_parent"] + \
           ["host_%s_%s" % (c, g) for c in HOST_CASES for g in ("without", "composite")]
    failed = None
    try:
        measure(a, res)
    except (subprocess.SubprocessError, ValueError, KeyError, IndexError) as e:      # a leg failed, faulted or hung, or left no usable trace: nothing more is started
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
        sys.exit("composite_rate: " + failed)


if __name__ == "__main__":
    main()

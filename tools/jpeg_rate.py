#!/usr/bin/env python
"""What JPEG output costs: the stage's kernels next to the whole launch sequence, the host -> host rate of a call that returns JPEG data next to
the uint8 call, and the file-writing driver with --gpu-jpeg next to its Pillow .avi path.  Writes one JSON object (with --out: to that file,
e.g. profiles/jpeg.json).  Needs an MI355X; a leg that did not run is recorded as "not measured", never estimated.  The legs' processes,
models and frames are those of tools/deliver_rate.py, which this tool imports.

  kernel legs  16 frames per call through transfer_tensor(out_layout="jpeg"), quality 90, 4:2:0: 512 x 512 uint8 BGR, and 3840 x 2160 NV12 worked
               on at 1920 x 1080 (pad / crop) and delivered at the source's size.  Each leg runs in a process of its own under `rocprofv3
               --kernel-trace --stats` (no counters in the same run); the trace is cut into calls behind every jpeg_entropy_k<1>, the first
               segment (preparation and the warm-up call) is dropped, and the medians over the others are recorded in ms per 16 frames: every
               kernel of the stage, conv_last_k next to them, and the sum of all kernels of the call.  bytes_per_pixel is what the call
               produced (the sizes it returned), for these frames: stylized noise, which compresses badly.
  host legs    transfer_batch over --frames 512 x 512 uint8 BGR frames per call, JPEG out and uint8 out; page-locked input, profiler off.
               The plain 512 x 512 call of tools/deliver_rate.py also runs -- with --parent-lib -- on a library built from the parent commit, the
               two taking turns: the plain path is held to the parent's, its median may fall below the parent's by the parent's own max - min.
  driver legs  rerevst-code_amd.driver over --driver-frames 512 x 512 PNG files, --video x.avi --no-frames, with --gpu-jpeg and without (Pillow on
               worker threads), same quality; frames/s file -> file as the driver reports it.
    python tools/jpeg_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/jpeg.json] [--skip-kernel-legs] [--skip-host-legs]
Every leg is a process in a session of its own.  The first leg that exits non-zero or runs past --leg-timeout ends the measurement: its whole
process group is killed, nothing more is started on the GPU, what was measured so far is written with "not measured" for the rest, and the
tool exits non-zero.  It also exits non-zero, with everything written, when the plain call measured on both libraries fell outside the
parent's spread.  `--leg NAME` runs one leg (what the child processes do; RRV_LIB_PATH names the library)."""
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
QUALITY, CHROMA = 90, "420"
# case: (source frame, working frame or None)
CASES = {"512": ((512, 512), None), "2160_at_1080": ((2160, 3840), (1080, 1920))}
STAGE = ("jpeg_blocks_k", "jpeg_entropy_k<0>", "jpeg_place_k", "jpeg_entropy_k<1>")


def leg_trace(pkg, case, repeats):
    import torch
    (SH, SW), work = CASES[case]
    m = DR._model(pkg, *(work or (SH, SW)))
    if work:
        x = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (FRAMES_PER_CALL, pkg.yuv_frame_bytes(SH, SW)), dtype=np.uint8)).cuda()
        kw = dict(layout="nv12", size=(SH, SW), work_size=work, out_size="source", pad_crop=True)
    else:
        x = torch.from_numpy(DR._source(FRAMES_PER_CALL, SH, SW)).cuda()
        kw = dict(layout="nhwc")
    torch.cuda.synchronize()
    for _ in range(repeats + 1):
        data, sizes = m.transfer_tensor(x, out_layout="jpeg", jpeg_quality=QUALITY, jpeg_chroma=CHROMA, jpeg_cap=4 * SH * SW + 631, **kw)      # (room for noise)
        m.sync()
        torch.cuda.synchronize()
    sizes = sizes.cpu().numpy()
    m.close()
    if (sizes <= 0).any():
        raise ValueError("a frame did not fit its slot: %r" % sizes.tolist())
    return {"case": case, "calls": repeats + 1, "bytes_per_pixel": round(float(sizes.mean()) / (SH * SW), 4)}


def _kernel(name):
    """the stage's name of a traced kernel (the trace holds demangled or mangled symbols), else None"""
    for key, marks in (("jpeg_entropy_k<0>", ("jpeg_entropy_k<0>", "jpeg_entropy_kILi0E")), ("jpeg_entropy_k<1>", ("jpeg_entropy_k<1>", "jpeg_entropy_kILi1E")),
                       ("jpeg_blocks_k", ("jpeg_blocks_k",)), ("jpeg_place_k", ("jpeg_place_k",)), ("conv_last_k", ("conv_last_k",))):
        if any(mk in name for mk in marks):
            return key
    return None


def parse_trace(path):
    """per call {kernel: ms} of a rocprofv3 kernel trace: a call ends with its last jpeg_entropy_k<1>.  The first segment holds the preparation and
    the warm-up call."""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    ends = [i for i, r in enumerate(rows) if _kernel(r[0]) == "jpeg_entropy_k<1>" and (i + 1 == len(rows) or _kernel(rows[i + 1][0]) not in STAGE)]
    if len(ends) < 2:
        raise ValueError("%s holds %d call ends: nothing to cut calls at" % (path, len(ends)))
    calls = []
    for a, b in zip(ends[:-1], ends[1:]):
        seg = rows[a + 1:b + 1]
        c = {k: sum((e - s) / 1e6 for n, s, e in seg if _kernel(n) == k) for k in STAGE + ("conv_last_k",)}
        c.update(all_kernels=sum((e - s) / 1e6 for _, s, e in seg), kernels=len(seg))
        calls.append(c)
    return calls


def kernel_leg(case, a):
    out_dir = tempfile.mkdtemp(prefix="jpeg_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", case, "--",
           sys.executable, os.path.abspath(__file__), "--leg", "trace:" + case, "--repeats", str(a.kernel_repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    print("kernel leg %s under rocprofv3" % case, file=sys.stderr, flush=True)
    try:
        leg = json.loads([ln for ln in DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().splitlines() if ln.startswith("{")][-1])      # (the profiler prints too)
        traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise ValueError("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
        calls = parse_trace(traces[0])
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    (SH, SW), work = CASES[case]
    res = {"source": [SH, SW], "work_size": list(work or (SH, SW)), "delivered": [SH, SW], "input": "nv12" if work else "uint8 bgr", "quality": QUALITY, "chroma": CHROMA,
           "frames_per_call": FRAMES_PER_CALL, "calls": len(calls), "kernels_per_call": calls[0]["kernels"], "bytes_per_pixel": leg["bytes_per_pixel"],
           "all_kernels_ms": DR._stat([c["all_kernels"] for c in calls], 3), "conv_last_k_ms": DR._stat([c["conv_last_k"] for c in calls], 4)}
    px = float(SH * SW) * FRAMES_PER_CALL
    for k in STAGE:
        res[k + "_ms"] = DR._stat([c[k] for c in calls], 4)
    res["stage_ms"] = DR._stat([sum(c[k] for k in STAGE) for c in calls], 4)
    # the first half against its bound: 12 bytes per pixel read, 3 written (1.5 samples of two bytes), at 8 TB/s
    t = res["jpeg_blocks_k_ms"]["median"] * 1e-3
    res["jpeg_blocks_k_share_of_hbm_peak"] = round(15.0 * px / DR.PEAK_BYTES_S / t, 4)
    return res


def leg_host(pkg, jpeg, n, repeats):
    """frames/s host -> host of transfer_batch over n 512 x 512 uint8 BGR frames, JPEG out or uint8 out"""
    m = DR._model(pkg, 512, 512)
    src = pkg.pinned_empty((n, 512, 512, 3), np.uint8)
    src[...] = DR._source(n, 512, 512)
    out = None if jpeg else pkg.pinned_empty((n, 512, 512, 3), np.uint8)
    rates, nbytes = [], 0
    for k in range(repeats + 1):            # call 0 warms up (workspaces, staging)
        t0 = time.perf_counter()
        if jpeg:
            got = m.transfer_batch(src, out_format="jpeg", jpeg_quality=QUALITY, jpeg_chroma=CHROMA, jpeg_cap=4 * 512 * 512 + 631)      # (room for noise)
            nbytes = sum(len(g) for g in got)
        else:
            m.transfer_batch(src, out=out)
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    res = dict(DR._stat(rates, 1), unit="frames/s host -> host", frames_per_call=n, output="jpeg q%d %s" % (QUALITY, CHROMA) if jpeg else "uint8 bgr")
    if jpeg:
        res["bytes_per_pixel"] = round(nbytes / (n * 512.0 * 512.0), 4)
    return res


def leg_driver(pkg, gpu_jpeg, n):
    """frames/s file -> file of the driver over n 512 x 512 PNG files into an .avi, no frame files"""
    import importlib
    from PIL import Image
    D = importlib.import_module("rerevst-code_amd.driver")
    tmp = tempfile.mkdtemp(prefix="jpeg_rate_driver_")
    try:
        for i, f in enumerate(DR._source(n, 512, 512)):
            Image.fromarray(f[..., ::-1].copy()).save(os.path.join(tmp, "f%05d.png" % i), compress_level=1)
        Image.fromarray(pkg.synth_style(512, 512, kind="noise", seed=7)[..., ::-1].copy()).save(os.path.join(tmp, "style.png"))
        stats = {}
        model = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
        kw = dict(gpu_jpeg=dict(quality=95, chroma=CHROMA)) if gpu_jpeg else {}
        paths = D.list_frames(os.path.join(tmp, "f*.png"))
        for _ in range(2):      # the first run warms up (workspaces, staging, the page cache)
            D.stylize_files(model, os.path.join(tmp, "style.png"), paths, os.path.join(tmp, "out"), os.path.join(tmp, "v.avi"), 24, stats=stats, write_frames=False,
                            log=lambda *a, **k: None, **kw)
        model.close()
        size = os.path.getsize(os.path.join(tmp, "v.avi"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {"frames_per_s": round(stats["frames_per_s"], 1), "unit": "frames/s file -> file", "frames": n, "gpu_call_s": round(stats["gpu_call_s"], 3),
            "io_threads": stats["io_threads"], "avi_bytes": size, "encoder": "GPU (--gpu-jpeg)" if gpu_jpeg else "Pillow on the worker threads", "quality": 95}


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
        for case in CASES:
            res["kernel_" + case] = "not measured (rocprofv3 not found)" if shutil.which("rocprofv3") is None else kernel_leg(case, a)
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
    res["host_512_uint8"] = dict(_child(None, "host:0", a, a.frames), library="this commit")
    res["host_512_jpeg"] = dict(_child(None, "host:1", a, a.frames), library="this commit")
    res["driver_avi_pillow"] = _child(None, "driver:0", a, a.driver_frames)
    res["driver_avi_gpu_jpeg"] = _child(None, "driver:1", a, a.driver_frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300, help="frames per call of the host legs")
    ap.add_argument("--driver-frames", type=int, default=192, help="PNG files of the driver legs")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", type=str, default=None, help="librerevst_hip.so built from the parent commit: the plain host leg is measured on it too")
    ap.add_argument("--skip-kernel-legs", action="store_true")
    ap.add_argument("--skip-host-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<case>, host:<jpeg 0|1>, driver:<gpu jpeg 0|1> or dr_host:plain")
    a = ap.parse_args()
    if a.leg:
        pkg = DR._load_pkg()
        kind, *what = a.leg.split(":")
        if kind == "trace":
            res = leg_trace(pkg, what[0], a.repeats)
        elif kind == "host":
            res = leg_host(pkg, bool(int(what[0])), a.frames, a.repeats)
        elif kind == "driver":
            res = leg_driver(pkg, bool(int(what[0])), a.frames)
        else:
            res = DR.leg_host(pkg, what[0], a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 frames per call, quality %d, %s; rocprofv3 --kernel-trace --stats, one run per leg; ms per call, medians over %d calls after a warm-up call"
                          % (QUALITY, CHROMA, a.kernel_repeats),
           "host_legs": "%d frames per call at 512 x 512 (uint8 BGR in), page-locked input, profiler off, %d repeats; the driver over %d PNG files, second of two runs"
                        % (a.frames, a.repeats, a.driver_frames)}
    keys = ["kernel_" + c for c in CASES] + ["host_plain_512", "host_plain_512_parent", "host_512_uint8", "host_512_jpeg", "driver_avi_pillow", "driver_avi_gpu_jpeg"]
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
        sys.exit("jpeg_rate: " + failed)
    held = res.get("plain_path_vs_parent")
    if isinstance(held, dict) and not held["inside_parent_spread"]:      # the one condition of the measurement
        sys.exit("jpeg_rate: the plain 512 x 512 call fell below the parent's median by more than the parent's own spread (ratio %.4f)" % held["ratio"])


if __name__ == "__main__":
    main()

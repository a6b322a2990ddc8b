#!/usr/bin/env python
"""What JPEG input costs: the three kernels of the stage (include/rerevst_hip.h "JPEG input") on three kinds of stream, and the plain call of this
commit next to the parent's.  Writes one JSON object (with --out: to that file, e.g. profiles/jpeg_in.json).  Needs an MI355X; a leg that did
not run is recorded as "not measured", never estimated.  The processes, the plain host leg and the statistics are tools/deliver_rate.py's.

  kernel legs  16 frames per call through decode_jpeg_tensor, quality 90, 4:2:0, at 512 x 512 and at 3840 x 2160, for three kinds of stream:
               "own" the project's encoder (one MCU row per restart interval), "pillow_rows" Pillow with restart_marker_rows=1, "pillow_none"
               Pillow without restart markers (one lane per frame).  The frames are the synthetic smooth frames of the package.  Each leg runs
               in a process of its own under `rocprofv3 --kernel-trace --stats` (no counters in the same run); the trace is cut into calls behind
               every jpeg_planes_k, the first call (warm-up) is dropped and the medians over the others are recorded in ms per 16 frames, with
               the bytes each kernel moves and the share of 8 TB/s that is.
  transfer legs  16 frames per call through transfer_frames(in_format="jpeg"), traced the same way: the three kernels next to conv_first_k and the sum
               of all kernels of the call, at 512 x 512 and at 3840 x 2160 worked on at 1920 x 1080 and delivered at the source's size.
  driver legs  rerevst-code_amd.driver.stylize_files over --driver-frames 512 x 512 frames into an .avi encoded on the GPU, no frame files: .jpg files
               decoded by Pillow on the worker threads, the same files with gpu_decode, and the same streams as an MJPG .avi's chunks.
  host legs    transfer_batch over --frames 512 x 512 frames per call, page-locked uint8 buffers: uint8 BGR in and out, JPEG streams in (Pillow, one restart
               interval per MCU row) with uint8 out, and the same streams in with JPEG out.
  plain leg    tools/deliver_rate.py's plain 512 x 512 host call on this commit and -- with --parent-lib -- on a library built from the parent
               commit, the two taking turns: its median may fall below the parent's by the parent's own max - min.
    python tools/jpeg_in_rate.py [--parent-lib PATH/librerevst_hip.so] [--out profiles/jpeg_in.json] [--skip-kernel-legs] [--skip-host-legs]
The first leg that exits non-zero or runs past --leg-timeout ends the measurement: nothing more is started on the GPU, what was measured is
written, and the tool exits non-zero.  It also exits non-zero when the plain call fell outside the parent's spread."""
import argparse
import csv
import glob
import io
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
QUALITY = 90
SIZES = {"512": (512, 512), "2160": (2160, 3840)}
KINDS = ("own", "pillow_rows", "pillow_none")
STAGE = ("jpeg_marks_k", "jpeg_huff_k", "jpeg_planes_k")


def _streams(pkg, kind, H, W):
    import torch
    from PIL import Image
    F = sys.modules[pkg.__name__ + ".framework"]
    frames = np.stack([pkg.synth_frame(i, H, W, kind="smooth") for i in range(FRAMES_PER_CALL)])
    assert frames.shape == (FRAMES_PER_CALL, H, W, 3), frames.shape
    if kind == "own":
        m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
        got = F.jpeg_frames(*m.encode_jpeg_tensor(torch.from_numpy(frames.astype(np.float32)).cuda(), jpeg_quality=QUALITY, jpeg_chroma="420"))
        m.close()
        return got
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(buf, "JPEG", quality=QUALITY, subsampling=2, **({"restart_marker_rows": 1} if kind == "pillow_rows" else {}))
        out.append(buf.getvalue())
    return out


def leg_trace(pkg, case, repeats):
    import torch
    kind, size = case.rsplit("@", 1)
    H, W = SIZES[size]
    pkg.Stylization      # (loads the framework module)
    streams = _streams(pkg, kind, H, W)
    info = sys.modules[pkg.__name__ + ".framework"].jpeg_info(streams[0])
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    for _ in range(repeats + 1):
        planes, layout = m.decode_jpeg_tensor(streams)
        torch.cuda.synchronize()
    m.close()
    return {"case": case, "calls": repeats + 1, "layout": layout, "intervals": info["intervals"], "blocks": info["blocks"],
            "stream_bytes": int(np.mean([len(s) for s in streams])), "scan_bytes": int(np.mean([len(s) for s in streams])) - info["scan_offset"]}


def leg_host_in(pkg, mode, n, repeats):
    """frames/s host -> host of transfer_batch over n 512 x 512 frames per call: mode "u8_u8" uint8 BGR in and out, "jpeg_u8" JPEG streams in (Pillow,
    quality 90, 4:2:0, one restart interval per MCU row) and uint8 out, "jpeg_jpeg" the same streams in and JPEG out"""
    import time
    m = DR._model(pkg, 512, 512)
    if mode == "u8_u8":
        src = pkg.pinned_empty((n, 512, 512, 3), np.uint8)
        src[...] = np.stack([pkg.synth_frame(i % 16, 512, 512, kind="smooth") for i in range(n)])
        kw = dict(out=pkg.pinned_empty((n, 512, 512, 3), np.uint8))
    else:
        base = _streams(pkg, "pillow_rows", 512, 512)
        src = [base[i % len(base)] for i in range(n)]
        kw = dict(in_format="jpeg", out_format="jpeg", jpeg_quality=QUALITY) if mode == "jpeg_jpeg" else dict(in_format="jpeg", out=pkg.pinned_empty((n, 512, 512, 3), np.uint8))
    rates = []
    for k in range(repeats + 1):            # call 0 warms up
        t0 = time.perf_counter()
        m.transfer_batch(src, **kw)
        if k:
            rates.append(n / (time.perf_counter() - t0))
    m.close()
    return dict(DR._stat(rates, 1), unit="frames/s host -> host", frames_per_call=n, mode=mode)


XFER_CASES = {"512": ((512, 512), None), "2160_at_1080": ((2160, 3840), (1080, 1920))}      # (source frame, working frame or None)


def leg_xfer(pkg, case, repeats):
    """the work a profiler run traces for a transfer leg: 1 + repeats calls of transfer_frames(in_format="jpeg") over 16 Pillow streams with one
    restart interval per MCU row, uint8 out; "2160_at_1080": worked on at 1920 x 1080 and delivered at the source's size"""
    (SH, SW), work = XFER_CASES[case]
    pkg.Stylization
    streams = _streams(pkg, "pillow_rows", SH, SW)
    m = DR._model(pkg, *(work or (SH, SW)))
    kw = dict(work_size=work, out_size="source") if work else {}
    for _ in range(repeats + 1):
        m.transfer_frames(streams, in_format="jpeg", dtype=np.uint8, **kw)
    m.close()
    return {"case": case, "calls": repeats + 1, "stream_bytes": int(np.mean([len(s) for s in streams]))}


def parse_xfer_trace(path):
    """per call {kernel: ms} of a traced transfer leg: a call starts at its jpeg_marks_k; the first call is the warm-up"""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    starts = [i for i, r in enumerate(rows) if "jpeg_marks_k" in r[0]]
    if len(starts) < 3:
        raise ValueError("%s holds %d calls" % (path, len(starts)))
    calls = []
    for a, b in zip(starts[1:], starts[2:] + [len(rows)]):
        seg = rows[a:b]
        c = {k: sum((e - s) / 1e6 for n, s, e in seg if k in n) for k in STAGE + ("conv_first_k",)}
        c["all_kernels"] = sum((e - s) / 1e6 for _, s, e in seg)
        calls.append(c)
    return calls


def xfer_leg(case, a):
    out_dir = tempfile.mkdtemp(prefix="jpeg_in_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "leg", "--",
           sys.executable, os.path.abspath(__file__), "--leg", "xfer:" + case, "--repeats", str(a.kernel_repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    print("transfer leg %s under rocprofv3" % case, file=sys.stderr, flush=True)
    try:
        leg = json.loads([ln for ln in DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().splitlines() if ln.startswith("{")][-1])
        traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise ValueError("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
        calls = parse_xfer_trace(traces[0])
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    (SH, SW), work = XFER_CASES[case]
    res = dict(leg, source=[SH, SW], work_size=list(work or (SH, SW)), frames_per_call=FRAMES_PER_CALL, calls=len(calls))
    for k in STAGE + ("conv_first_k", "all_kernels"):
        res[k + "_ms"] = DR._stat([c[k] for c in calls], 4)
    res["stage_ms"] = DR._stat([sum(c[k] for k in STAGE) for c in calls], 4)
    res["stage_share_of_all_kernels"] = round(res["stage_ms"]["median"] / res["all_kernels_ms"]["median"], 4)
    return res


def leg_driver(pkg, mode, n):
    """frames/s file -> file of the driver over n 512 x 512 frames into an .avi encoded on the GPU, no frame files: "jpg_pillow" .jpg files decoded by
    Pillow on the worker threads, "jpg_gpu" the same files with gpu_decode, "avi_avi" the same streams as the chunks of an MJPG .avi"""
    import importlib
    from PIL import Image
    D = importlib.import_module("rerevst-code_amd.driver")
    pkg.Stylization
    tmp = tempfile.mkdtemp(prefix="jpeg_in_rate_driver_")
    try:
        base = _streams(pkg, "pillow_rows", 512, 512)
        streams = [base[i % len(base)] for i in range(n)]
        paths = []
        for i, data in enumerate(streams):
            paths.append(os.path.join(tmp, "f%05d.jpg" % i))
            with open(paths[-1], "wb") as f:
                f.write(data)
        Image.fromarray(pkg.synth_style(512, 512, kind="noise", seed=7)[..., ::-1].copy()).save(os.path.join(tmp, "style.png"))
        stats = {}
        model = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
        kw = dict(gpu_jpeg=dict(quality=95, chroma="420"))
        if mode == "jpg_gpu":
            kw["gpu_decode"] = True
        elif mode == "avi_avi":
            kw.update(gpu_decode=True, frame_data=streams)
        for _ in range(2):      # the first run warms up (workspaces, staging, the page cache)
            D.stylize_files(model, os.path.join(tmp, "style.png"), paths, os.path.join(tmp, "out"), os.path.join(tmp, "v.avi"), 24, stats=stats, write_frames=False,
                            log=lambda *a, **k: None, **kw)
        model.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {"frames_per_s": round(stats["frames_per_s"], 1), "unit": "frames/s file -> file", "frames": n, "gpu_call_s": round(stats["gpu_call_s"], 3),
            "prep_s": round(stats["prep_s"], 3), "io_threads": stats["io_threads"], "mode": mode}


def parse_trace(path):
    """per call {kernel: ms} of a rocprofv3 kernel trace: a call ends with its jpeg_planes_k; the first call is the warm-up"""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    first = next((i for i, r in enumerate(rows) if "jpeg_marks_k" in r[0]), None)
    if first is None:
        raise ValueError("%s holds no jpeg_marks_k" % path)
    calls, cur = [], {}
    for name, s, e in rows[first:]:
        key = next((k for k in STAGE if k in name), None)
        if key:
            cur[key] = cur.get(key, 0.0) + (e - s) / 1e6
            if key == "jpeg_planes_k":
                calls.append(cur)
                cur = {}
    if len(calls) < 2:
        raise ValueError("%s holds %d calls" % (path, len(calls)))
    return calls[1:]


def kernel_leg(case, a):
    out_dir = tempfile.mkdtemp(prefix="jpeg_in_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "leg", "--",
           sys.executable, os.path.abspath(__file__), "--leg", "trace:" + case, "--repeats", str(a.kernel_repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    print("kernel leg %s under rocprofv3" % case, file=sys.stderr, flush=True)
    try:
        leg = json.loads([ln for ln in DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().splitlines() if ln.startswith("{")][-1])
        traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise ValueError("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
        calls = parse_trace(traces[0])
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    H, W = SIZES[case.rsplit("@", 1)[1]]
    res = dict(leg, size=[H, W], quality=QUALITY, chroma="420", frames_per_call=FRAMES_PER_CALL, calls=len(calls))
    for k in STAGE:
        res[k + "_ms"] = DR._stat([c.get(k, 0.0) for c in calls], 4)
    res["stage_ms"] = DR._stat([sum(c.get(k, 0.0) for k in STAGE) for c in calls], 4)
    # bytes per call: the markers' search and the decode each read the scan once (the decode also stores the non-zero coefficients: not
    # counted); the planes read 128 bytes per block and write 1.5 bytes per pixel
    moved = {"jpeg_marks_k": leg["scan_bytes"] if leg["intervals"] > 1 else 0, "jpeg_huff_k": leg["scan_bytes"], "jpeg_planes_k": 128 * leg["blocks"] + H * W * 3 // 2}
    for k in STAGE:
        t = res[k + "_ms"]["median"] * 1e-3
        res[k + "_bytes_per_call"] = moved[k] * FRAMES_PER_CALL
        res[k + "_gbytes_per_s"] = round(moved[k] * FRAMES_PER_CALL / t / 1e9, 3) if t > 0 else 0.0
        res[k + "_share_of_hbm_peak"] = float("%.3g" % (moved[k] * FRAMES_PER_CALL / DR.PEAK_BYTES_S / t)) if t > 0 else 0.0
    return res


def _child(lib, leg, a, frames):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames), "--repeats", str(a.repeats)]
    env = dict(os.environ)
    env.pop("RRV_LIB_PATH", None)
    if lib:
        env["RRV_LIB_PATH"] = os.path.abspath(lib)
    print("leg %s on %s" % (leg, lib or "this tree's library"), file=sys.stderr, flush=True)
    return json.loads(DR._run(cmd, env, a.leg_timeout, subprocess.PIPE).decode().strip().splitlines()[-1])


def measure(a, res, save):
    if not a.skip_kernel_legs:
        for case in XFER_CASES:
            res["transfer_" + case] = "not measured (rocprofv3 not found)" if shutil.which("rocprofv3") is None else xfer_leg(case, a)
            save()
    if not a.skip_host_legs:
        for mode in ("jpg_pillow", "jpg_gpu", "avi_avi"):
            res["driver_" + mode] = _child(None, "driver:" + mode, a, a.driver_frames)
            save()
    if not a.skip_kernel_legs:
        for size in a.sizes.split(","):
            for kind in KINDS:
                case = kind + "@" + size
                res["kernel_" + case] = "not measured (rocprofv3 not found)" if shutil.which("rocprofv3") is None else kernel_leg(case, a)
                save()
    if a.skip_host_legs:
        return
    for mode in ("u8_u8", "jpeg_u8", "jpeg_jpeg"):
        res["host_512_" + mode] = dict(_child(None, "host_in:" + mode, a, a.frames), library="this commit")
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
    if a.parent_lib:
        p, t = res["host_plain_512_parent"], res["host_plain_512"]
        spread = p["max"] - p["min"]
        res["plain_path_vs_parent"] = {"parent_median": p["median"], "parent_spread": round(spread, 1), "this_median": t["median"], "this_spread": round(t["max"] - t["min"], 1),
                                       "ratio": round(t["median"] / p["median"], 4), "inside_parent_spread": t["median"] >= p["median"] - spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300, help="frames per call of the plain host leg")
    ap.add_argument("--driver-frames", type=int, default=192, help=".jpg files / AVI chunks of the driver legs")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-repeats", type=int, default=5)
    ap.add_argument("--sizes", type=str, default="512,2160")
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", type=str, default=None, help="librerevst_hip.so built from the parent commit: the plain host leg is measured on it too")
    ap.add_argument("--skip-kernel-legs", action="store_true")
    ap.add_argument("--skip-host-legs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--leg", type=str, default=None, help="trace:<kind>@<size> or dr_host:plain")
    a = ap.parse_args()
    if a.leg:
        pkg = DR._load_pkg()
        kind, what = a.leg.split(":", 1)
        pkg.Stylization      # (loads the framework module)
        if kind == "trace":
            res = leg_trace(pkg, what, a.repeats)
        elif kind == "xfer":
            res = leg_xfer(pkg, what, a.repeats)
        elif kind == "driver":
            res = leg_driver(pkg, what, a.frames)
        elif kind == "host_in":
            res = leg_host_in(pkg, what, a.frames, a.repeats)
        else:
            res = DR.leg_host(pkg, what, a.frames, a.repeats)
        print(json.dumps(res))
        return
    res = {"kernel_legs": "16 frames per call through decode_jpeg_tensor, quality %d, 4:2:0; rocprofv3 --kernel-trace --stats, one run per leg; ms per call, medians over %d "
                          "calls after a warm-up call" % (QUALITY, a.kernel_repeats),
           "host_legs": "%d frames per call at 512 x 512 (uint8 BGR in and out), page-locked input, profiler off, %d repeats" % (a.frames, a.repeats),
           "transfer_legs": "16 frames per call through transfer_frames(in_format=\"jpeg\"), uint8 out, Pillow streams with one restart interval per MCU row; one "
                            "rocprofv3 run per leg; the stage's kernels, conv_first_k and the sum of all kernels of the call, ms per call",
           "driver_legs": "%d frames of 512 x 512 into an .avi encoded on the GPU (quality 95), no frame files, second of two runs" % a.driver_frames}

    def save():      # what is measured so far: a run cut short still leaves its legs
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    failed = None
    try:
        measure(a, res, save)
    except (subprocess.SubprocessError, ValueError, KeyError, IndexError) as e:      # a leg failed, faulted or hung, or left no usable trace: nothing more is started
        failed = "%s: %s" % (type(e).__name__, str(e)[:300])
        res["stopped"] = "a leg did not complete (%s); the legs after it were not run" % failed
    for k in ["transfer_" + c for c in XFER_CASES] + ["driver_jpg_pillow", "driver_jpg_gpu", "driver_avi_avi"] + ["kernel_%s@%s" % (kind, size) for size in a.sizes.split(",") for kind in KINDS] + ["host_plain_512", "host_plain_512_parent", "host_512_u8_u8", "host_512_jpeg_u8", "host_512_jpeg_jpeg"]:
        res.setdefault(k, "not measured")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if failed:
        sys.exit("jpeg_in_rate: " + failed)
    held = res.get("plain_path_vs_parent")
    if isinstance(held, dict) and not held["inside_parent_spread"]:      # the one condition of the measurement
        sys.exit("jpeg_in_rate: the plain 512 x 512 call fell below the parent's median by more than the parent's own spread (ratio %.4f)" % held["ratio"])


if __name__ == "__main__":
    main()

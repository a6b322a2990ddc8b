#!/usr/bin/env python
"""Per-kernel breakdown of Stylization(use_Global=False).transfer at 512x512 (padded 640x640), one frame per call:
HIP-event time per launch group inside the library + wall time per call.  Prints one JSON object.

--batch S [S ...]: the batched frame-mode entries at each frame size S (padded to V.padded_size(S)), one JSON line per size:
frames/s of transfer (one frame per call), transfer_batch (padded frames) and transfer_frames (unpadded, pad / crop on the
device), measured in the same process, host buffers to host buffers; launches per frame and the per-kernel table of one
16-frame transfer_batch.  --driver N: also time driver.stylize_files on N PNG frames of the first size (the --no-global flow)."""
import importlib, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("rerevst-code_amd")
V = importlib.import_module("rerevst-code_amd.video")


def table(rows):
    agg = {}
    for name, ms, fl, by, fx in rows:
        k = name.split("@")[0]
        a = agg.setdefault(k, [0, 0.0])
        a[0] += 1; a[1] += ms
    return agg, [{"kernel": k, "launches": a[0], "ms": round(a[1], 4)} for k, a in sorted(agg.items(), key=lambda kv: -kv[1][1])]


def rate(fn, frames_per_call, n):
    fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return round(n * frames_per_call / (time.perf_counter() - t0), 1)


def one_frame(S):
    P = V.padded_size(S)
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True, use_Global=False)
    m.prepare_style(pkg.synth_style(512, 512, kind="noise", seed=7))
    frames = [V.reflect_pad(pkg.synth_frame(i, S, S, kind="noise"), P, P) for i in range(4)]
    for f in frames[:2]:
        m.transfer(f)
    t0 = time.perf_counter()
    n = 24
    for i in range(n):
        m.transfer(frames[i % 4])
    wall = (time.perf_counter() - t0) / n
    m.profile_begin()
    m.transfer(frames[0])
    rows = m.profile_end()
    agg, kernels = table(rows)
    print(json.dumps({"size": S, "wall_ms_per_frame": round(wall * 1e3, 3), "frames_per_s": round(1 / wall, 1), "launches_profiled": len(rows),
                      "event_ms_total": round(sum(a[1] for a in agg.values()), 3), "kernels": kernels}))


def batched(S, n_driver):
    P = V.padded_size(S)
    B = 64 if S <= 512 else 32
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True, use_Global=False)
    m.prepare_style(pkg.synth_style(512, 512, kind="noise", seed=7))
    raw = np.stack([pkg.synth_frame(i, S, S, kind="noise") for i in range(B)])
    padded = np.stack([V.reflect_pad(f, P, P) for f in raw])
    out_b = pkg.pinned_empty((B, P, P, 3))
    out_f = pkg.pinned_empty((B, S, S, 3))
    res = {"size": S, "padded": P, "frames_per_call": B}
    res["one_frame_per_call_fps"] = rate(lambda: [m.transfer(padded[i]) for i in range(8)], 8, 4)
    res["transfer_batch_fps"] = rate(lambda: m.transfer_batch(padded, out=out_b), B, 4)
    res["transfer_frames_fps"] = rate(lambda: m.transfer_frames(raw, out=out_f), B, 4)
    res["speedup_batch_vs_one_frame"] = round(res["transfer_batch_fps"] / res["one_frame_per_call_fps"], 2)
    m.profile_begin()
    m.transfer_batch(padded[:16])
    rows = m.profile_end()
    agg, kernels = table(rows)
    res["launches_per_16_frames"] = len(rows)
    res["launches_per_frame"] = round(len(rows) / 16, 2)
    res["event_ms_per_frame"] = round(sum(a[1] for a in agg.values()) / 16, 4)
    res["kernels_16_frames"] = kernels
    m.profile_begin()
    m.transfer(padded[0])
    res["launches_one_frame_entry"] = len(m.profile_end())
    if n_driver:
        D = importlib.import_module("rerevst-code_amd.driver")
        with tempfile.TemporaryDirectory() as d:
            for i in range(n_driver):
                D.write_image_bgr(os.path.join(d, "f%04d.png" % i), raw[i % B])
            D.write_image_bgr(os.path.join(d, "style.png"), pkg.synth_style(512, 512, kind="noise", seed=7))
            paths = D.list_frames(os.path.join(d, "f*.png"))
            stats = {}
            D.stylize_files(m, os.path.join(d, "style.png"), paths, os.path.join(d, "out"), log=lambda *_: None, stats=stats)
            stats = {}
            t0 = time.perf_counter()
            D.stylize_files(m, os.path.join(d, "style.png"), paths, os.path.join(d, "out"), log=lambda *_: None, stats=stats)
            res["driver_no_global_frames"] = n_driver
            res["driver_no_global_fps_wall"] = round(n_driver / (time.perf_counter() - t0), 1)
            res["driver_no_global_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items()}
    m.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--batch":
        n_driver = 0
        if "--driver" in args:
            i = args.index("--driver")
            n_driver = int(args[i + 1])
            del args[i:i + 2]
        sizes = [int(a) for a in args[1:]] or [512, 1024]
        for k, S in enumerate(sizes):
            batched(S, n_driver if k == 0 else 0)
    else:
        one_frame(int(args[0]) if args else 512)

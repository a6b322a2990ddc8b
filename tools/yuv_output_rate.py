#!/usr/bin/env python
"""float32, uint8 BGR, I420 and NV12 output of transfer_frames side by side, where the output's bytes cross PCIe: host -> host
staged (host_io 0) and zero copy (host_io 1), page-locked buffers, the four formats taking turns round by round in one process;
conv_last_k's event time per launch (rrv_profile_*, 16 frames per launch, device-resident: rrv_transfer_image_device with the four
output descriptors); and the driver on the same PNG frames, PNG output against --no-frames --video out.y4m.
    python tools/yuv_output_rate.py [--sizes 512,1024] [--rounds 5] [--out profiles/yuv_output.json]
Prints one JSON object and, with --out, writes it there."""
import argparse
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = ("float32", "uint8", "i420", "nv12")


def _stat(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def _alternate(rounds, run):
    """run(format) -> figure; one warm-up call of each format, then `rounds` of each, the order reversed every other round"""
    for f in FORMATS:
        run(f)
    got = {f: [] for f in FORMATS}
    for k in range(rounds):
        for f in (FORMATS if k % 2 == 0 else FORMATS[::-1]):
            got[f].append(run(f))
    return got


def _size_legs(pkg, m, S, B, rounds):
    import torch
    legs = {}
    frames = np.stack([pkg.synth_frame(i, S, S, kind="noise") for i in range(B)])
    pin_in = pkg.pinned_empty(frames.shape, np.uint8)
    pin_in[...] = frames
    fb = pkg.yuv_frame_bytes(S, S)
    outs = {"float32": pkg.pinned_empty(frames.shape, np.float32), "uint8": pkg.pinned_empty(frames.shape, np.uint8),
            "i420": pkg.pinned_empty((B, fb), np.uint8), "nv12": pkg.pinned_empty((B, fb), np.uint8)}
    for io, name in ((0, "staged"), (1, "zero_copy")):
        def call(f, io=io):
            m.set_host_io(io)
            t0 = time.perf_counter()
            if f in ("i420", "nv12"):
                m.transfer_frames(pin_in, out=outs[f], out_format=f)
            else:
                m.transfer_frames(pin_in, out=outs[f])
            r = B / (time.perf_counter() - t0)
            m.set_host_io(0)
            return r
        got = _alternate(rounds, call)
        leg = {f: _stat(v) for f, v in got.items()}
        for f in ("i420", "nv12"):
            leg[f + "_over_uint8"] = round(leg[f]["median"] / leg["uint8"]["median"], 3)
        leg["uint8_spread"] = round((leg["uint8"]["max"] - leg["uint8"]["min"]) / leg["uint8"]["median"], 3)
        legs["transfer_frames_frames_per_s_" + name] = leg
    # conv_last_k alone: HIP events around its launch, 16 frames per launch, device-resident
    L = importlib.import_module("rerevst-code_amd._lib")
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames[:16]).to(dev)
    d_out = torch.empty(16 * S * S * 3 * 4, dtype=torch.uint8, device=dev)
    u8 = L.ImageDesc(L.DT_U8, L.LAY_HWC_BGR, L.SP_PIXEL)
    desc = {"float32": L.ImageDesc(L.DT_F32, L.LAY_HWC_BGR, L.SP_PIXEL), "uint8": u8,
            "i420": L.ImageDesc(L.DT_U8, L.LAY_I420, L.SP_PIXEL), "nv12": L.ImageDesc(L.DT_U8, L.LAY_NV12, L.SP_PIXEL)}

    def last_ms(f):
        import ctypes as C
        m.profile_begin()
        m._chk(m._lib.rrv_transfer_image_device(m._h, C.c_void_p(d_in.data_ptr()), u8, 16, S, S, C.c_void_p(d_out.data_ptr()), desc[f], L.TF_PAD_CROP, None))
        return sum(r[1] for r in m.profile_end() if r[0] == "conv_last")
    legs["conv_last_k_ms_16_frames"] = {f: _stat(v, 4) for f, v in _alternate(rounds, last_ms).items()}
    return legs


def _driver_leg(pkg, m, S, n, rounds, threads):
    D = importlib.import_module("rerevst-code_amd.driver")
    tmp = tempfile.mkdtemp(prefix="yuv_rate_")
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        for i in range(n):
            D.write_image_bgr(os.path.join(src, "f%04d.png" % i), pkg.synth_frame(i % 16, S, S, kind="noise"))
        D.write_image_bgr(os.path.join(tmp, "style.png"), pkg.synth_style(512, 512, kind="noise", seed=7))
        paths = D.list_frames(os.path.join(src, "*.png"))
        rates = {"png": [], "y4m_no_frames": []}
        last = {}
        for k in range(rounds + 1):          # round 0 warms up
            for name in rates:
                st = {}
                kw = dict(video_path=os.path.join(tmp, "out.y4m"), write_frames=False) if name == "y4m_no_frames" else {}
                D.stylize_files(m, os.path.join(tmp, "style.png"), paths, os.path.join(tmp, "out"), io_threads=threads, log=lambda *_: None, stats=st, **kw)
                if k:
                    rates[name].append(st["frames_per_s"])
                    last[name] = {a: (round(b, 4) if isinstance(b, float) else b) for a, b in st.items()}
        res = {name: dict(_stat(v), stats_last=last[name]) for name, v in rates.items()}
        res["y4m_over_png"] = round(res["y4m_no_frames"]["median"] / res["png"]["median"], 3)
        res.update(size=S, frames=n, io_threads=threads)
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="512,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--driver-frames", type=int, default=128)
    ap.add_argument("--driver-rounds", type=int, default=2)
    ap.add_argument("--io-threads", type=int, default=16)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("rerevst-code_amd")
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    m.prepare_style(pkg.synth_style(512, 512, kind="noise", seed=7))
    m.clean()
    for i in (0, 8, 16):
        m.add(pkg.synth_frame(i, 512, 512, kind="noise"))
    m.compute()
    res = {"rounds": a.rounds, "sizes": {}}
    for S in [int(s) for s in a.sizes.split(",")]:
        B = 32 if S <= 512 else 16
        res["sizes"][str(S)] = dict(frames_per_call=B, **_size_legs(pkg, m, S, B, a.rounds))
    res["driver_512"] = _driver_leg(pkg, m, 512, a.driver_frames, a.driver_rounds, a.io_threads)
    m.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""float32 against uint8 output (the rrv_*_u8 twins) on the legs where the output's bytes cross PCIe or sit in page-locked
memory: blocking transfer() one frame per call, tickets with three ahead, transfer_batch host -> host (staged, host_io=1 and 3),
transfer_frames, conv_last_k's event time (rrv_profile_*, 16 frames per launch), and one driver PNG -> PNG run per format.
Every shape is warmed up first; the two formats alternate round by round in one process.
    python tools/u8_output_rate.py [--sizes 512,1024] [--rounds 5]
Prints one JSON object (commit it under profiles/)."""
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

DTYPES = (("float32", np.float32), ("uint8", np.uint8))


def _summary(rates):
    out = {}
    for name, _ in DTYPES:
        r = rates[name]
        out[name] = {"median": round(statistics.median(r), 1), "min": round(min(r), 1), "max": round(max(r), 1)}
    out["uint8_over_float32"] = round(out["uint8"]["median"] / out["float32"]["median"], 3)
    return out


def _alternate(rounds, run):
    """run(dtype) -> rate; float32 and uint8 alternate, `rounds` of each after one warm-up call of each"""
    for _, dt in DTYPES:
        run(dt)
    rates = {name: [] for name, _ in DTYPES}
    for k in range(rounds):
        for name, dt in (DTYPES if k % 2 == 0 else DTYPES[::-1]):
            rates[name].append(run(dt))
    return _summary(rates)


def _size_legs(pkg, m, S, B, rounds):
    import torch
    legs = {}
    frames = np.stack([pkg.synth_frame(i, S, S, kind="noise") for i in range(B)])
    pin_in = pkg.pinned_empty(frames.shape, np.uint8)
    pin_in[...] = frames
    nf = 32 if S <= 512 else 12

    def one_per_call(dt):
        t0 = time.perf_counter()
        for i in range(nf):
            m.transfer(pin_in[i % B], dtype=dt)
        return nf / (time.perf_counter() - t0)
    legs["transfer_one_frame_per_call"] = _alternate(rounds, one_per_call)

    def tickets(dt):
        t0 = time.perf_counter()
        open_ = []
        for i in range(nf):
            open_.append(m.transfer_async(pin_in[i % B], dtype=dt))
            if len(open_) > 3:
                m.result(open_.pop(0))
        for t in open_:
            m.result(t)
        return nf / (time.perf_counter() - t0)
    legs["tickets_three_ahead"] = _alternate(rounds, tickets)

    outs = {name: pkg.pinned_empty(frames.shape, dt) for name, dt in DTYPES}
    for io in (0, 1, 3):          # staged; zero copy both ways; zero copy output only (the last kernel stores into page-locked memory)
        def batch(dt, io=io):
            m.set_host_io(io)
            t0 = time.perf_counter()
            m.transfer_batch(pin_in, out=outs[np.dtype(dt).name])
            r = B / (time.perf_counter() - t0)
            m.set_host_io(0)
            return r
        legs["transfer_batch_host_io_%d" % io] = _alternate(rounds, batch)

    def frames_entry(dt):
        t0 = time.perf_counter()
        m.transfer_frames(pin_in, out=outs[np.dtype(dt).name])
        return B / (time.perf_counter() - t0)
    legs["transfer_frames"] = _alternate(rounds, frames_entry)

    # conv_last_k alone: HIP events around its launch, 16 frames per launch, device-resident
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(frames[:16]).to(dev)
    d_out = {name: torch.empty((16, S, S, 3), dtype=torch.float32 if name == "float32" else torch.uint8, device=dev) for name, _ in DTYPES}
    ms = {name: [] for name, _ in DTYPES}
    for k in range(rounds + 1):
        for name, dt in DTYPES:
            m.profile_begin()
            m.transfer_batch_device(d_in.data_ptr(), 16, S, S, d_out[name].data_ptr(), dtype=dt)
            rows = m.profile_end()
            if k:
                ms[name].append(sum(r[1] for r in rows if r[0] == "conv_last"))
    legs["conv_last_k_ms_16_frames"] = {name: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                        for name, v in ms.items()}
    return legs


def _driver_leg(pkg, m, S, n, rounds, threads):
    D = importlib.import_module("rerevst-code_amd.driver")
    tmp = tempfile.mkdtemp(prefix="u8_rate_")
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        for i in range(n):
            D.write_image_bgr(os.path.join(src, "f%04d.png" % i), pkg.synth_frame(i % 16, S, S, kind="noise"))
        D.write_image_bgr(os.path.join(tmp, "style.png"), pkg.synth_style(512, 512, kind="noise", seed=7))
        paths = D.list_frames(os.path.join(src, "*.png"))
        stats = {name: [] for name, _ in DTYPES}

        def run(dt):
            m.uint8_output = dt == np.uint8          # the driver's capability check: False = the float path it takes for other models
            st = {}
            D.stylize_files(m, os.path.join(tmp, "style.png"), paths, os.path.join(tmp, "out"), io_threads=threads, log=lambda *_: None, stats=st)
            del m.uint8_output
            stats[np.dtype(dt).name].append(st)
            return st["frames_per_s"]
        res = _alternate(rounds, run)
        for name, _ in DTYPES:
            res[name]["stats_last"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats[name][-1].items()}
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
    res["driver_png_to_png"] = _driver_leg(pkg, m, 512, a.driver_frames, a.driver_rounds, a.io_threads)
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

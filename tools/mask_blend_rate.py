#!/usr/bin/env python
"""Per-pixel multi-style blending, frames/s on device tensors at 512 x 512 frames (padded 640 x 640 on the device), sixteen frames
per call, with S = 2 and S = 4 styles; every entry through transfer_tensor(pad_crop=True) on torch's current stream:
  masked       style_masks = a [B][S][H][W] device tensor                           (rrv_transfer_image_mask_device)
  frame_mode   the batched frame-mode entry on a use_Global=False handle            (rrv_transfer_image_device, RRV_TF_FRAME_MODE)
  blend        style_weights = a [B][S] device tensor: one weight vector per frame  (rrv_transfer_image_blend_device)
  composite    what the masked entry replaces: S plain passes, one per style (set_state of style s into a one-style handle
               each), and a torch composite sum_s mask_s * out_s
One process, every leg warmed up first, the legs alternate round by round, each timed over `calls` calls between two device
synchronisations (wall clock), medians.  Launches per frame of the masked entry from the library's own launch log.
    python tools/mask_blend_rate.py [--rounds 5] [--calls 4] [--out profiles/mask_blend.json]
Prints one JSON object and writes it to --out."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, B, SMAX = 512, 16, 4


def _med(v, nd=1):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def _masks(S, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.stack([np.stack([1.2 + np.sin(yy / (17 + 5 * s + b) + s) * np.cos(xx / (23 + 3 * s + b) + b) for s in range(S)]) for b in range(B)])
    return (m / m.sum(axis=1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mask_blend.json"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("rerevst-code_amd")
    V = importlib.import_module("rerevst-code_amd.video")
    w = pkg.synthetic_weights(0)
    styles = [V.resize_bilinear(pkg.synth_style(512, 512, kind="noise", seed=7 + k), (384, 384)) for k in range(SMAX)]
    m = pkg.MultiStyleStylization(w, cuda=True, style_num=SMAX)
    m.prepare_style(styles)
    m.clean()
    for i in (0, 8, 16):
        m.add(V.reflect_pad(pkg.synth_frame(i, SIZE, SIZE, kind="noise"), 640, 640))
    m.compute()
    fm = pkg.Stylization(w, cuda=True, use_Global=False)
    fm.prepare_style(styles[0])
    singles = []
    for k in range(SMAX):
        s = pkg.Stylization(w, cuda=True)
        s.set_state(m.get_state(k))
        singles.append(s)
    dev = torch.device("cuda", m.device)
    x = torch.from_numpy(np.stack([pkg.synth_frame(i, SIZE, SIZE, kind="noise") for i in range(B)])).to(dev)
    res = {"frame": SIZE, "padded": V.padded_size(SIZE), "frames_per_call": B, "rounds": a.rounds, "calls_per_timing": a.calls, "styles": {}}
    for S in (2, 4):
        M = torch.from_numpy(_masks(S, SIZE, SIZE)).to(dev)
        Wt = M.mean(dim=(2, 3)).contiguous()

        def masked():
            return m.transfer_tensor(x, layout="nhwc", pad_crop=True, style_masks=M)

        def frame_mode():
            return fm.transfer_tensor(x, layout="nhwc", pad_crop=True)

        def blend():
            return m.transfer_tensor(x, layout="nhwc", pad_crop=True, style_weights=Wt)

        def composite():
            acc = None
            for k in range(S):
                o = singles[k].transfer_tensor(x, layout="nhwc", pad_crop=True) * M[:, k, :, :, None]
                acc = o if acc is None else acc + o
            return acc

        legs = (("masked", masked), ("frame_mode", frame_mode), ("blend", blend), ("composite", composite))
        rates = {name: [] for name, _ in legs}
        for k in range(a.rounds + 1):                       # round 0 warms every leg up
            for name, fn in (legs if k % 2 else legs[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                if k:
                    rates[name].append(a.calls * B / (time.perf_counter() - t0))
        r = {"frames_per_s": {name: _med(v) for name, v in rates.items()}}
        med = {name: r["frames_per_s"][name]["median"] for name in rates}
        r["masked_over_frame_mode"] = round(med["masked"] / med["frame_mode"], 3)
        r["masked_over_blend"] = round(med["masked"] / med["blend"], 3)
        r["masked_over_composite"] = round(med["masked"] / med["composite"], 3)
        torch.cuda.synchronize()
        m.profile_begin()
        masked()
        log = m.profile_end()
        r["masked_launches_per_call"] = len(log)
        r["masked_launches_per_frame"] = round(len(log) / B, 2)
        by = {}
        for name, ms, *_ in log:
            key = name.split("@")[0]
            by[key] = round(by.get(key, 0.0) + ms, 3)
        r["masked_ms_per_call_by_kernel"] = dict(sorted(by.items(), key=lambda kv: -kv[1]))
        res["styles"][str(S)] = r
    for s in [m, fm] + singles:
        s.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

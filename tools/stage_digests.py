#!/usr/bin/env python
"""Do two builds of the library give the frame stages' outputs the same bits?
    RRV_LIB_PATH=OLD/librerevst_hip.so python tools/stage_digests.py > old.txt;  python tools/stage_digests.py > new.txt;  diff old.txt new.txt
Prints one line per case: name, SHA-256 of the output bytes, dtype, shape.  Needs an MI355X; run once per library, a process each
(RRV_LIB_PATH names the library, which finds its companion libraries beside itself).  Inputs are seeded noise.
  resample  rrv_resample_view_device (resample_tensor): the eight input forms
  deliver   rrv_deliver_view_device (deliver_tensor): the six output forms, the YUV ones planar and semi-planar at 4:2:0, 4:2:2 and 4:4:4
each at five sizes: 3 x 3 tiles ragged on both edges, downscale by 8 (a tile's vertical taps span RS_ROWS_MAX rows), upscale by 8, a
single-pixel source, and identity axes; then three frames per call, a pitched view on either side, and two guided cases
(rrv_deliver_guided_view_device) whose apply kernel runs tiles of 64 and of 32 columns."""
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (source, destination)
SIZES = {"edge_tiles": ((37, 150), (45, 131)), "down8": ((280, 1048), (35, 131)), "up8": ((5, 9), (40, 72)), "smallest": ((1, 1), (8, 8)),
         "identity": ((33, 70), (33, 70))}
IN_FORMS = ("u8_nhwc", "u8_nchw", "f32_nhwc", "f32_nchw", "i420", "nv12", "i420p10", "p010")
YUV_FORMATS = {}      # the package's table, filled in by main()
OUT_FORMS = ("f32_nhwc", "f32_nchw", "u8_nhwc", "u8_nchw", "i420", "nv12", "i422", "nv16", "i444", "nv24", "i420p10", "p010", "i422p10", "p210", "i444p10", "p410")


def guided_tw(L, H, W, DH, DW, r):
    v = [C.c_int() for _ in range(5)]
    assert L.rrv_guided_tile(H, W, DH, DW, r, *[C.byref(x) for x in v]) == 0
    return v[0].value


def line(name, t):
    a = t.detach().cpu().contiguous().numpy()
    print("%-34s %s %s %s" % (name, hashlib.sha256(a.tobytes()).hexdigest(), a.dtype, "x".join(str(n) for n in a.shape)), flush=True)


def source(pkg, rng, form, B, H, W):
    """(tensor, resample_tensor's keywords) of B seeded frames of H x W in an input form"""
    import torch
    if form in YUV_FORMATS:
        f = YUV_FORMATS[form]
        a = rng.integers(0, 1 << f.bits, (B, pkg.yuv_frame_bytes(H, W, chroma=f.chroma)), dtype=np.uint16)
        a = a.astype(np.uint8) if f.bits == 8 else (a if f.planar else a << (16 - f.bits)).view(np.int16)      # (int16: the same bits, for a torch without uint16)
        if min(H, W) >= 8:
            return torch.from_numpy(a).cuda(), dict(layout=form, size=(H, W))
        # the tensor calls take YUV frames from 8 x 8 on: a smaller one goes in as a view of the same packed samples
        cw = W if f.chroma == "444" else (W + 1) // 2
        return pkg.ImageView(torch.from_numpy(a.reshape(-1)).cuda(), form, (H, W), [W, cw, cw] if f.planar else [W, 2 * cw], frame_stride=a.shape[1], frames=B), {}
    dt, layout = form.split("_")
    a = rng.integers(0, 256, (B, 3, H, W) if layout == "nchw" else (B, H, W, 3), dtype=np.uint8)
    if dt == "f32":
        a = (a + rng.uniform(-0.5, 0.5, a.shape)).astype(np.float32)
    return torch.from_numpy(a).cuda(), dict(layout=layout)


def frames(rng, B, H, W):
    """stylized working frames: float32 BGR PIXEL, a little beyond 0..255 so that the integer forms clamp"""
    import torch
    return torch.from_numpy(rng.uniform(-8.0, 263.0, (B, H, W, 3)).astype(np.float32)).cuda()


def out_kw(form):
    import torch
    if form in YUV_FORMATS:
        return dict(out_layout=form)
    dt, layout = form.split("_")
    return dict(out_layout=layout, out_dtype=torch.uint8 if dt == "u8" else torch.float32)


def main():
    import torch
    sys.path.insert(0, HERE)
    pkg = importlib.import_module("rerevst-code_amd")
    L = importlib.import_module("rerevst-code_amd._lib").load()
    YUV_FORMATS.update(importlib.import_module("rerevst-code_amd.video").YUV_FORMATS)
    m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
    rng = np.random.default_rng(20)
    for size, ((SH, SW), (DH, DW)) in SIZES.items():
        for form in IN_FORMS:
            x, kw = source(pkg, rng, form, 1, SH, SW)
            line("resample %s %s" % (size, form), m.resample_tensor(x, (DH, DW), **kw))
        y = frames(rng, 1, SH, SW)
        for form in OUT_FORMS:
            line("deliver %s %s" % (size, form), m.deliver_tensor(y, (DH, DW), **out_kw(form)))
    (SH, SW), (DH, DW) = SIZES["edge_tiles"]
    x, kw = source(pkg, rng, "nv12", 3, SH, SW)
    line("resample batch_of_3 nv12", m.resample_tensor(x, (DH, DW), **kw))
    line("deliver batch_of_3 nv12", m.deliver_tensor(frames(rng, 3, SH, SW), (DH, DW), out_layout="nv12"))
    # pitched views: rows 17 elements longer than the frame's, two frames a little more than a frame apart
    pitch, fs = SW * 3 + 17, (SW * 3 + 17) * SH + 29
    store = torch.from_numpy(rng.integers(0, 256, 2 * fs, dtype=np.uint8)).cuda()
    line("resample pitched u8_nhwc", m.resample_tensor(pkg.ImageView(store, "nhwc", (SH, SW), pitch, frame_stride=fs, frames=2), (DH, DW)))
    pitch, fs = DW + 17, (DW + 17) * DH * 3 + 29
    canvas = torch.full((2 * fs,), 7, dtype=torch.uint8).cuda()
    m.deliver_tensor(frames(rng, 2, SH, SW), (DH, DW), out=pkg.ImageView(canvas, "nchw", (DH, DW), pitch, frame_stride=fs, frames=2))
    line("deliver pitched u8_nchw", canvas)
    # guided: gf_apply_k on tiles of 64 columns, and (r = 16, where those no longer fit the LDS) of 32
    for name, (H, W), (GH, GW), r in (("guided tw64", (24, 40), (45, 131), 4), ("guided tw32_r16", (40, 72), (45, 80), 16)):
        P, lo, hi = frames(rng, 2, H, W), frames(rng, 2, H, W), frames(rng, 2, GH, GW)
        line("%s (tile %d)" % (name, guided_tw(L, H, W, GH, GW, r)), m.deliver_tensor(P, (GH, GW), guide_lo=lo, guide_hi=hi, guide_radius=r, guide_eps=1e-3))
    m.sync()
    m.close()


if __name__ == "__main__":
    main()

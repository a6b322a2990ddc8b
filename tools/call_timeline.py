#!/usr/bin/env python
"""Where a pipelined host call's time goes outside its kernels: the fill (call entry -> first kernel), when the last two
sub-batches finish, and the drain (last kernel end -> return), from the library's own RRV_TIMELINE events (no profiler: under
one the runtime copies with blit kernels, which changes what is measured).
    python tools/call_timeline.py [--reps 5] [--legs 512,256,ms4] [--rows]
Runs benchmark-shaped calls with page-locked caller arrays: 128 frames at 640 x 640 (the 512 x 512 configuration), 128 at
384 x 384 (256 x 256) and a config-5-shaped call (32 cached features at 1152 x 1152, four styles, groups of 4).  Prints one JSON
line per call and a median line per leg (commit the output under profiles/).  --rows adds the per-launch event times of one
profiled sub-batch in launch order, with their running sum: the half-way boundary of a launch sequence is read from it.
RRV_HOST_PHASE=0 RRV_HOST_PIECE=0 give host_pipeline without its tail wait and piecewise delivery (sub-batches finish in pairs, whole
copies); RRV_HOST_PIECE=n sets the piece size in 640 x 640 frames."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["RRV_TIMELINE"] = "1"      # read by rrv_create


class Stderr:
    """The library prints with fprintf(stderr): collect file descriptor 2 in a file while the calls run."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read()
        self.tmp.close()


def parse(text):
    calls = []
    for line in text.splitlines():
        if not line.startswith("rrv_timeline "):
            sys.stderr.write(line + "\n")
            continue
        tok = line.split()
        d = {"entry": tok[1]}
        for t in tok[2:]:
            k, v = t.split("=")
            d[k] = [float(x) for x in v.split(",")] if k in ("k_end", "d2h_end") else (v if k == "size" else float(v))
        last = max(d["k_end"])
        d["fill_ms"] = round(d["setup"] + d["first_kernel"], 3)
        d["drain_ms"] = round(d["wall"] - d["setup"] - last, 3)
        d["last_two_k_end_ms"] = sorted(d["k_end"])[-2:]
        d["idle_frac"] = round((d["fill_ms"] + d["drain_ms"]) / d["wall"], 4)
        calls.append(d)
    return calls


def report(leg, calls, warm):
    for c in calls[warm:]:
        print(json.dumps({"leg": leg, **c}))
    med = lambda k: round(statistics.median(c[k] for c in calls[warm:]), 3)
    gap = round(statistics.median(c["last_two_k_end_ms"][1] - c["last_two_k_end_ms"][0] for c in calls[warm:]), 3)
    print(json.dumps({"leg": leg, "median_of": len(calls) - warm, "wall_ms": med("wall"), "fill_ms": med("fill_ms"), "drain_ms": med("drain_ms"),
                      "last_two_sub_batches_finish_apart_ms": gap, "fill_plus_drain_frac_of_call": med("idle_frac")}), flush=True)


def rows_of_one_sequence(m, call, nseq, leg):
    m.profile_begin()
    call()
    rows = m.profile_end()
    n = len(rows) // nseq
    total, acc, out = sum(r[1] for r in rows[:n]), 0.0, []
    for name, ms, *_ in rows[:n]:
        acc += ms
        out.append([name, round(ms, 4), round(acc / total, 3)])
    print(json.dumps({"leg": leg, "one_sequence_ms": round(total, 3), "rows_name_ms_cumulative_frac": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", type=str, default="512,256,ms4")
    ap.add_argument("--rows", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("rerevst-code_amd")
    V = importlib.import_module("rerevst-code_amd.video")
    warm = 2
    print(json.dumps({"knobs": {k: os.environ.get(k) for k in ("RRV_HOST_PHASE", "RRV_HOST_PIECE", "RRV_LIB_PATH")}}), flush=True)
    for leg in a.legs.split(","):
        if leg == "ms4":
            S, NS, B, G = 1024, 4, 32, 4
            P = V.padded_size(S)
            m = pkg.MultiStyleStylization(pkg.synthetic_weights(0), cuda=True, style_num=NS)
            m.set_multistyle_group(G)
            m.prepare_style([V.resize_bilinear(pkg.synth_style(512, 512, kind="noise", seed=7 + k), (384, 384)) for k in range(NS)])
            m.clean()
            for i in (0, 8):
                m.add_patch(m.generate_content_features(V.reflect_pad(pkg.synth_frame(i, S, S, kind="noise"), P, P)))
            m.compute_norm()
            m.release_features()
            h_frames = pkg.pinned_empty((B, P, P, 3), np.uint8)
            for k in range(B):
                h_frames[k] = V.reflect_pad(pkg.synth_frame(k % 4, S, S, kind="noise"), P, P)
            feats = m.generate_content_features_batch(h_frames)
            del h_frames
            wts = [V.ramp_weights(k, 300, NS, blend="all") for k in range(B)]
            h_out = pkg.pinned_empty((2, B, P, P, 3), np.float32)
            call = lambda i=0: m.transfer_many(feats, wts, out=h_out[i & 1])
            nseq = B // G
        else:
            S = int(leg)
            P = V.padded_size(S)
            B = 128
            m = pkg.Stylization(pkg.synthetic_weights(0), cuda=True)
            m.prepare_style(pkg.synth_style(512, 512, kind="noise", seed=7))
            m.clean()
            for i in (0, 8, 16):
                m.add(pkg.synth_frame(i, S, S, kind="noise"))
            m.compute()
            h_in = pkg.pinned_empty((B, P, P, 3), np.uint8)
            for k in range(B):
                h_in[k] = V.reflect_pad(pkg.synth_frame(k % 8, S, S, kind="noise"), P, P)
            h_out = pkg.pinned_empty((2, B, P, P, 3), np.float32)
            call = lambda i=0: m.transfer_batch(h_in, out=h_out[i & 1])
            nseq = B // max(1, min(32, (16 * 640 * 640) // (P * P)))
        with Stderr() as err:
            for i in range(warm + a.reps):
                call(i)
            m.sync()
        report(leg, parse(err.text), warm)
        if a.rows:
            with Stderr() as err:
                rows_of_one_sequence(m, call, nseq, leg)
        m.close()


if __name__ == "__main__":
    main()

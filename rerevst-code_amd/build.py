"""Builds librerevst_scale.so (the input resampler's kernels), librerevst_deliver.so (the output resampler's), librerevst_guided.so (the
guided delivery stage's) and librerevst_hip.so (everything else, linked against the three) in-tree with hipcc for gfx950 (cross-compiles
without a GPU).  Four libraries so that each code object holds exactly the kernels its ledger names."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librerevst_hip.so")
SCALE_LIB = os.path.join(HERE, "librerevst_scale.so")
DELIVER_LIB = os.path.join(HERE, "librerevst_deliver.so")
GUIDED_LIB = os.path.join(HERE, "librerevst_guided.so")
SOURCES = ["rerevst_hip.hip"]
SCALE_SOURCES = ["resample.hip"]
SCALE_HEADERS = ["resample.h", "conv_thin.h", "conv_mfma.h"]
DELIVER_SOURCES = ["deliver.hip"]
DELIVER_HEADERS = ["deliver.h", *SCALE_HEADERS]
GUIDED_SOURCES = ["guided.hip"]
GUIDED_HEADERS = ["guided.h", *SCALE_HEADERS]
HEADERS = ["conv_mfma.h", "conv_wino.h", "conv_ups5.h", "conv_wino_split.h", "conv_f43.h", "conv_thin.h", "prep_kernels.h", "mask_kernels.h", "resample.h", "deliver.h", "guided.h",
           "../../include/rerevst_hip.h"]


def _newer(lib, files):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in files)


def _stale():
    return (_newer(SCALE_LIB, SCALE_SOURCES + SCALE_HEADERS) or _newer(DELIVER_LIB, DELIVER_SOURCES + DELIVER_HEADERS) or
            _newer(GUIDED_LIB, GUIDED_SOURCES + GUIDED_HEADERS) or _newer(LIB, SOURCES + HEADERS))


def _run(cmd, verbose):
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_lib(force=False, verbose=True, extra=()):
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-result"]
    if force or _newer(SCALE_LIB, SCALE_SOURCES + SCALE_HEADERS):
        _run([*common, *[os.path.join(CSRC, s) for s in SCALE_SOURCES], "-o", SCALE_LIB], verbose)
    if force or _newer(DELIVER_LIB, DELIVER_SOURCES + DELIVER_HEADERS):
        _run([*common, *[os.path.join(CSRC, s) for s in DELIVER_SOURCES], "-o", DELIVER_LIB], verbose)
    if force or _newer(GUIDED_LIB, GUIDED_SOURCES + GUIDED_HEADERS):
        _run([*common, *[os.path.join(CSRC, s) for s in GUIDED_SOURCES], "-o", GUIDED_LIB], verbose)
    # the main library finds its three companions next to itself, wherever the package lies
    _run([*common, *extra, *[os.path.join(CSRC, s) for s in SOURCES], "-L" + HERE, "-lrerevst_scale", "-lrerevst_deliver", "-lrerevst_guided",
          "-Wl,-rpath,$ORIGIN", "-o", LIB], verbose)
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)

"""Builds librerevst_stages.so (the kernels of the frame stages around the network: input resampler, delivery, guided delivery; one
translation unit, csrc/stages.hip), librerevst_compose.so (the compositing stage behind them; one translation unit, csrc/compose.hip),
librerevst_jpeg.so (the JPEG output stage; one translation unit, csrc/jpeg.hip), librerevst_jpeg_in.so (the JPEG input stage; one translation
unit, csrc/jpeg_in.hip), librerevst_shots.so (the shot signature; one translation unit, csrc/shots.hip), librerevst_picture.so (the line profile of the picture-area
detector; one translation unit, csrc/picture.hip) and librerevst_hip.so (everything
else, linked against the six) in-tree with hipcc for gfx950 (cross-compiles without
a GPU).  Seven libraries so that the main unit's kernel set and compile time stay
what they are, the stages rebuild in seconds, and the kernel sets of the stages and the compositing library stay what their ledgers pin."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librerevst_hip.so")
STAGES_LIB = os.path.join(HERE, "librerevst_stages.so")
SOURCES = ["rerevst_hip.hip"]
COMPOSE_LIB = os.path.join(HERE, "librerevst_compose.so")
STAGES_SOURCES = ["stages.hip"]
COMPOSE_SOURCES = ["compose.hip"]
COMPOSE_HEADERS = ["compose.h", "compose_k.h"]
JPEG_LIB = os.path.join(HERE, "librerevst_jpeg.so")
JPEG_SOURCES = ["jpeg.hip"]
JPEG_HEADERS = ["jpeg.h", "jpeg_k.h"]
JPEG_IN_LIB = os.path.join(HERE, "librerevst_jpeg_in.so")
JPEG_IN_SOURCES = ["jpeg_in.hip"]
JPEG_IN_HEADERS = ["jpeg_dec.h", "jpeg_dec_k.h", "jpeg.h"]
SHOTS_LIB = os.path.join(HERE, "librerevst_shots.so")
SHOTS_SOURCES = ["shots.hip"]
SHOTS_HEADERS = ["shots.h", "shots_k.h"]
PICTURE_LIB = os.path.join(HERE, "librerevst_picture.so")
PICTURE_SOURCES = ["picture.hip"]
PICTURE_HEADERS = ["picture.h", "picture_k.h"]
STAGES_HEADERS = ["resample_k.h", "deliver_k.h", "guided_k.h", "rs_tile.h", "resample.h", "deliver.h", "guided.h", "conv_thin.h", "conv_mfma.h"]
HEADERS = ["conv_mfma.h", "conv_wino.h", "conv_ups5.h", "conv_wino_split.h", "conv_f43.h", "conv_thin.h", "prep_kernels.h", "mask_kernels.h", "resample.h", "deliver.h", "guided.h", "compose.h", "jpeg.h", "jpeg_dec.h", "shots.h", "picture.h",
           "../../include/rerevst_hip.h"]


def _newer(lib, files):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in files)


def _run(cmd, verbose):
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_lib(force=False, verbose=True, extra=()):
    stages = force or _newer(STAGES_LIB, STAGES_SOURCES + STAGES_HEADERS)
    compose = force or _newer(COMPOSE_LIB, COMPOSE_SOURCES + COMPOSE_HEADERS)
    jpeg = force or _newer(JPEG_LIB, JPEG_SOURCES + JPEG_HEADERS)
    jpeg_in = force or _newer(JPEG_IN_LIB, JPEG_IN_SOURCES + JPEG_IN_HEADERS)
    shots = force or _newer(SHOTS_LIB, SHOTS_SOURCES + SHOTS_HEADERS)
    picture = force or _newer(PICTURE_LIB, PICTURE_SOURCES + PICTURE_HEADERS)
    if not stages and not compose and not jpeg and not jpeg_in and not shots and not picture and not _newer(LIB, SOURCES + HEADERS):
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-result"]
    if stages:
        _run([*common, *[os.path.join(CSRC, s) for s in STAGES_SOURCES], "-o", STAGES_LIB], verbose)
    if compose:
        _run([*common, *[os.path.join(CSRC, s) for s in COMPOSE_SOURCES], "-o", COMPOSE_LIB], verbose)
    if jpeg:
        _run([*common, *[os.path.join(CSRC, s) for s in JPEG_SOURCES], "-o", JPEG_LIB], verbose)
    if jpeg_in:
        _run([*common, *[os.path.join(CSRC, s) for s in JPEG_IN_SOURCES], "-o", JPEG_IN_LIB], verbose)
    if shots:
        _run([*common, *[os.path.join(CSRC, s) for s in SHOTS_SOURCES], "-o", SHOTS_LIB], verbose)
    if picture:
        _run([*common, *[os.path.join(CSRC, s) for s in PICTURE_SOURCES], "-o", PICTURE_LIB], verbose)
    # the main library finds its companions next to itself, wherever the package lies
    _run([*common, *extra, *[os.path.join(CSRC, s) for s in SOURCES], "-L" + HERE, "-lrerevst_stages", "-lrerevst_compose", "-lrerevst_jpeg", "-lrerevst_jpeg_in", "-lrerevst_shots", "-lrerevst_picture", "-Wl,-rpath,$ORIGIN", "-o", LIB],
         verbose)
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)

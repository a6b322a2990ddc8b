"""Which test would fail if a kernel computed something slightly wrong?  LEDGER maps every kernel symbol of the cross-compiled gfx950
code object (symbols() below: tools/isa_diff.py kernels() on the built library, demangled, without return type and parameter list)
to one entry (kind, what):
  layer        a float64 layer reference of the kernel's own GPU input: ("file::test", how the test proves that THIS kernel ran)
  entry        an entry-level reference, or bit-identity to a `layer`-checked instantiation: ("file::test", what it compares)
  debug        dbg_*: (None, what it is for)
  unreachable  compiled, but no lookup can select it: (None, the lookup that never does)
Every instantiation is its own compile here (inline-asm MFMAs, pinned AGPRs, 150 KB of LDS), and one instantiation alone has been
wrong before (profiles/HISTORY.md: conv_wino_k<2,0,4,1,1,.> passed an accumulator quad through scratch), so "the same source is
tested" is not an entry.  tests/test_kernel_ledger.py keeps the ledger and the library equal.  Plain module, names only: nothing here
reads a kernel's instructions."""
import importlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_lib():
    return importlib.import_module("rerevst-code_amd.build").build_lib(verbose=False)


def short(demangled):
    """'void conv_f43_k<1, 0>(ConvP)' -> 'conv_f43_k<1, 0>'"""
    d = re.sub(r"\((?!anonymous namespace\)).*$", "", demangled.strip())
    return d[5:] if d.startswith("void ") else d


def symbols(lib):
    """The kernel symbols of the library's gfx950 code object, demangled and shortened, in the code object's order."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        isa_diff = importlib.import_module("isa_diff")
    finally:
        sys.path.pop(0)
    with tempfile.TemporaryDirectory() as tmp:
        names = list(isa_diff.kernels(lib, tmp, "ledger"))
    out = subprocess.run(["c++filt"], input="\n".join(names).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(names)
    return [short(d) for d in out]


def check_stage_ledger(ledger, family, one_test_each):
    """A stage's ledger (kernel symbol -> "file::test", the test that holds THAT kernel to its reference) against librerevst_stages.so:
    the kernels of the library whose name contains `family` are exactly the ledger's keys, and every test it names exists."""
    build = importlib.import_module("rerevst-code_amd.build")
    build.build_lib(verbose=False)
    stages = symbols(build.STAGES_LIB)
    assert len(stages) == len(set(stages))
    mine = {s for s in stages if family in s}
    assert mine == set(ledger), (sorted(mine - set(ledger)), sorted(set(ledger) - mine))
    if one_test_each:
        assert len(set(ledger.values())) == len(ledger)
    for key, ref in ledger.items():
        path, name = ref.split("::")
        assert os.path.isfile(os.path.join(ROOT, path)), (key, ref)
        mod = importlib.import_module(os.path.splitext(os.path.basename(path))[0])
        assert callable(getattr(mod, name, None)), (key, ref)


GL = "tests/test_gpu_layers.py::"
FM = "tests/test_gpu_frame_mode_layers.py::"
MK = "tests/test_gpu_mask_layers.py::"
PL = "tests/test_gpu_prep_layers.py::"
IN = "tests/test_gpu_instantiations.py::"
PK = "tests/test_gpu_packs.py::"
WIN = "; windowed launch (pad / crop): tests/test_gpu_window_layers.py::"

LEDGER = {}


def _add(kind, keys, ref, what):
    for k in ([keys] if isinstance(keys, str) else keys):
        assert k not in LEDGER, k
        LEDGER[k] = (kind, ref, what)


# ---- the convolutions ---------------------------------------------------------------------------------------------------------------------
# conv_wino_split_k<EPI, IMG> (CONV_ROWS: WS(EPI, 0) = shared state, WS(EPI, 1) = the per-image row, where a caller reaches one).  EPI: 1 ReLU, 65 + pool, 5 + Decoder.norm[0],
# 54 ResidualBlock.conv2, 2 LeakyReLU, 0 raw split-K slices, 8 + residual, 40 + residual + AdaIN
EVERY = GL + "test_every_layer_against_its_own_input"
_add("layer", "conv_wino_split_k<1, 0>", EVERY, "kind f23: the rows of c21 / c31 / c32 / c33 are conv_wino<E_RELU> (family_of), NHWC taps")
_add("layer", "conv_wino_split_k<65, 0>", EVERY, "kind f23: the rows of p1 / p2 / p3 are conv_wino<E_RELU | E_POOL>")
_add("layer", "conv_wino_split_k<5, 0>", EVERY, "every kind: c41's row is conv_wino<E_RELU | E_NORM1>, one shared state set")
_add("layer", "conv_wino_split_k<54, 0>", EVERY, "kind f23: the rows of o4 / o3 / o2 are conv_wino, asserted f23" + WIN + "test_windowed_launch_on_a_stale_workspace, kind f23")
_add("layer", "conv_wino_split_k<2, 0>", GL + "test_split_k_kernel_filter", "1536 x 2048: no sum_parts row follows, dpart is refused: the unsplit LeakyReLU kernel")
_add("layer", "conv_wino_split_k<0, 0>", GL + "test_split_k_kernel_filter", "640 and 1152: sum_parts follows each down row, dpart has 32 x split channels")
_add("layer", "conv_wino_split_k<8, 0>", EVERY, "f1 / f2 (two kernels in one, LR.COMPOSITE): the up rows are conv_wino<E_RES>")
_add("layer", "conv_wino_split_k<40, 0>", EVERY, "f3's row is conv_wino, family f23")
_add("layer", "conv_wino_split_k<5, 1>", IN + "test_blended_frames_per_image_conv4_1",
     "c41's row is conv_wino<..> at 256 x 512 and debug_state_set(0, 1) succeeds: conv() took the IMG row; image 2 on set 0 fails")
_add("layer", "conv_wino_split_k<54, 1>", IN + "test_blended_frames_per_image_conv4_1",
     "kind default: o4 / o3 / o2 asserted f23 in a launch with per-image state (the grouped test of the frame-mode suite too)" + WIN + "test_windowed_launch_with_per_image_state")
_add("layer", "conv_wino_split_k<2, 1>", IN + "test_filter_down_per_image_weights_frame_mode",
     "64 x 16400: the down rows are conv_wino<E_LRELU> without sum_parts, dpart refused, two images; image 1's d on set 0 fails")
_add("layer", "conv_wino_split_k<0, 1>", FM + "test_every_frame_mode_stage",
     "B > 1: dpart has 256 channels (split 8) under per-image folded weights; split 4: test_gpu_instantiations, 64 x 5136")
_add("layer", "conv_wino_split_k<8, 1>", FM + "test_every_frame_mode_stage", "B > 1: f1 / f2 on each image's own folded weights; image 7 on set 8 fails f1")
_add("layer", "conv_wino_split_k<40, 1>", FM + "test_every_frame_mode_stage", "B > 1: f3 on each image's own set; image 7 on set 8 fails f3")

# conv_wino_k<EPI, 0, 4, UPS=1, SC, IMG> (CONV_ROWS: UP(EPI, SC, IMG)): the upsample-fused ResidualBlock.conv1 (EPI 6: LeakyReLU + norm1; 2: raw LeakyReLU)
_add("layer", "conv_wino_k<6, 0, 4, 1, 1, 0>", EVERY, "every kind: a4 / a3 / a2 and xs4 / xs3 / xs2 asserted family ups (conv_upw_sc rows)" + WIN + "test_windowed_launch_on_a_stale_workspace, every kind")
_add("layer", "conv_wino_k<6, 0, 4, 1, 1, 1>", IN + "test_blended_frames_per_image_conv4_1",
     "a4 / a3 / a2 of images 0 and 2 on their own sets in a launch with per-image state (resblock_frame sets par_bstride)" + WIN + "test_windowed_launch_with_per_image_state")
_add("layer", "conv_wino_k<2, 0, 4, 1, 1, 0>", FM + "test_every_frame_mode_stage", "frame_families: the conv1 rows are conv_upw_sc, family ups, raw output + statistics")
_add("layer", "conv_wino_k<2, 0, 4, 1, 0, 0>", PL + "test_every_stop_of_the_resident_pass", "the nine-product conv_upw<E_LRELU> of the preparation pass (unfused shortcut)")

# conv_f43_k<EPI, LAY> (CONV_ROWS: F4(EPI, LAY); per-image parameters are read by the same instantiation)
_add("layer", ["conv_f43_k<1, 0>", "conv_f43_k<65, 0>", "conv_f43_k<54, 0>"], EVERY, "kind f43_nhwc: ENC_F43 + DEC_F43 asserted f43, every layout 0" + WIN + "test_windowed_launch_on_a_stale_workspace, kind f43_nhwc (<54, 0>)")
_add("layer", ["conv_f43_k<65, 3>", "conv_f43_k<1, 3>", "conv_f43_k<65, 1>", "conv_f43_k<54, 1>"], EVERY,
     "kind f43_p8: ENC_F43 + DEC_F43 asserted f43, c11 .. c33 and a4 / a3 / a2 layout 1, p3 layout 0" + WIN + "test_windowed_launch_on_a_stale_workspace, kind f43_p8 (<54, 1>)")

# conv_mfma_k<BN, TAPS, EPI, ..> (CONV_ROWS: MF(BN, TAPS, EPI))
_add("layer", ["conv_mfma_k<128, 1, 0, 0, 0, 1>", "conv_mfma_k<64, 1, 0, 0, 0, 1>"], PL + "test_every_stop_of_the_resident_pass",
     "the unfused 1 x 1 shortcuts of the preparation pass, family gemm")
_add("layer", "conv_mfma_k<32, 9, 0, 0, 0, 1>", PL + "test_every_stop_of_the_resident_pass", "the FilterPredictor 512 -> 32 convolutions, family gemm")
_add("layer", ["conv_mfma_k<64, 9, 65, 0, 0, 1>", "conv_mfma_k<128, 9, 1, 0, 0, 1>", "conv_mfma_k<128, 9, 65, 0, 0, 1>", "conv_mfma_k<128, 9, 5, 0, 0, 1>"],
     IN + "test_direct_form_encoder", "RRV_DIRECT_LAYERS=0x1fe: the eight encoder rows are conv_mfma<64,9,..> / <128,9,..>, four distinct names")

# conv_first_k<IN>, conv_last_k<U8, CHW, SPACE, YUV, Y16> (conv_thin.h)
_add("layer", "conv_first_k<0>", EVERY, "c11 from grey_input of the uint8 BGR frame, family direct")
_add("entry", ["conv_first_k<1>", "conv_first_k<2>", "conv_first_k<3>"], "tests/test_gpu_tensor_io.py::test_input_forms_equal_uint8_path",
     "planar / float32 input gives the bits of the uint8 HWC path (conv_first_k<0>)")
_add("entry", ["conv_first_k<4>", "conv_first_k<5>"], "tests/test_gpu_yuv_input.py::test_device_entries", "8-bit I420 / NV12 input against the converted frame's path")
_add("entry", ["conv_first_k<6>", "conv_first_k<7>"], "tests/test_gpu_yuv16.py::test_input_device_entries", "10 / 12 / 16-bit planar and P01x input")
_add("layer", "conv_last_k<false, false, 0, false, false>", EVERY, "pre (the pre-clamp output) from o2, family direct" + WIN + "test_windowed_launch_on_a_stale_workspace; the uint8 and NV12 forms: test_windowed_launch_in_the_quantising_output_forms")
_add("entry", ["conv_last_k<false, false, 1, false, false>", "conv_last_k<false, false, 2, false, false>", "conv_last_k<false, true, 0, false, false>",
               "conv_last_k<false, true, 1, false, false>", "conv_last_k<false, true, 2, false, false>", "conv_last_k<true, true, 0, false, false>"],
     "tests/test_gpu_tensor_io.py::test_output_forms", "every output form against the float32 BGR frame of conv_last_k<false, false, 0, false, false>")
_add("entry", "conv_last_k<true, false, 0, false, false>", "tests/test_gpu_u8_output.py::test_global_device_entries", "uint8 = the float32 frame rounded half to even")
_add("entry", "conv_last_k<true, false, 0, true, false>", "tests/test_gpu_yuv_output.py::test_global_host_entries", "8-bit YUV 4:2:0 of the float32 frame (tests/yuv_ref.py)")
_add("entry", "conv_last_k<true, false, 0, true, true>", "tests/test_gpu_yuv16.py::test_output_device_entries", "10 / 12 / 16-bit YUV 4:2:0 (tests/yuv16_ref.py)")

# ---- statistics, predictions, pointwise passes ----------------------------------------------------------------------------------------------
_add("layer", ["chan_stat_k", "chan_final_k", "fc_filter_k"], PL + "test_every_stop_of_the_resident_pass", "families pstat / ppred at all 14 sync points")
_add("layer", ["chan_merge_k", "chan_finish_k"], PL + "test_streaming_ragged_groups", "the merged statistics of groups of 1, 2 and 3 frames, family pstat")
_add("layer", ["chan_stat1_k", "chan_stat1_final_k", "rect_sums_k", "pred_mean_k", "frame_sets_init_k"], FM + "test_every_frame_mode_stage",
     "frame_families asserts FRAME_SEQ; families stat / pred, the identity entry exactly")
_add("layer", "pointwise_k", FM + "test_every_frame_mode_stage",
     "family point on every normalised tap; with per-image Decoder.norm[0] of cached features: test_gpu_instantiations, case b")
_add("layer", "sum_parts_lrelu_k", GL + "test_split_k_kernel_filter", "d is the sum of dpart's slices + LeakyReLU, family splitk")
_add("layer", "blend_sets_k", FM + "test_grouped_multistyle_launch_state_sets_and_layers", "each image's set against the float64 blend (LR.blend_ref), family stat")
_add("layer", ["mask_norm_k", "mask_filter_k"] + ["mask_pyramid_k<%d>" % s for s in range(1, 9)], MK + "test_every_masked_stage",
     "mask_families asserts the 37-launch sequence; S = 1 .. 8 each have a case; level masks bit for bit, families mnorm / mfilt")

# ---- packs and folds: each buffer a handle holds, read back (rrv_debug_copy_weights) and held to a reference of its own ------------------------
# The read-back walks the handle's own ConvW / first_w / last_w / state-set pointers, the ones every launch passes to its kernel, and
# test_the_enumeration_is_the_cases pins the walk to the cases: the buffer a case reads is the buffer that kernel wrote.
BUF = PK + "test_buffer_against_its_reference"
_add("layer", "pack_wino_k", BUF, "every pk_wino (16 positions; the folded KernelFilters' at 32 and at 32 x nsets couts) and pk_ups (9 positions) buffer: float32, n = 4")
_add("layer", "pack_f43_k", BUF, "every pk_f43 buffer: each element the one rounding of the extended-precision U")
_add("layer", "pack_ups5_k", BUF, "every pk_ups_sc buffer: the 25 positions rounded once, the shortcut block w / 4 exactly")
_add("layer", "pack_conv_k", BUF, "every pk buffer at BN 32, 64 and 128, 1 and 9 taps: bit for bit")
_add("layer", "pack_first_k", BUF, "the `first` buffers of both encoders: bit for bit")
_add("layer", "pack_first_grey_k", BUF, "Encoder.slice.0's first_grey buffer: W1, W0 and the folded bias, float32 with n = 3 / 4 / 29")
_add("layer", "pack_last_k", BUF, "Decoder.slice1's `last` buffer with its zero rows 27..31: bit for bit")
_add("layer", "fold_down_k", BUF, "Decoder.Filter<f>.fold_down raw and bias: set 0 under two states in turn, sets 0..2 of a grouped launch each on its own F1; image 1 on set 0's fails")
_add("layer", "fold_up_k", BUF, "Decoder.Filter<f>.fold_up raw: the same sets on their own F2; image 1 on set 0's fails")

# ---- debug -------------------------------------------------------------------------------------------------------------------------------
_add("debug", ["dbg_poke_k", "(anonymous namespace)::dbg_check_k", "(anonymous namespace)::dbg_fill_k"], None, "rrv_set_debug's canaries and self-test")

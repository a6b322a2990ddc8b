// rerevst_hip.hip — host side of librerevst_hip.so: the C ABI declared in
// include/rerevst_hip.h, weight upload/repack, the per-frame launch sequence
// (Stylization.transfer, test/framework.py:106-118) and the preparation passes
// (prepare_style / add / compute, test/framework.py:82-104).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <thread>
#include <stdio.h>
#include <map>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rerevst_hip.h"
#include "conv_mfma.h"
#include "conv_wino.h"
#include "conv_wino_split.h"
#include "conv_f43.h"
#include "conv_thin.h"
#include "prep_kernels.h"
#include "mask_kernels.h"
#include "resample.h"      // librerevst_stages.so: parameters and the launch entry of the resampler
#include "guided.h"        //                       of the guided delivery stage
#include "compose.h"       //                       of the compositing stage (librerevst_compose.so)
#include "deliver.h"       //                       of the output-side resampler
#include <functional>
#include "jpeg.h"          // librerevst_jpeg.so: plan, tables, header and the launch entries of the JPEG output stage
#include "jpeg_dec.h"      // ... and of the JPEG input stage: parser, plan, decode tables and launch entries
#include "shots.h"         // librerevst_shots.so: parameters and the launch entry of the shot signature
#include "picture.h"       // librerevst_picture.so: parameters and the launch entry of the line profile

namespace {

// ---- state blob layout (must match oracle/rerevst_oracle.py and DESIGN.md) -------------
const int NORM_CH[11] = {512, 512, 256, 128, 64, 256, 256, 128, 128, 64, 64};
enum { N_DEC0 = 0, N_DEC1, N_DEC2, N_DEC3, N_DEC4, N_S4N1, N_S4N2, N_S3N1, N_S3N2, N_S2N1, N_S2N2 };
const int STYLE_CH[4] = {64, 128, 256, 512};
struct StateLayout {
    int norm[11], filt[6], sty[4];
    StateLayout() {
        int o = 0;
        for (int i = 0; i < 11; ++i) { norm[i] = o; o += 4 * NORM_CH[i]; }
        for (int i = 0; i < 6; ++i) { filt[i] = o; o += 1024; }
        for (int i = 0; i < 4; ++i) { sty[i] = o; o += 2 * STYLE_CH[i]; }
    }
};
const StateLayout SL;

struct Tens {
    float* p = nullptr;
    float* base = nullptr;            // debug mode: start of the allocation (guard band in front of p)
    int B = 0, H = 0, W = 0, C = 0;
    mutable unsigned gen = 0;         // launch (rrv_ctx::launch_gen) whose kernels last wrote this tensor, and for how many images
    mutable int gen_B = 0;            // (rrv_debug_copy_tensor_ex refuses a tensor its plan's last launch did not write)
    size_t img_floats() const { return (size_t)(H + 2) * (W + 2) * C; }
};

struct ConvW {           // one convolution's device weights
    float* raw = nullptr;    // OIHW as in the checkpoint
    float* pk = nullptr;     // kernel-native packed
    float* pk_wino = nullptr; // Winograd F(2x2,3x3) transformed pack for conv_wino_k
    float* pk_ups = nullptr; // upsample-fused transform pack (9 positions) for conv_wino_k<.., UPS = 1> (convs behind a nearest-x2 upsample)
    float* pk_ups_sc = nullptr; // five-product upsample transform (25 positions) + the block's 1x1 shortcut (conv_ups5.h: conv_wino_k<.., UPS = 1, SC = 1>)
    int f43_bit = 0;         // index of the layer in rrv_ctx::f43_layers (encoder conv1_2 .. conv3_4 = 0..6, slice4/3/2.conv2 = 7..9)
    float* pk_f43 = nullptr; // Winograd F(4x4,3x3) transformed pack for conv_f43_k (encoder convs and ResidualBlock.conv2 of the per-frame path)
    float* bias = nullptr;   // [Cout] (zeros for bias-free convs)
    int Cout = 0, Cin = 0, taps = 0, BN = 0;
};

struct ProfEntry { std::string name; hipEvent_t e0, e1; double flops, bytes; float ms; double flops_exec;
                   unsigned grid; int xcd_slabs; };      // rrv_profile_entry_grid: the grid launch() was told of (0, -1: none recorded)

// VGG conv indices and (cin,cout)
const int VGG_IDX[9] = {0, 2, 5, 7, 10, 12, 14, 16, 19};
const int VGG_CIN[9] = {3, 64, 64, 128, 128, 256, 256, 256, 256};
const int VGG_COUT[9] = {64, 64, 128, 128, 256, 256, 256, 256, 512};
const int STYLE_SLICE[9] = {1, 2, 2, 3, 3, 4, 4, 4, 4};
std::string enc_key(int which, int i) {      // the checkpoint's name of VGG conv i (0..8) of the content (which = 0) / style (1) encoder
    char k[64];
    if (which == 0) snprintf(k, sizeof k, "Encoder.slice.%d", VGG_IDX[i]);
    else snprintf(k, sizeof k, "EncoderStyle.slice%d.%d", STYLE_SLICE[i], VGG_IDX[i]);
    return k;
}

struct EncPlan {   // encoder activations for one (B, H, W)
    int B = 0, H = 0, W = 0;
    unsigned stamp = 0;
    unsigned gen = 0;       // last launch that used this plan (rrv_ctx::launch_gen)     // last use (two geometries per slot, least recently used one is replaced)
    Tens c11, p1, c21, p2, c31, c32, c33, p3, c41;
    // channel-chunk-major ("P8": [B][C/8][H+2][W+8][8], conv_f43.h LAY) twins of the tensors BETWEEN two conv_f43_k launches — and of c11, which
    // conv_first_k can write either way — built with the per-frame plans as ring-layout tensors of B * C/8 eight-channel images of width W + 6
    // (so the debug mode's ring / guard checks cover them unchanged).  A twin and its NHWC original never mix: each keeps its own zero ring.
    Tens q11, q1, q21, q2, q31, q32, q33;
};
struct DecPlan {   // per-frame decoder activations for one (B, H, W) of the FRAME batch
    int B = 0, H = 0, W = 0;
    unsigned stamp = 0;
    unsigned gen = 0;
    Tens d, f[3];           // KernelFilter: the 32-channel intermediate, the outputs of Filter1..3
    Tens xs[3], a[3], o[3]; // per residual block (BLKS: slice4, slice3, slice2): shortcut, conv1 output, block output
    Tens dpart;             // [.., 32 * split]: partial sums of the split-K 512->32 KernelFilter convolution (kf_split > 1 only)
    Tens qa[3];             // channel-chunk-major twins of a[0..2] (ResidualBlock.conv1's output when conv2 runs conv_f43_k; EncPlan::q11 .. above)
    // batched frame mode only (frame_mode_device): per-image scratch, image b in interior row b (frame_row): chan_stat1_k partials
    // (min(H_l, 512) x 3 x C_l doubles <= 3 x 64 x H), rect_sums_k's nine sums [9][512], pred_mean_k's two predicted means [2][32]
    Tens spart, srect, scm;
    // masked multi-style entries only (mask_mode_device): the four level masks, level l at H >> l x W >> l, the S weights of a pixel
    // contiguous in the interior of a ring-layout tensor of RRV_MAX_STYLES channels (mask_kernels.h LevelMask)
    Tens lm[4];
    float* pre = nullptr;   // [H][W][3] pre-clamp tap
};

// workspace of one rrv_compute: the preparation pass (compute_style) or its streaming form (compute_style_streaming)
struct PrepPlan {
    Tens cn, nxt, t32, d32, u, xs[3], a[3], o[3];
    Tens content;                   // resident pass: the relu4_1 features of every sampled frame
    Tens grp, f0, su[3];            // streaming pass: one group's features, frame 0's, and its three KernelFilter residuals
};

// One workspace tensor of a plan: where it lives in the plan, its level (H, W >> level of the plan geometry), its channels
// and flags.  A P8 twin of a C-channel tensor is B * C/8 eight-channel images of width W + 6 (EncPlan::q11 ..).
enum { TS_P8 = 1, TS_ONE = 2 /* one image */, TS_SPLIT = 4 /* C x the KernelFilter split, absent at 1 */, TS_RES = 8 /* resident pass only */, TS_STREAM = 16 /* streaming pass only */,
       TS_FRAME = 32 /* batched frame-mode scratch: ONE tensor of B rows of C x 64 floats (one row per image), built for frame-mode plans only */,
       TS_PER_ROW = 64 /* TS_FRAME: C x 64 floats per pixel row of the plan (C x 64 x H per image) */,
       TS_MASK = 128 /* level masks: built for the plans of the masked multi-style entries only */ };
template <class P> struct TSpec {
    size_t off; int level, C, flags;
    Tens& of(P& p) const { return *(Tens*)((char*)&p + off); }
    void geo(int& B, int& H, int& W, int& C) const {     // B, H, W of the plan, C of the tensor -> the tensor's talloc arguments
        if (flags & TS_FRAME) { W = C * ((flags & TS_PER_ROW) ? H : 1); H = B; B = 1; C = 64; return; }
        if (flags & TS_ONE) B = 1;
        H >>= level; W >>= level;
        if (flags & TS_P8) { B *= C / 8; W += 6; C = 8; }
    }
};
// (the order of the rows is that of the debug taps: tap_row)
const TSpec<EncPlan> ENC_T[] = {
    {offsetof(EncPlan, c11), 0, 64}, {offsetof(EncPlan, p1), 1, 64}, {offsetof(EncPlan, c21), 1, 128}, {offsetof(EncPlan, p2), 2, 128}, {offsetof(EncPlan, c31), 2, 256},
    {offsetof(EncPlan, c32), 2, 256}, {offsetof(EncPlan, c33), 2, 256}, {offsetof(EncPlan, p3), 3, 256}, {offsetof(EncPlan, c41), 3, 512},
    {offsetof(EncPlan, q11), 0, 64, TS_P8}, {offsetof(EncPlan, q1), 1, 64, TS_P8}, {offsetof(EncPlan, q21), 1, 128, TS_P8}, {offsetof(EncPlan, q2), 2, 128, TS_P8},
    {offsetof(EncPlan, q31), 2, 256, TS_P8}, {offsetof(EncPlan, q32), 2, 256, TS_P8}, {offsetof(EncPlan, q33), 2, 256, TS_P8},
};
// The encoder's 3x3 layers conv1_2 .. conv4_1 (VGG conv 1..8): level (H, W >> level), epilogue, and what the layer reads and writes in the
// NHWC chain and in the channel-chunk-major one — a P8 twin where the two differ: conv3_4 writes, and conv4_1 reads, the NHWC p3 in either.
typedef Tens EncPlan::*EncT;
struct EncLayer { int level, epi; EncT in, out, qin, qout; };
const EncLayer ENC_LAYERS[8] = {
    {0, E_RELU | E_POOL, &EncPlan::c11, &EncPlan::p1, &EncPlan::q11, &EncPlan::q1},   {1, E_RELU, &EncPlan::p1, &EncPlan::c21, &EncPlan::q1, &EncPlan::q21},
    {1, E_RELU | E_POOL, &EncPlan::c21, &EncPlan::p2, &EncPlan::q21, &EncPlan::q2},   {2, E_RELU, &EncPlan::p2, &EncPlan::c31, &EncPlan::q2, &EncPlan::q31},
    {2, E_RELU, &EncPlan::c31, &EncPlan::c32, &EncPlan::q31, &EncPlan::q32},          {2, E_RELU, &EncPlan::c32, &EncPlan::c33, &EncPlan::q32, &EncPlan::q33},
    {2, E_RELU | E_POOL, &EncPlan::c33, &EncPlan::p3, &EncPlan::q33, &EncPlan::p3},   {3, E_RELU, &EncPlan::p3, &EncPlan::c41, &EncPlan::p3, &EncPlan::c41},
};
const TSpec<DecPlan> DEC_T[] = {
    {offsetof(DecPlan, d), 3, 32}, {offsetof(DecPlan, f[0]), 3, 512}, {offsetof(DecPlan, f[1]), 3, 512}, {offsetof(DecPlan, f[2]), 3, 512}, {offsetof(DecPlan, xs[0]), 3, 256},
    {offsetof(DecPlan, a[0]), 2, 256}, {offsetof(DecPlan, o[0]), 2, 256}, {offsetof(DecPlan, xs[1]), 2, 128}, {offsetof(DecPlan, a[1]), 1, 128}, {offsetof(DecPlan, o[1]), 1, 128},
    {offsetof(DecPlan, xs[2]), 1, 64}, {offsetof(DecPlan, a[2]), 0, 64}, {offsetof(DecPlan, o[2]), 0, 64}, {offsetof(DecPlan, dpart), 3, 32, TS_SPLIT},
    {offsetof(DecPlan, qa[0]), 2, 256, TS_P8}, {offsetof(DecPlan, qa[1]), 1, 128, TS_P8}, {offsetof(DecPlan, qa[2]), 0, 64, TS_P8},
    {offsetof(DecPlan, spart), 0, 6, TS_FRAME | TS_PER_ROW}, {offsetof(DecPlan, srect), 0, 9 * 512 / 64, TS_FRAME}, {offsetof(DecPlan, scm), 0, 1, TS_FRAME},
    {offsetof(DecPlan, lm[0]), 0, RRV_MAX_STYLES, TS_MASK}, {offsetof(DecPlan, lm[1]), 1, RRV_MAX_STYLES, TS_MASK}, {offsetof(DecPlan, lm[2]), 2, RRV_MAX_STYLES, TS_MASK},
    {offsetof(DecPlan, lm[3]), 3, RRV_MAX_STYLES, TS_MASK},
};
// levels count from the full-resolution decoder output: relu4_1 (the plan's hh x ww) is level 3
const TSpec<PrepPlan> PREP_T[] = {
    {offsetof(PrepPlan, cn), 3, 512}, {offsetof(PrepPlan, nxt), 3, 512}, {offsetof(PrepPlan, t32), 3, 32}, {offsetof(PrepPlan, d32), 3, 32, TS_ONE}, {offsetof(PrepPlan, u), 3, 512, TS_ONE},
    {offsetof(PrepPlan, xs[0]), 3, 256}, {offsetof(PrepPlan, a[0]), 2, 256}, {offsetof(PrepPlan, o[0]), 2, 256}, {offsetof(PrepPlan, xs[1]), 2, 128}, {offsetof(PrepPlan, a[1]), 1, 128},
    {offsetof(PrepPlan, o[1]), 1, 128}, {offsetof(PrepPlan, xs[2]), 1, 64}, {offsetof(PrepPlan, a[2]), 0, 64}, {offsetof(PrepPlan, o[2]), 0, 64},
    {offsetof(PrepPlan, content), 3, 512, TS_RES}, {offsetof(PrepPlan, grp), 3, 512, TS_STREAM}, {offsetof(PrepPlan, f0), 3, 512, TS_ONE | TS_STREAM},
    {offsetof(PrepPlan, su[0]), 3, 512, TS_ONE | TS_STREAM}, {offsetof(PrepPlan, su[1]), 3, 512, TS_ONE | TS_STREAM}, {offsetof(PrepPlan, su[2]), 3, 512, TS_ONE | TS_STREAM},
};

struct StyleState {
    bool prepared = false, computed = false;
    bool illcond = false;            // its dynamic filters are far from the O(1) scale (filter_conditioning): F(4x4,3x3) stays off the encoder
    float* blob = nullptr;           // RRV_STATE_FLOATS on device
    Tens map;                        // relu4_1 style map
    float* smean = nullptr;          // [6][32]: mean_{HW} F{1,2}.down_sample(normalised style map) of Filter1..3 (FilterPredictor's style half, constant per style)
};

// Format of the frames an encoder launch reads: form = IN_* (the conv_first_k instantiation), space = SP_* of a float32 form.  It travels
// with the request (Xfer::in, the pending sampled frames), never on the handle.
struct InFmt { int form, space; int cs = CS_420; };      // cs: chroma format of a YUV form (CS_*), carried next to the layout
constexpr InFmt IN_BGR8{IN_U8_HWC, SP_PIXEL};      // uint8 HWC BGR PIXEL: what every entry without a descriptor or an in_layout takes
inline bool operator!=(InFmt a, InFmt b) { return a.form != b.form || a.space != b.space || a.cs != b.cs; }

// The YUV conversion state of one direction (rrv_ctx::yuv_in: rows R, G, B x (Y, Cb, Cr, offset); yuv_out: rows Y, Cb, Cr x (R, G, B, offset)),
// read when a launch is queued (yuv_launch_params): launches already queued keep what they were queued with.
struct YuvSide {
    float m8[12];                         // the 8-bit forms' matrix (rrv_set_yuv_[input_]matrix); BT.601 limited range at rrv_create
    float m16[12]; bool set16 = false;    // the uint16 forms' own (rrv_set_yuv16_[input_]matrix); not set: BT.601 limited range at the depth in force at launch
    int bits = 10;                        // code depth of the uint16 forms (rrv_set_yuv_depth)
};

}  // namespace

// Layers that run F(4x4,3x3) where the launch geometry lets it win (use_f43): bit 0..6 = encoder conv1_2, conv2_1, conv2_2,
// conv3_1, conv3_2, conv3_3, conv3_4; bit 7..9 = slice4 / slice3 / slice2 .conv2.
// Default: all ten.  With the textbook interpolation points (0, +-1, +-2, inf) the ENCODER layers could not ship: Decoder.norm[0]
// multiplies relu4_1 errors by rstd up to 4e3 on near-dead channels, and the worst pre-clamp margin over the reference
// goldens reached 0.74-1.15 of the stated bound (profiles/r04_f43_layer_sets.txt).  With the balanced points of
// conv_f43.h (0, +-3/4, +-3/2, inf: 2.4x less rounding error) every golden stays <= 0.63 with all ten layers
// (profiles/r04_parity_margin.txt; F(2x2,3x3) everywhere: <= 0.49).  RRV_F43_LAYERS narrows the set (parity attribution).
constexpr unsigned F43_DEFAULT_LAYERS = 0x3ff;

struct rrv_ctx {
    int dev = 0;
    // A slot: a stream, its workspace and what belongs to a launch sequence on it.  How a sequence runs (its stream, state sets, kernel
    // choice) is never kept here: the entry that starts it says so in a Seq (below) and passes that down.
    struct Slot {
        hipStream_t stream = nullptr;
        hipEvent_t ev = nullptr;                     // ordering against the caller's stream (CallerOrder)
        // Two workspace geometries per slot: a caller alternating between two frame sizes (e.g. a video and its preview)
        // keeps both resident instead of re-allocating ~0.76 GB per call; a third size replaces the least recently used.
        EncPlan enc[2];
        DecPlan dec[2];
        // The scaled entries (Xfer::SH): a launch group's resampled float32 BGR PIXEL frames, grow-only, written and read on the slot's stream
        float* rs_buf = nullptr; size_t rs_cap = 0;
        // A delivered size (Xfer::DH): a launch group's stylized working frames, float32 BGR PIXEL, grow-only, between conv_last_k and deliver_k
        float* dl_buf = nullptr; size_t dl_cap = 0;
        // Guided delivery (Xfer::gr): a launch group's source at the delivered size, coefficient planes and result (X_hi, [6][H][W], Q), grow-only
        float* gd_xhi = nullptr; size_t gd_xhi_cap = 0;
        float* pc_canvas = nullptr; size_t pc_canvas_cap = 0;      // a picture request's canvas: the group's whole source frames, float32 HWC BGR PIXEL
        float* gd_ab = nullptr; size_t gd_ab_cap = 0;
        float* gd_q = nullptr; size_t gd_q_cap = 0;
        // JPEG output (Xfer::jp): a launch group's coefficient blocks and its interval lengths and offsets ([2][frames][intervals]), grow-only
        int16_t* jp_coef = nullptr; size_t jp_coef_cap = 0;
        uint32_t* jp_idx = nullptr; size_t jp_idx_cap = 0;
        int set_images = 0;                          // images whose state sets the slot's last launch wrote (frame mode, grouped multi-style); 0: it kept no per-image state (rrv_debug_copy_state)
    } slots[RRV_MAX_SLOTS];
    int n_slots = 2, next_slot = 0;                  // the alternating device entries cycle over n_slots slots
    hipStream_t caller_stream = nullptr; bool caller_sync = false;      // rrv_set_caller_stream's setting, written there only (a call with a stream of its own: Xfer::on_stream)
    int user_style = -1;                             // style the plain transfer entries use (first computed / last set_state)
    std::string err;
    std::map<std::string, std::vector<float>> hostw;
    std::map<std::string, std::vector<int64_t>> hostshape;
    bool finalized = false;
    std::map<std::string, ConvW> conv;         // keyed by state_dict prefix (without .weight)
    float *first_w[2] = {nullptr, nullptr}, *first_b[2] = {nullptr, nullptr};   // 0: Encoder, 1: EncoderStyle
    float* first_wg = nullptr;                                                  // Encoder conv1_1 folded for greyscaled frames
    float *last_w = nullptr, *last_b = nullptr;
    float* fc_w[6] = {nullptr}; float* fc_b[6] = {nullptr};
    float* zero_bias = nullptr;                // 512 zeros
    // The state the per-frame path reads (blob layout) and the KernelFilter weights folded with its dynamic filters.
    // Set 0 serves every single-state entry; the grouped models (frame mode, blended frames and cached features: run_xfer) give image g
    // of a launch sequence on slot 0 / 1 the set MS_GROUP_MAX * slot + g, since every image there has its own state (blend_sets writes
    // the blended ones).  Which set a launch sequence reads is in its Seq.
    // The sets live in CONTIGUOUS arrays (set i = base + i * stride): a launch whose images carry their own state
    // passes the first set and the strides, the kernels index by image.
    static constexpr int MS_GROUP_MAX = 16;      // multi-style frames per launch sequence (each with its own blended state set)
    static constexpr int N_SETS = 2 * MS_GROUP_MAX;      // two groups in flight.  9.9 MB per set (state blob + three KernelFilters' folded raw and packed weights), 316 MB of the 288 GB per handle, allocated once by rrv_finalize_weights
    struct StateSet { float* active = nullptr; ConvW fold_down[3], fold_up[3]; unsigned folded = 0; } sets[N_SETS];      // folded: bit f = fold_filters has written KernelFilter f's weights (rrv_debug_copy_weights)
    StateSet* slot_sets(int slot) { return &sets[MS_GROUP_MAX * slot]; }      // the first of the slot's sixteen sets.  Slots 0 and 1 only: the others own none (the grouped models alternate over these two, next_frame_slot)
    float* fold_tmp = nullptr;                 // OIHW scratch for folds (512*32*9 floats)
    StyleState styles[RRV_MAX_STYLES];
    int active_src = -1;                       // style id whose state is folded (-1: none, frame mode ran or the state was invalidated; -2: blend).  Written where the sets are written
    EncPlan enc_add, enc_style;
    unsigned plan_clock = 0;
    unsigned launch_gen = 0;                   // counts the launches of the per-frame chain (Tens::gen)
    // cached raw relu4_1 feature of one (padded) frame, H x W = frame size.  Beyond feat_cap (rrv_set_feature_cache_cap)
    // a frame is kept as its uint8 pixels instead (u8, ~10x smaller) and re-encoded when it is used: the reference's
    // cache is on disk and unbounded (test.py:87-101), this one degrades to "encode + decode per frame" instead of failing
    struct Feature { float* p; int H, W; uint8_t* u8; bool owned = true; };      // owned: its own allocation; else it lives in one of feat_blocks
    std::vector<Feature> features;
    std::vector<void*> feat_blocks;            // arenas of rrv_generate_content_features_batch (one allocation per call, features back to back)
    size_t feat_cap = (size_t)64 << 30, feat_bytes = 0;
    std::vector<float*> patches;               // relu4_1 features of added frames (ring layout images)
    int patch_h = 0, patch_w = 0, add_H = 0, add_W = 0;
    uint8_t* d_u8 = nullptr; size_t d_u8_cap = 0;      // a style image / a frame to cache on its way in (prepare_style, rrv_generate_content_features)
    // fixed-size scratch, one allocation made by rrv_finalize_weights: chan_stats partials and means; streaming compute(): second
    // partial buffer, two running accumulators [4][512] doubles; compute(): the predicted content means
    double *stat_part = nullptr, *stat_part2 = nullptr, *stat_acc = nullptr;
    float *stat_mean = nullptr, *prep_cmean = nullptr;
    size_t ws_cap = (size_t)64 << 30;          // preparation-pass workspace above which compute() streams groups of frames
    int last_groups = 0, last_group_size = 0; size_t last_ws_bytes = 0;
    PrepPlan prep;
    int prep_stop = -1;               // rrv_debug_prep_stop: rrv_compute ends at this sync point (ST_*) and keeps the plan; -1: off
    // frames handed to rrv_add wait here (uint8, HBM) and are encoded together, 8 per encoder launch, when their
    // features are first needed (rrv_compute): the encoder at B = 1 runs at a fraction of its batched rate
    uint8_t* pend_u8 = nullptr; size_t pend_cap = 0; int pend_n = 0;
    InFmt pend_in = IN_BGR8;          // format of the pending frames (a frame is kept as it arrived; conv_first_k<IN> reads it)
    // The scaled entries (Xfer::SH): the tap tables of every (source, destination) axis pair seen so far, in HBM (rs_tables; Slot::rs_buf holds the frames)
    struct RsTab { void* block = nullptr; RsAxis axis{}; int span = 0; };      // span: source samples the taps of RS_TH consecutive outputs cover, at most
    std::map<std::pair<int, int>, RsTab> rs_tabs;
    // rrv_deliver_guided_view_device's own coefficient planes and result (it runs on the caller's stream, beside whatever the slots hold in flight)
    float* gd_ab = nullptr; size_t gd_ab_cap = 0;
    float* gd_q = nullptr; size_t gd_q_cap = 0;
    // rrv_composite_view_device's own mixed frame (it runs on the caller's stream too)
    float* cm_buf = nullptr; size_t cm_cap = 0;
    // the JPEG entries' own scratch (they run on the caller's stream too): rrv_jpeg_encode_device's coefficient blocks, and the interval
    // lengths and offsets of the entropy half ([2][B][intervals]).  Grow-only; every word read was written by the same call
    int16_t* jp_coef = nullptr; size_t jp_coef_cap = 0;
    uint32_t* jp_idx = nullptr; size_t jp_idx_cap = 0;
    // the JPEG input entries' scratch (caller's stream too): the frame descriptors and decode tables of a call, the interval starts
    // ([B][intervals + 1]) and rrv_jpeg_decode_device's coefficient blocks.  Grow-only; every word read was written by the same call
    JpegDecFrame* jd_frames = nullptr; size_t jd_frames_cap = 0;
    uint32_t* jd_ivl = nullptr; size_t jd_ivl_cap = 0;
    int16_t* jd_coef = nullptr; size_t jd_coef_cap = 0;
    // the from-JPEG transfer entries: the decoded planes the network reads; the host twins' stream slots, statuses, output and matte of a sub-batch
    uint8_t* jd_planes = nullptr; size_t jd_planes_cap = 0;
    uint8_t* jd_streams = nullptr; size_t jd_streams_cap = 0;
    int* jd_status = nullptr; size_t jd_status_cap = 0;
    uint8_t* jd_out = nullptr; size_t jd_out_cap = 0;
    uint8_t* jd_matte = nullptr; size_t jd_matte_cap = 0;
    // the shot signature entries (include/rerevst_hip.h "Shots"): the thumbnails of a call (caller's stream too), and the host twins' frames and
    // signatures of a sub-batch.  Grow-only; every word read was written by the same call
    float* sg_thumb = nullptr; size_t sg_thumb_cap = 0;
    uint8_t* sg_in = nullptr; size_t sg_in_cap = 0;
    uint32_t* sg_sig = nullptr; size_t sg_sig_cap = 0;
    // the picture-area entries (include/rerevst_hip.h "Picture area"): the float frames and the column scratch of a profile call (caller's stream
    // too), and rrv_scan_frames' frames and results of a sub-batch.  Grow-only; every word read was written by the same call
    float* pc_frames = nullptr; size_t pc_frames_cap = 0;
    uint32_t* pc_part = nullptr; size_t pc_part_cap = 0;
    uint8_t* pc_in = nullptr; size_t pc_in_cap = 0;
    uint32_t* pc_prof = nullptr; size_t pc_prof_cap = 0;
    void* jd_pin = nullptr; size_t jd_pin_cap = 0; hipEvent_t jd_ev = nullptr;      // the descriptors' page-locked staging and the event behind its last copy
    const float* last_pre = nullptr; int last_pre_H = 0, last_pre_W = 0, last_pre_B = 0;   // where rrv_get_preclamp finds the last tap
    // host-buffer entry: two staging sets (pinned host + device, input and output) so that H2D / kernels / D2H /
    // the copies from and to the caller's pageable arrays of consecutive sub-batches overlap
    // Four sets and two dedicated copy streams: the compute streams never wait behind a DMA of their own stream.
    // Each set holds a device pair and a page-locked host pair (stage_reserve), in bytes of frames / bytes of output.
    struct StageBufs { uint8_t* in = nullptr; void* out = nullptr; size_t in_cap = 0, out_cap = 0; };
    struct HostStage {
        StageBufs dev, pin; hipEvent_t in_done = nullptr, k_done = nullptr, out_done = nullptr;
        // rrv_transfer_mask_batch: the sub-batch's style masks, in HBM and (for a pageable caller array) page-locked.  Grow-only and
        // released by rrv_destroy, as the staging buffers above are: rrv_set_debug and the other calls that drop the WORKSPACES keep all of them
        float *mask = nullptr, *mask_pin = nullptr; size_t mask_cap = 0, mask_pin_cap = 0;
        // the call's last sub-batch leaves in pieces (SeqHook): piece i's conv_last records piece_ev[i], its D2H on copy_out waits for it
        static constexpr int PIECES_MAX = 16;
        hipEvent_t piece_ev[PIECES_MAX] = {nullptr};
    } hstage[4];
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    // How host_pipeline orders its sub-batches (SeqHook; RRV_HOST_PHASE / RRV_HOST_PIECE are A/B knobs, the defaults the measured choice).
    // host_phase: the tail of sub-batch k+1's launch sequence waits for the last kernel of sub-batch k.  host_piece_px: pixels per piece of
    // the last sub-batch's conv_last + D2H (0: one launch, one copy; 1 / 2 / 4 frames at 640 x 640 measured alike, 1.03 / 1.07 / 1.12 ms of drain).
    bool host_phase = true;
    long host_piece_px = 2L * 640 * 640;
    // RRV_TIMELINE: the pipelined host entries time each call with events of their own (created by rrv_create, none per call) and print
    // one line per call to stderr.  Unset: no event exists and no call records one.
    struct Timeline {
        static constexpr int N = 64;      // sub-batches per call it can describe (a longer call prints nothing)
        bool on = false;
        hipEvent_t entry = nullptr, first = nullptr, k_end[N] = {nullptr}, d_end[N] = {nullptr};
    } tl;
    // rrv_transfer_async: ticket t lives in staging set t % 4 until rrv_transfer_wait(t) (or a later submission that needs
    // its set) retires it; `out` / `out_bytes` = where a pageable caller buffer still has to be filled from pin_out
    struct Ticket { long id = -1; void* out = nullptr; size_t out_bytes = 0; bool open = false; } tickets[4];
    long next_ticket = 0;
    int grid_share = 1;               // rrv_set_grid_share: persistent grids use 1/grid_share of the CUs (a Seq starts with it; written by that entry only)
    int f43_mode = 1;                 // rrv_set_f43 / RRV_F43: layers with an F(4x4,3x3) pack run on conv_f43_k — 0 never, 1 where the launch has enough work items for it to win (use_f43), 2 always
    unsigned f43_layers = F43_DEFAULT_LAYERS;   // which of the packed layers may run on conv_f43_k (RRV_F43_LAYERS overrides: experiments / parity attribution)
    bool illcond = false;             // some computed style's state is ill-conditioned (StyleState::illcond)
    int p8 = 3;                      // channel-chunk-major tensors in front of conv_f43_k launches (conv_f43.h LAY): bit 0 the encoder chain (EncPlan::q11 ..), bit 1 ResidualBlock.conv2's input (DecPlan::qa); RRV_P8=0: NHWC everywhere (A/B, same bits)
    unsigned direct_layers = 0;       // RRV_DIRECT_LAYERS: encoder convs (bit i = vgg conv i: 1 conv1_2 .. 8 conv4_1) of the per-frame path that run the direct-form kernel
    int ms_group = 0;                 // rrv_set_multistyle_group: frames per launch sequence of rrv_transfer_features_batch (0 = by the frame size)
    YuvSide yuv_in, yuv_out;          // YUV 4:2:0 input (run_encoder) and output (run_last) conversion
    int host_io = 0;                  // rrv_set_host_io: 0 = staged H2D / D2H copies, 1 = zero copy (kernels read / write page-locked host memory), 2 = input only, 3 = output only
    int n_cus = 256;
    int debug = 0;                    // rrv_set_debug / RRV_DEBUG: 1 = sync + check after every API call, 2 = after every kernel launch
    int fail_alloc_in = 0;            // rrv_debug_fail_alloc: the n-th next device allocation reports out-of-memory
    bool profiling = false;
    std::vector<ProfEntry> prof;
};

namespace {

// How one launch sequence runs.  The entry that knows builds it once (base_seq, slot_seq) and passes it down by reference to everything
// that launches or chooses a kernel; the request (Xfer) says what the call is, the handle keeps settings and what persists between calls.
struct Seq {
    hipStream_t stream;               // every launch of the sequence
    int slot;                         // the slot whose workspace it uses; -1: none (the preparation pass, weight packing, prepare_style)
    rrv_ctx::StateSet* set;           // the state set its kernels read ...
    int state_images;                 // ... or, > 0: image b of 0..state_images-1 reads set + b (per-image state)
    bool f43;                         // layers with an F(4x4,3x3) pack may run conv_f43_k (use_f43): the per-frame path only, the preparation pass and the unfused walks always run F(2x2,3x3)
    int share;                        // its persistent grids take 1/share of the CUs (resident_wgs)
};
// stream 0, set 0, no F(4x4), the handle's share: everything outside the per-frame path
Seq base_seq(rrv_handle h) { return Seq{h->slots[0].stream, -1, &h->sets[0], 0, false, h->grid_share}; }
// a sequence on `slot`: on the shared set 0, or (own_sets, slots 0 and 1) on the slot's own sixteen
Seq slot_seq(rrv_handle h, int slot, bool own_sets = false) {
    return Seq{h->slots[slot].stream, slot, own_sets ? h->slot_sets(slot) : &h->sets[0], 0, false, h->grid_share};
}

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            char _b[512];                                                                         \
            snprintf(_b, sizeof _b, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            h->err = _b;                                                                          \
            return _e == hipErrorOutOfMemory ? RRV_E_NOMEM : RRV_E_HIP;                           \
        }                                                                                         \
    } while (0)
#define RCHK(expr) do { int _r = (expr); if (_r != RRV_OK) return _r; } while (0)

int fail(rrv_handle h, int code, const std::string& msg) { h->err = msg; return code; }
int dmalloc(rrv_handle h, void** p, size_t bytes);

// Element indices inside one image are 32-bit in the kernels' epilogues: (H+2)(W+2) x 64 channels must stay below 2^31.
// The encoder (also run on style images) checks only that; check_frame adds the entries' minimum of 8 x 8 pixels.
int check_image_size(rrv_handle h, double H, double W, const char* who) {
    if ((H + 2) * (W + 2) * 64.0 < 2147483648.0) return RRV_OK;
    return fail(h, RRV_E_ARG, std::string(who) + ": frame too large ((H+2)*(W+2)*64 must be < 2^31)");
}
int check_frame(rrv_handle h, int H, int W, const char* who) {
    if (H < 8 || W < 8) return fail(h, RRV_E_ARG, std::string(who) + ": frames must be at least 8 x 8 pixels");
    return check_image_size(h, H, W, who);
}

int sync_all(rrv_handle h) {
    for (rrv_ctx::Slot& sl : h->slots)
        if (sl.stream) HIPCHK(hipStreamSynchronize(sl.stream));
    if (h->copy_in) HIPCHK(hipStreamSynchronize(h->copy_in));
    if (h->copy_out) HIPCHK(hipStreamSynchronize(h->copy_out));
    return RRV_OK;
}

// Every device allocation of a handle goes through here: device out-of-memory is RRV_E_NOMEM (not a generic HIP
// error), and the debug hook rrv_debug_fail_alloc makes the n-th next allocation fail that way (tests of the
// failure paths: a half-built workspace must never be used).
int dmalloc(rrv_handle h, void** p, size_t bytes) {
    *p = nullptr;
    if (h->fail_alloc_in > 0 && --h->fail_alloc_in == 0) {
        char b[160];
        snprintf(b, sizeof b, "out of device memory (injected by rrv_debug_fail_alloc) allocating %zu bytes", bytes);
        return fail(h, RRV_E_NOMEM, b);
    }
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        char b[200];
        snprintf(b, sizeof b, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return fail(h, e == hipErrorOutOfMemory ? RRV_E_NOMEM : RRV_E_HIP, b);
    }
    return RRV_OK;
}

int dalloc(rrv_handle h, const Seq& q, float** p, size_t floats, bool zero = true) {
    RCHK(dmalloc(h, (void**)p, floats * sizeof(float)));
    if (zero) HIPCHK(hipMemsetAsync(*p, 0, floats * sizeof(float), q.stream));
    return RRV_OK;
}

// ---- bounds-checked debug mode (rrv_set_debug) -------------------------------------------------------------------
// Every ring-layout tensor is allocated between two guard bands filled with a canary; after every API call (level 1)
// or every kernel launch (level 2) the stream is synchronised (an asynchronous fault is reported with the kernel's
// name) and every live tensor of the handle is verified: guard bands intact, the one-pixel zero ring and the slack
// rows behind the last image still zero (the kernels rely on both and must never store outside the valid pixels).
constexpr size_t DBG_GUARD = 16384;                 // floats per guard band (64 KB)
constexpr uint32_t DBG_CANARY = 0xDEADBEEFu;
struct DbgRec { rrv_ctx* h; float* base; int B, H, W, C; size_t floats; };
std::mutex g_dbg_mu;
std::map<float*, DbgRec> g_dbg;

__global__ void dbg_check_k(const float* base, const float* p, int B, int H, int W, int C, size_t floats, unsigned* counters) {
    const uint32_t* gb = (const uint32_t*)base;
    const uint32_t* u = (const uint32_t*)p;
    const size_t img = (size_t)(H + 2) * (W + 2) * C;
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    unsigned bad_guard = 0, bad_ring = 0;
    for (size_t i = tid; i < DBG_GUARD; i += nth) bad_guard += (gb[i] != DBG_CANARY) + (((const uint32_t*)(p + floats))[i] != DBG_CANARY);
    // ring: rows 0 and H+1, columns 0 and W+1 of every image
    const size_t ring_px = (size_t)2 * (W + 2) + (size_t)2 * H;
    for (size_t i = tid; i < (size_t)B * ring_px * C; i += nth) {
        const size_t c = i % C, r = (i / C) % ring_px, b = i / C / ring_px;
        size_t y, x;
        if (r < (size_t)(W + 2)) { y = 0; x = r; }
        else if (r < (size_t)2 * (W + 2)) { y = H + 1; x = r - (W + 2); }
        else { const size_t q = r - 2 * (W + 2); y = 1 + (q >> 1); x = (q & 1) ? W + 1 : 0; }
        bad_ring += u[b * img + (y * (W + 2) + x) * C + c] != 0u;
    }
    for (size_t i = (size_t)B * img + tid; i < floats; i += nth) bad_ring += u[i] != 0u;     // slack behind the last image
    if (bad_guard) atomicAdd(&counters[0], bad_guard);
    if (bad_ring) atomicAdd(&counters[1], bad_ring);
}
__global__ void dbg_fill_k(uint32_t* p, size_t n, uint32_t v) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

int debug_verify(rrv_handle h, const char* where) {
    std::vector<DbgRec> recs;
    std::vector<float*> ptrs;
    {
        std::lock_guard<std::mutex> lk(g_dbg_mu);
        for (auto& kv : g_dbg) if (kv.second.h == h) { recs.push_back(kv.second); ptrs.push_back(kv.first); }
    }
    for (rrv_ctx::Slot& sl : h->slots) if (sl.stream) {
        const hipError_t e = hipStreamSynchronize(sl.stream);
        if (e != hipSuccess) return fail(h, RRV_E_HIP, std::string("debug: asynchronous fault after ") + where + ": " + hipGetErrorString(e));
    }
    if (recs.empty()) return RRV_OK;
    unsigned* d_cnt = nullptr;
    HIPCHK(hipMalloc((void**)&d_cnt, recs.size() * 2 * sizeof(unsigned)));      // the checker's own scratch: not subject to rrv_debug_fail_alloc
    HIPCHK(hipMemset(d_cnt, 0, recs.size() * 2 * sizeof(unsigned)));
    for (size_t i = 0; i < recs.size(); ++i)
        hipLaunchKernelGGL(dbg_check_k, dim3(64), dim3(256), 0, h->slots[0].stream, (const float*)recs[i].base, (const float*)ptrs[i], recs[i].B, recs[i].H, recs[i].W,
                           recs[i].C, recs[i].floats, d_cnt + 2 * i);
    std::vector<unsigned> cnt(recs.size() * 2);
    HIPCHK(hipMemcpy(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    (void)hipFree(d_cnt);
    for (size_t i = 0; i < recs.size(); ++i)
        if (cnt[2 * i] || cnt[2 * i + 1]) {
            char b[256];
            snprintf(b, sizeof b, "debug: after %s tensor [%d,%d,%d,%d] has %u guard-band words overwritten and %u non-zero ring/slack words",
                     where, recs[i].B, recs[i].H, recs[i].W, recs[i].C, cnt[2 * i], cnt[2 * i + 1]);
            return fail(h, RRV_E_DEBUG, b);
        }
    return RRV_OK;
}

void tfree(Tens* t) {
    if (t->base) {
        { std::lock_guard<std::mutex> lk(g_dbg_mu); g_dbg.erase(t->p); }
        (void)hipFree(t->base);
    } else if (t->p) {
        (void)hipFree(t->p);
    }
    t->p = nullptr; t->base = nullptr;
}

// floats of a ring-layout tensor; slack rows keep tile-overrun halo reads inside the allocation
size_t tens_floats(int B, int H, int W, int C) { return (size_t)B * (H + 2) * (W + 2) * C + (size_t)20 * (W + 2 + 20) * C; }

int talloc(rrv_handle h, const Seq& q, Tens* t, int B, int H, int W, int C) {
    tfree(t);
    t->B = B; t->H = H; t->W = W; t->C = C;
    const size_t floats = tens_floats(B, H, W, C);
    if (!h->debug) return dalloc(h, q, &t->p, floats, true);
    RCHK(dmalloc(h, (void**)&t->base, (floats + 2 * DBG_GUARD) * sizeof(float)));
    t->p = t->base + DBG_GUARD;
    hipLaunchKernelGGL(dbg_fill_k, dim3(16), dim3(256), 0, q.stream, (uint32_t*)t->base, DBG_GUARD, DBG_CANARY);
    hipLaunchKernelGGL(dbg_fill_k, dim3(16), dim3(256), 0, q.stream, (uint32_t*)(t->p + floats), DBG_GUARD, DBG_CANARY);
    HIPCHK(hipMemsetAsync(t->p, 0, floats * sizeof(float), q.stream));
    std::lock_guard<std::mutex> lk(g_dbg_mu);
    g_dbg[t->p] = DbgRec{h, t->base, B, H, W, C, floats};
    return RRV_OK;
}

template <class P, size_t N>
void plan_tfree(P& p, const TSpec<P> (&spec)[N]) { for (const TSpec<P>& s : spec) tfree(&s.of(p)); }
// The tensors of a plan's table that `chans` gives a channel count (0: not in this plan), for B images of H x W at level 0.
// Complete or empty: a failed allocation frees every tensor of the table.
template <class P, size_t N, class F>
int plan_talloc(rrv_handle h, const Seq& q, P& p, const TSpec<P> (&spec)[N], int B, int H, int W, F&& chans) {
    for (const TSpec<P>& s : spec) {
        int b = B, hh = H, ww = W, c = chans(s);
        if (!c) continue;
        s.geo(b, hh, ww, c);
        const int rc = talloc(h, q, &s.of(p), b, hh, ww, c);
        if (rc != RRV_OK) { plan_tfree(p, spec); return rc; }
    }
    return RRV_OK;
}

void stamp(rrv_handle h, const Tens* t, int B) { t->gen = h->launch_gen; t->gen_B = B; }

// grid, xcd: the persistent launches (conv(), run_last) say which grid.x and ConvP::xcd_slabs they launch, filed with the profile entry
template <typename F>
int launch(rrv_handle h, const Seq& q, const char* name, double flops, double bytes, F&& f, double flops_exec = -1.0, unsigned grid = 0, int xcd = -1) {
    if (h->profiling) {
        ProfEntry e{name, nullptr, nullptr, flops, bytes, 0.f, flops_exec < 0 ? flops : flops_exec, grid, xcd};
        HIPCHK(hipEventCreate(&e.e0)); HIPCHK(hipEventCreate(&e.e1));
        HIPCHK(hipEventRecord(e.e0, q.stream));
        f();
        HIPCHK(hipEventRecord(e.e1, q.stream));
        h->prof.push_back(e);
    } else {
        f();
    }
    HIPCHK(hipGetLastError());
    if (h->debug >= 2) return debug_verify(h, name);
    if (h->debug == 1) {
        const hipError_t e = hipStreamSynchronize(q.stream);
        if (e != hipSuccess) return fail(h, RRV_E_HIP, std::string("debug: asynchronous fault in ") + name + ": " + hipGetErrorString(e));
    }
    return RRV_OK;
}

// ---- convolution dispatch -------------------------------------------------------------
struct ConvCall {
    const Tens* in; Tens* out; const ConvW* w;
    int H, W;                 // convolution resolution
    bool ups = false; int epi = 0;
    Tens* sc_out = nullptr;   // ups only: also produce the fused 1x1 shortcut (needs w->pk_ups_sc)
    int wy0 = 0, wx0 = 0, wy1 = 0, wx1 = 0;   // transform-domain kernels: compute only output rows [wy0,wy1) x columns [wx0,wx1) (multiples of 16; all 0 = everything)
    const float* n1 = nullptr; const Tens* res = nullptr; const float* n2 = nullptr; const float* sty = nullptr;
    int B = 1;
    int ksplit = 0;                // split K (row-split kernel, a 32-cout layer): ksplit "slabs" each contract Cin/ksplit input channels into
                                   // output channels [32 s, 32 s + 32) of a [.., 32 * ksplit] tensor (partial sums, summed by sum_parts_lrelu_k)
    const float* bias = nullptr;   // override of the layer's bias (split K: [32 * ksplit] = the bias, then zeros)
    int par_bstride = 0, bias_bstride = 0; long long w_bstride = 0;      // per-image state (ConvP): floats between consecutive images' n1 / n2 / sty, bias, weights
    bool direct = false;           // the direct-form implicit-GEMM kernel (conv_mfma_k: 9 multiplies per output, no transform-domain rounding) instead of a Winograd form
    bool in_p8 = false, out_p8 = false;      // conv_f43_k only: `in` / `out` is the channel-chunk-major twin (a Tens of B * C/8 eight-channel images; conv_f43.h LAY)
    bool enc_p8 = false;           // an encoder layer of a P8 chain: use_f43 prices it with conv_f43_k's P8-input ratios (run_encoder)
};

typedef void (*ConvFn)(const ConvP&, dim3, hipStream_t);
typedef hipError_t (*AttrFn)();       // per-DEVICE opt-in for > 64 KB of dynamic LDS (run by rrv_create after hipSetDevice)
constexpr int UPW_NW = 4;      // upsample-fused form: 4 waves, 54 KB of LDS, two workgroups per CU (with the shortcut: 154 KB, one, conv_ups5.h)

// The four kernel families, each with its launch and (where it needs > 64 KB of LDS) its attribute function — of ONE instantiation each
template <int BN, int TAPS, int EPI>
void mfma_launch(const ConvP& p, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((conv_mfma_k<BN, TAPS, EPI>), grid, dim3(256), 0, s, p); }
template <int EPI, int IMG>
void wsplit_launch(const ConvP& p, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((conv_wino_split_k<EPI, IMG>), grid, dim3(512), WSPLIT_SMEM_BYTES, s, p); }
template <int EPI, int IMG>
hipError_t wsplit_attr() { return hipFuncSetAttribute((const void*)conv_wino_split_k<EPI, IMG>, hipFuncAttributeMaxDynamicSharedMemorySize, WSPLIT_SMEM_BYTES); }
template <int SC>
constexpr int upw_smem() { return SC ? Ups5Geo::SMEM : WinoGeo<UPW_NW, 1>::SMEM; }
template <int EPI, int SC, int IMG>
void upw_launch(const ConvP& p, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((conv_wino_k<EPI, 0, UPW_NW, 1, SC, IMG>), grid, dim3(UPW_NW * 64), upw_smem<SC>(), s, p); }
template <int EPI, int SC, int IMG>
hipError_t upw_attr() { return hipFuncSetAttribute((const void*)conv_wino_k<EPI, 0, UPW_NW, 1, SC, IMG>, hipFuncAttributeMaxDynamicSharedMemorySize, upw_smem<SC>()); }
template <int EPI, int LAY>
void f43_launch(const ConvP& p, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((conv_f43_k<EPI, LAY>), grid, dim3(F43Geo::NT), F43Geo::SMEM, s, p); }
template <int EPI, int LAY>
hipError_t f43_attr() { return hipFuncSetAttribute((const void*)conv_f43_k<EPI, LAY>, hipFuncAttributeMaxDynamicSharedMemorySize, F43Geo::SMEM); }

// One row per launchable instantiation: what selects it (choose_conv), then what launches it.  A row exists only for a kernel
// some caller reaches, so the library holds no other (tests/kernel_ledger.py).
//   MFMA  conv_mfma_k        direct-form implicit GEMM, keyed by the layer's BN / TAPS as well
//   WINO  conv_wino_split_k  F(2x2,3x3), row-split: every 3x3 layer with a transform-domain pack
//   UPW   conv_wino_k        the upsample-fused form; SC: with the block's 1x1 shortcut fused in (five-product form, 25 + 4 positions per 2x2 input pixels)
//   F43   conv_f43_k         F(4x4,3x3) where use_f43 says so; LAY: channel-chunk-major tensors (conv_f43.h: bit 0 input, bit 1 output)
// IMG: the instantiation that reads per-image state (grouped multi-style launches, blended frames); conv_f43_k reads par_bstride itself.
enum ConvFam { MFMA, WINO, UPW, F43 };
struct ConvRow { ConvFam fam; int BN, TAPS, EPI, SC, LAY, IMG; ConvFn fn; AttrFn attr; const char* name; };
#define MF(BN, TAPS, EPI) {MFMA, BN, TAPS, EPI, 0, 0, 0, &mfma_launch<BN, TAPS, EPI>, nullptr, "conv_mfma<" #BN "," #TAPS "," #EPI ">"}
#define WS(EPI, IMG) {WINO, 32, 9, EPI, 0, 0, IMG, &wsplit_launch<EPI, IMG>, &wsplit_attr<EPI, IMG>, "conv_wino<" #EPI ">"}
#define UP(EPI, SC, IMG) {UPW, 32, SC ? 29 : 9, EPI, SC, 0, IMG, &upw_launch<EPI, SC, IMG>, &upw_attr<EPI, SC, IMG>, SC ? "conv_upw_sc<" #EPI ">" : "conv_upw<" #EPI ">"}
#define F4(EPI, LAY) {F43, 32, 9, EPI, 0, LAY, 0, &f43_launch<EPI, LAY>, &f43_attr<EPI, LAY>, LAY ? "conv_f43<" #EPI ", " #LAY ">" : "conv_f43<" #EPI ">"}
const ConvRow CONV_ROWS[] = {
    // 1x1 shortcuts of the residual blocks (evaluated before the upsample)
    MF(128, 1, 0), MF(64, 1, 0),
    // preparation pass: FilterPredictor 512->32 convs (raw outputs)
    MF(32, 9, 0),
    // direct-form encoder layers (RRV_DIRECT_LAYERS, read by rrv_create: accuracy where Decoder.norm[0] amplifies the encoder's rounding noise)
    MF(64, 9, E_RELU | E_POOL), MF(128, 9, E_RELU), MF(128, 9, E_RELU | E_POOL), MF(128, 9, E_RELU | E_NORM1),
    // encoder layers
    WS(E_RELU, 0), WS(E_RELU | E_POOL, 0),
    // decoder layers, also with per-image state: conv4_1 + Decoder.norm[0] (per image: blended frames), ResidualBlock.conv2,
    // filter_down (per image: a batched frame-mode launch without split K), the raw partial sums of a split-K launch
    WS(E_RELU | E_NORM1, 0), WS(E_RELU | E_NORM1, 1), WS(E_LRELU | E_NORM1 | E_RES_UPS | E_NORM2, 0), WS(E_LRELU | E_NORM1 | E_RES_UPS | E_NORM2, 1),
    WS(E_LRELU, 0), WS(E_LRELU, 1), WS(0, 0), WS(0, 1),
    // KernelFilter 32->512 convs with the folded dynamic filter (+ residual, + AdaIN after Filter3)
    WS(E_RES, 0), WS(E_RES, 1), WS(E_RES | E_NORM2, 0), WS(E_RES | E_NORM2, 1),
    // ResidualBlock.conv1 behind the nearest-x2 upsample (forward pass / preparation pass)
    UP(E_LRELU, 0, 0),
    // the same with the block's shortcut fused in (per-frame path); frame mode: raw conv1 output (its statistics are per frame)
    UP(E_LRELU | E_NORM1, 1, 0), UP(E_LRELU | E_NORM1, 1, 1), UP(E_LRELU, 1, 0),
    // F(4x4,3x3): the same-resolution 3x3 layers of the per-frame path with Cin, Cout >= 64, when the launch carries enough
    // frames (use_f43).  3-6x the rounding error of F(2x2,3x3) and 1.13-1.22x its rate at 8 frames per launch.
    F4(E_RELU, 0), F4(E_RELU | E_POOL, 0), F4(E_LRELU | E_NORM1 | E_RES_UPS | E_NORM2, 0),
    F4(E_RELU | E_POOL, 3), F4(E_RELU, 3),      // conv1_2, conv2_2 / conv2_1, conv3_1 .. conv3_3: P8 in, P8 out
    F4(E_RELU | E_POOL, 1),                     // conv3_4: P8 in, NHWC out (conv4_1 runs the row-split kernel)
    F4(E_LRELU | E_NORM1 | E_RES_UPS | E_NORM2, 1),      // ResidualBlock.conv2: P8 in (written by the upsample-fused conv1), NHWC out
};

// Persistent workgroups of a transform-domain launch: `occ` per CU, on the 1/share of the CUs this sequence may use
// (Seq::share: rrv_set_grid_share, look-ahead tickets: whole XCD rows, never empty).  conv() sizes its grid with it and use_f43 its rounds.
unsigned resident_wgs(rrv_handle h, const Seq& q, int occ) {
    unsigned r = (unsigned)h->n_cus * (unsigned)occ;
    if (q.share > 1) {
        r = (r / q.share) & ~7u;      // (a small / partitioned / CU-masked device: n_cus * occ / share < 8)
        if (r < 8) r = 8;
    }
    return r;
}

// Does this call run on conv_f43_k?  (Also asked by the callers that choose window alignments.)
// Mode 1 decides per layer and launch geometry.  A conv_f43_k work item is 32 x 32 pixels x 32 couts — four F(2x2,3x3)
// items — and takes 4 / base of an F(2x2,3x3) item's time (`base` = the rate ratio on a long item stream: tools/f43_bench.hip
// at sixteen 640 x 640 frames per launch with the partially filled last rounds taken out, profiles/r04_f43_bench.txt).  The
// 256 persistent workgroups run ceil(items / 256) rounds, so a launch with few items pays for F(4x4,3x3)'s coarser
// granularity: F(4x4,3x3) runs where rounds23 / (rounds43 x 4 / base) >= 1.04 — from four 640 x 640 frames per launch on
// every packed layer, from two 1152 x 1152 frames, from one where the items are long (256 channels); never on small
// frames in small batches.  The rule depends on the layer, the batch and the frame size only (not on what else is in
// flight): the same call always makes the same choice.
// enc_p8: price an encoder layer with the P8-input ratios (the chain is P8 only as a whole: run_encoder asks so first and falls back to the NHWC ones)
// Everything comes from the call that will be launched, and no tensor is read: a caller may ask before `in` / `out` are bound.
bool use_f43(rrv_handle h, const Seq& q, const ConvCall& c) {
    const ConvW& w = *c.w;
    const bool per_image = c.bias_bstride != 0 || c.w_bstride != 0;      // per-image PARAMETERS are conv_f43_k's too (par_bstride); per-image bias / weights (the folded KernelFilter convs) are not
    if (c.direct || ((c.wy0 | c.wx0 | c.wy1 | c.wx1) & 31)) return false;      // 32 x 32 pixel work items: a window must be aligned to them
    if (!q.f43 || !w.pk_f43 || !((h->f43_layers >> w.f43_bit) & 1u) || c.ups || c.ksplit > 1 || per_image || h->f43_mode == 0) return false;
    if (h->f43_mode == 2) return true;
    // Ill-conditioned state (filter_conditioning): the decoder multiplies whatever error the encoder makes, and F(4x4,3x3) on the
    // seven encoder layers makes 1.4x the error of F(2x2,3x3) (profiles/r05_parity_margin.txt: the x4-decoder weight set goes from
    // 0.73 to 1.42 of the pre-clamp bound with them, stays at 0.73 with the three decoder layers alone): the rule keeps them off.
    if (h->illcond && w.f43_bit < 7) return false;
    const double R = (double)resident_wgs(h, q, 1);      // persistent workgroups of this launch: one per CU the handle may use (rrv_create: device CU count under HSA_CU_MASK / RRV_CUS; rrv_set_grid_share / look-ahead tickets: a share of them)
    auto rounds = [&](double items) { return std::ceil(items / R); };
    const double slabs = w.Cout / 32;
    const double items43 = (double)((c.H + 31) / 32) * ((c.W + 31) / 32) * c.B * slabs, items23 = (double)((c.H + 15) / 16) * ((c.W + 15) / 16) * c.B * slabs;
    const int ci = w.Cin >= 256 ? 2 : (w.Cin >= 128 ? 1 : 0);
    static const double BASE_POOL[3] = {1.33, 1.38, 1.41}, BASE_RELU[3] = {1.29, 1.35, 1.39}, BASE_RES[3] = {1.26, 1.33, 1.38};      // round 5 (profiles/r05_f43_timeline.txt, F43_DMA=6)
    // round 6: with its input channel-chunk-major conv_f43_k is 12 % faster (run_encoder / resblock_frame feed it that way whenever the
    // consumer runs conv_f43_k; the ReLU layers also WRITE it, 32-byte pieces: profiles/r06_f43_layout.txt, tools/f43_bench.hip -DF43_LAY=1 / 3)
    static const double P8_POOL[3] = {1.47, 1.53, 1.56}, P8_RELU[3] = {1.36, 1.44, 1.52}, P8_RES[3] = {1.41, 1.48, 1.53};
    const bool p8 = w.f43_bit < 7 ? c.enc_p8 : (h->p8 & 2) != 0;
    const double base = (c.epi & E_POOL) ? (p8 ? P8_POOL : BASE_POOL)[ci] : (c.epi & E_RES_UPS) ? (p8 ? P8_RES : BASE_RES)[ci] : (p8 ? P8_RELU : BASE_RELU)[ci];
    return rounds(items23) >= 1.04 * rounds(items43) * 4.0 / base;
}

inline bool per_image_state(const ConvCall& c) { return (c.par_bstride | c.bias_bstride) != 0 || c.w_bstride != 0; }
inline int conv_ksplit(const ConvCall& c) { return c.ksplit > 1 ? c.ksplit : 1; }

const ConvRow* conv_row(ConvFam fam, const ConvCall& c, bool sc, int lay, bool img) {
    for (const ConvRow& e : CONV_ROWS)
        if (e.fam == fam && e.EPI == c.epi && e.SC == (int)sc && e.LAY == lay && e.IMG == (int)img && (fam != MFMA || (e.BN == c.w->BN && e.TAPS == c.w->taps))) return &e;
    return nullptr;
}

// The kernel that runs this call: its row of CONV_ROWS, or null with the refusal in `why`.  Like use_f43 it reads the call and the
// layer's packs, never a tensor.  F(4x4,3x3) where use_f43 says so, else the layer's transform-domain form where it has the pack,
// else the direct form.
const ConvRow* choose_conv(rrv_handle h, const Seq& q, const ConvCall& c, std::string& why) {
    const ConvW& w = *c.w;
    const bool fuse_sc = c.ups && c.sc_out != nullptr, img = per_image_state(c);
    const int lay = (c.in_p8 ? 1 : 0) | (c.out_p8 ? 2 : 0);
    const bool ups_p8 = lay == 2 && c.ups;      // the upsample-fused kernel writes a P8 tensor through ConvP::out_p8 (no separate instantiation)
    auto refuse = [&](const char* text) { why = text; return nullptr; };
    if (fuse_sc && !w.pk_ups_sc) return refuse("conv: no shortcut-fused pack for this layer");
    const ConvRow* k = nullptr;
    bool no_img = false;
    if (use_f43(h, q, c)) {      // (an epilogue conv_f43_k does not have in any layout: the F(2x2,3x3) form)
        k = conv_row(F43, c, false, lay, false);
        if (!k && lay && conv_row(F43, c, false, 0, false)) return refuse("conv: no conv_f43_k instantiation for this layout");
    }
    if (!k && !c.direct && (c.ups ? w.pk_ups != nullptr : w.pk_wino != nullptr)) {      // every 3x3 layer with a transform-domain pack runs its Winograd form
        const ConvFam fam = c.ups ? UPW : WINO;
        k = conv_row(fam, c, fuse_sc, 0, img);
        if (!k && img) { k = conv_row(fam, c, fuse_sc, 0, false); no_img = k != nullptr; }      // (refused below, behind the refusals that came first)
    }
    const bool wino = k != nullptr;
    if (c.ksplit > 1 && !(wino && !c.ups && w.Cout == 32 && (w.Cin % (32 * c.ksplit)) == 0 && c.bias))
        return refuse("conv: split K needs the row-split kernel, a 32-cout layer, an even number of 16-channel chunks per slice and a split bias");
    if (!k && !c.ups) k = conv_row(MFMA, c, false, 0, false);
    if (!k) {
        char b[128];
        snprintf(b, sizeof b, "no conv kernel for BN=%d taps=%d ups=%d epi=%d", w.BN, w.taps, (int)c.ups, c.epi);
        return refuse(b);
    }
    if (lay && !ups_p8 && k->fam != F43) return refuse("conv: channel-chunk-major tensors are conv_f43_k's");
    if (ups_p8 && !wino) return refuse("conv: no upsample-fused kernel for this layer");
    if (img && !wino) return refuse("conv: per-image state needs a transform-domain kernel");
    if (c.ups && (c.bias_bstride || c.w_bstride)) return refuse("conv: the upsample-fused kernel shares weights and bias over the images of a launch");
    if (no_img) return refuse("conv: this layer has no per-image-state kernel");
    return k;
}

// The launch parameters of call `c` on row `k`, the geometry of its tensors checked.  win_frac: the part of the (tile-rounded) frame the window computes
int conv_params(rrv_handle h, const ConvCall& c, const ConvRow& k, ConvP& p, double& win_frac) {
    const ConvW& w = *c.w;
    const bool wino = k.fam != MFMA, f43 = k.fam == F43, fuse_sc = k.SC != 0;
    const int ks = conv_ksplit(c);
    p.in = c.in->p; p.Hi = c.in->H; p.Wi = c.in->W - (c.in_p8 ? 6 : 0); p.Cin = w.Cin;
    p.out = c.out->p; p.H = c.H; p.W = c.W; p.Cout = w.Cout; p.B = c.B;
    p.in_bstride0 = 1;
    p.wpk = f43 ? w.pk_f43 : k.fam == UPW ? (fuse_sc ? w.pk_ups_sc : w.pk_ups) : wino ? w.pk_wino : w.pk; p.bias = w.bias;
    if (fuse_sc) {
        if (c.sc_out->H != c.in->H || c.sc_out->W != c.in->W || c.sc_out->C != w.Cout) return fail(h, RRV_E_ARG, "conv: shortcut output geometry mismatch");
        p.sc_out = c.sc_out->p;
    }
    if (!p.wpk) return fail(h, RRV_E_ARG, "conv: weights not packed for this kernel");
    p.n1 = c.n1; p.n2 = c.n2; p.sty = c.sty;
    if (c.bias) p.bias = c.bias;
    p.par_bstride = c.par_bstride; p.bias_bstride = c.bias_bstride; p.w_bstride = c.w_bstride;
    if (c.out_p8 && c.ups) p.out_p8 = 1;
    if (ks > 1) {       // the [1 slab][Cin/16 chunks] weight pack read as [ks slabs][Cin/16/ks chunks]: slab s = input channel slice s
        p.Cin = w.Cin / ks; p.cstride = w.Cin; p.cin_slab_step = w.Cin / ks; p.Cout = 32 * ks;
    }
    if (c.res) { p.res = c.res->p; p.Hr = c.res->H; p.Wr = c.res->W; }
    if ((c.in_p8 ? c.in->C != 8 || c.in->B < c.B * (w.Cin / 8) : c.in->C != w.Cin) ||
        (c.out_p8 ? c.out->C != 8 || c.out->B < c.B * (w.Cout / 8) : c.out->C != w.Cout * ks)) return fail(h, RRV_E_ARG, "conv: channel mismatch");
    const int eh = c.ups ? c.H / 2 : c.H, ew = c.ups ? c.W / 2 : c.W;
    if (c.in->H != eh || c.in->W != ew + (c.in_p8 ? 6 : 0)) return fail(h, RRV_E_ARG, "conv: input geometry mismatch");      // (a P8 twin is 6 pixels wider: conv_f43.h P8_PAD)
    const int oh = (c.epi & E_POOL) ? c.H / 2 : c.H, ow = (c.epi & E_POOL) ? c.W / 2 : c.W;
    if (c.out->H != oh || c.out->W != ow + (c.out_p8 ? 6 : 0)) return fail(h, RRV_E_ARG, "conv: output geometry mismatch");
    const int TS = f43 || fuse_sc ? 32 : 16, TY = wino ? TS : 8;             // pixel tile edge of a work item (the direct form: 16 x 8)
    p.tiles_x = (c.W + TS - 1) / TS; p.tiles_y = (c.H + TY - 1) / TY;
    if (wino && c.wy1 > c.wy0 && c.wx1 > c.wx0) {      // output window (on-device crop: nothing outside it is ever read)
        if ((c.wy0 | c.wx0 | c.wy1 | c.wx1) & 15) return fail(h, RRV_E_ARG, "conv: window must be tile aligned");
        int wy0 = c.wy0, wx0 = c.wx0, wy1 = c.wy1, wx1 = c.wx1;
        if (fuse_sc) {      // shortcut-fused conv1: round the window out to its 32 x 32 items (the extra outputs are exact)
            wy0 &= ~31; wx0 &= ~31; wy1 = (wy1 + 31) & ~31; wx1 = (wx1 + 31) & ~31;
            if (wy1 > ((c.H + 31) & ~31)) wy1 = (c.H + 31) & ~31;
            if (wx1 > ((c.W + 31) & ~31)) wx1 = (c.W + 31) & ~31;
        }
        p.ty0 = wy0 / TS; p.tx0 = wx0 / TS;
        p.tiles_y = (wy1 - wy0) / TS; p.tiles_x = (wx1 - wx0) / TS;
        const int TD = fuse_sc ? 32 : 16;          // the shortcut-fused form computes the rounded window's tiles
        win_frac = ((double)(wy1 - wy0) * (wx1 - wx0)) / ((double)((c.H + TD - 1) / TD * TD) * ((c.W + TD - 1) / TD * TD));
    }
    return RRV_OK;
}

// The grid of the launch; a transform-domain launch also learns here whether the slabs of one pixel tile share an XCD (ConvP::xcd_slabs)
dim3 conv_grid(rrv_handle h, const Seq& q, const ConvCall& c, const ConvRow& k, ConvP& p) {
    const ConvW& w = *c.w;
    if (k.fam == MFMA) return dim3((unsigned)(p.tiles_x * p.tiles_y * c.B), (unsigned)(w.Cout / w.BN));
    // persistent workgroups (one per CU; two for the upsample-fused form), walking tiles_x*tiles_y*B*(Cout/32) work items
    const unsigned slabs = (unsigned)(w.Cout / 32) * conv_ksplit(c);
    const unsigned items = (unsigned)(p.tiles_x * p.tiles_y * c.B) * slabs;
    const unsigned resident = resident_wgs(h, q, k.SC ? Ups5Geo::OCC : c.ups ? WinoGeo<UPW_NW, 1>::OCC : 1);      // rrv_set_grid_share leaves CUs to the launches of the other stream(s)
    const unsigned gx = items < resident ? items : resident;
    // slabs of one pixel tile on one XCD (workgroup w runs on XCD w % 8): the raw tile is fetched once per XCD group
    p.xcd_slabs = (gx % 8 == 0 && (gx / 8) % slabs == 0) ? 1 : 0;
    return dim3(gx, 1);
}

// What the profile files with the launch.  flops: algorithmic = the reference's direct convolution (taps multiply-adds per output).
// flops_exec: Winograd F(2x2,3x3) needs 16 multiplies per 2x2 outputs (4 per pixel), F(4x4,3x3) 36 per 4x4 (2.25 per pixel), the upsample-fused
// form 9 (2.25 per pixel) (with the fused shortcut the five-product form: 25 + 4 positions per 4x4 outputs, 29/16 per output pixel)
struct ConvCost { double flops, flops_exec, bytes; };
ConvCost conv_cost(const ConvCall& c, const ConvRow& k, double win_frac) {
    const ConvW& w = *c.w;
    const bool fuse_sc = k.SC != 0;
    const double px = (double)c.B * c.H * c.W * win_frac, cin = w.Cin, in_px = (double)c.B * c.in->H * c.in->W;
    const int oh = (c.epi & E_POOL) ? c.H / 2 : c.H, ow = (c.epi & E_POOL) ? c.W / 2 : c.W;
    const double flops_sc = fuse_sc ? 2.0 * c.B * c.in->H * c.in->W * (double)w.Cout * cin : 0.0;
    const double per_px = k.fam == F43 ? 2.25 : k.fam == UPW ? (fuse_sc ? 29.0 / 16.0 : 2.25) : k.fam == WINO ? 4.0 : (double)w.taps;
    return {2.0 * px * w.Cout * cin * w.taps + flops_sc, 2.0 * px * w.Cout * cin * per_px,
            4.0 * (in_px * cin + (double)c.B * oh * ow * w.Cout + (c.res ? (double)c.B * c.res->H * c.res->W * w.Cout : 0.0) + (double)w.Cout * cin * w.taps +
                   (fuse_sc ? in_px * w.Cout + (double)w.Cout * cin : 0.0))};
}

int conv(rrv_handle h, const Seq& q, const ConvCall& c) {
    std::string why;
    const ConvRow* k = choose_conv(h, q, c, why);
    if (!k) return fail(h, RRV_E_ARG, why);
    ConvP p{};
    double win_frac = 1.0;
    RCHK(conv_params(h, c, *k, p, win_frac));
    const dim3 grid = conv_grid(h, q, c, *k, p);
    const ConvCost cost = conv_cost(c, *k, win_frac);
    stamp(h, c.out, c.B);
    if (k->SC) stamp(h, c.sc_out, c.B);
    char nm[160];
    if (h->profiling) snprintf(nm, sizeof nm, "%s@%dx%d@%dx%d", k->name, c.w->Cin, c.w->Cout, c.H, c.W);      // "<kernel>@CinxCout@HxW": bench.py groups by the part before '@'
    const hipStream_t s = q.stream;
    return launch(h, q, h->profiling ? nm : k->name, cost.flops, cost.bytes, [&] { k->fn(p, grid, s); }, cost.flops_exec, grid.x, k->fam != MFMA ? p.xcd_slabs : -1);
}

// ---- weights ----------------------------------------------------------------------------
int upload(rrv_handle h, const Seq& q, const std::string& key, float** dst, size_t expect) {
    auto it = h->hostw.find(key);
    if (it == h->hostw.end()) return fail(h, RRV_E_WEIGHTS, "missing weight " + key);
    if (it->second.size() != expect) return fail(h, RRV_E_WEIGHTS, "wrong size for " + key);
    RCHK(dalloc(h, q, dst, expect, false));
    HIPCHK(hipMemcpyAsync(*dst, it->second.data(), expect * sizeof(float), hipMemcpyHostToDevice, q.stream));
    return RRV_OK;
}

int pack(rrv_handle h, const Seq& q, ConvW& w) {
    if (!w.pk) RCHK(dalloc(h, q, &w.pk, (size_t)w.Cout * w.Cin * w.taps, false));
    const size_t total = (size_t)w.Cout * w.Cin * w.taps;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_conv_k, dim3(blocks), dim3(256), 0, q.stream, (const float*)w.raw, w.pk, w.Cout, w.Cin, w.taps, w.BN);
    HIPCHK(hipGetLastError());
    return RRV_OK;
}

int bn_for(int cout) { return cout >= 128 ? 128 : (cout >= 64 ? 64 : 32); }

int pack_wino(rrv_handle h, const Seq& q, ConvW& w) {
    const size_t total = (size_t)w.Cout * w.Cin * 16;
    if (!w.pk_wino) RCHK(dalloc(h, q, &w.pk_wino, total, false));
    hipLaunchKernelGGL(pack_wino_k, dim3(4096), dim3(256), 0, q.stream, (const float*)w.raw, w.pk_wino, w.Cout, w.Cin, 0);
    HIPCHK(hipGetLastError());
    return RRV_OK;
}

int pack_f43(rrv_handle h, const Seq& q, ConvW& w) {
    const size_t total = (size_t)w.Cout * w.Cin * 36;
    if (!w.pk_f43) RCHK(dalloc(h, q, &w.pk_f43, total, false));
    hipLaunchKernelGGL(pack_f43_k, dim3(4096), dim3(256), 0, q.stream, (const float*)w.raw, w.pk_f43, w.Cout, w.Cin);
    HIPCHK(hipGetLastError());
    return RRV_OK;
}

int pack_ups(rrv_handle h, const Seq& q, ConvW& w) {
    const size_t total = (size_t)w.Cout * w.Cin * 9;
    if (!w.pk_ups) RCHK(dalloc(h, q, &w.pk_ups, total, false));
    hipLaunchKernelGGL(pack_wino_k, dim3(4096), dim3(256), 0, q.stream, (const float*)w.raw, w.pk_ups, w.Cout, w.Cin, 1);
    HIPCHK(hipGetLastError());
    return RRV_OK;
}

// the ResidualBlock's conv1 pack for the five-product form, with the block's 1x1 shortcut (conv_ups5.h)
int pack_ups_sc(rrv_handle h, const Seq& q, ConvW& w, const ConvW& sc) {
    if (sc.Cout != w.Cout || sc.Cin != w.Cin || sc.taps != 1) return fail(h, RRV_E_WEIGHTS, "shortcut / conv1 shape mismatch");
    const size_t total = (size_t)w.Cout * w.Cin * Ups5Geo::NUB;
    if (!w.pk_ups_sc) RCHK(dalloc(h, q, &w.pk_ups_sc, total, false));
    hipLaunchKernelGGL(pack_ups5_k, dim3(4096), dim3(256), 0, q.stream, (const float*)w.raw, (const float*)sc.raw, w.pk_ups_sc, w.Cout, w.Cin);
    HIPCHK(hipGetLastError());
    return RRV_OK;
}

int make_conv(rrv_handle h, const Seq& q, const std::string& prefix, int cout, int cin, int taps, bool has_bias, bool do_pack = true) {
    ConvW w;
    w.Cout = cout; w.Cin = cin; w.taps = taps; w.BN = bn_for(cout);
    RCHK(upload(h, q, prefix + ".weight", &w.raw, (size_t)cout * cin * taps));
    if (has_bias) RCHK(upload(h, q, prefix + ".bias", &w.bias, (size_t)cout));
    else w.bias = h->zero_bias;
    if (do_pack) RCHK(pack(h, q, w));
    if (do_pack && taps == 9 && cin >= 64 && cout >= 64) RCHK(pack_wino(h, q, w));
    h->conv[prefix] = w;
    return RRV_OK;
}

// ---- statistics helpers -----------------------------------------------------------------
// mode 0: out[C] = mean;  mode 1: out = norm params [4][C];  mode 2: out = style (mean,std) [2][C]
int chan_stats(rrv_handle h, const Seq& q, const Tens& t, int mode, float* out) {
    const long npix = (long)t.B * t.H * t.W;
    int nblk = (int)((npix + 255) / 256);        // small tensors (frame mode, B = 1) still get a few dozen workgroups
    if (nblk > 1024) nblk = 1024;
    if (nblk < 1) nblk = 1;
    const int ppb = (int)((npix + nblk - 1) / nblk);
    // scratch shared by all calls: they are ordered on q.stream (1024 partial blocks x 3 x 512 channels at most)
    if (t.C > 512) return fail(h, RRV_E_ARG, "chan_stats: more than 512 channels");
    double* part = h->stat_part;
    float* mean = h->stat_mean;
    StatP sp{t.p, t.B, t.H, t.W, t.C, nullptr, part, 0, ppb};
    const int fb = (t.C + 15) / 16;
    RCHK(launch(h, q, "chan_stat", 0, 0, [&] { hipLaunchKernelGGL(chan_stat_k, dim3(nblk), dim3(256), 0, q.stream, sp); }));
    RCHK(launch(h, q, "chan_final", 0, 0, [&] {
        hipLaunchKernelGGL(chan_final_k, dim3(fb), dim3(256), 0, q.stream, (const double*)part, nblk, t.C, (double)npix, 0,
                           (const float*)nullptr, mode == 0 ? out : mean);
    }));
    if (mode != 0) {
        sp.pass = 1; sp.mean = mean;
        RCHK(launch(h, q, "chan_stat", 0, 0, [&] { hipLaunchKernelGGL(chan_stat_k, dim3(nblk), dim3(256), 0, q.stream, sp); }));
        RCHK(launch(h, q, "chan_final", 0, 0, [&] {
            hipLaunchKernelGGL(chan_final_k, dim3(fb), dim3(256), 0, q.stream, (const double*)part, nblk, t.C, (double)npix, mode,
                               (const float*)mean, out);
        }));
    }
    return RRV_OK;
}

// par_bstride > 0: image b of x normalises with mean / scale / smean / sstd + b * par_bstride (batched frame mode)
int pointwise(rrv_handle h, const Seq& q, const Tens& x, Tens& y, const float* mean, const float* scale, bool div, const Tens* res,
              int res_mode, const float* smean, const float* sstd, const float* lo = nullptr, const float* hi = nullptr, long par_bstride = 0) {
    PointP p{x.p, y.p, x.B, x.H, x.W, x.C, mean, scale, div ? 1 : 0, res ? res->p : nullptr, res_mode,
             res ? res->H : 0, res ? res->W : 0, smean, sstd, lo, hi, 1, par_bstride};
    // image rows x segments per row: ~4 float4 per thread, at most 16384 blocks (further rows are strided)
    int rows = x.B * x.H;
    int segs = (x.W * (x.C / 4) + 1023) / 1024;
    if (segs < 1) segs = 1;
    while (rows * segs > 16384 && segs > 1) --segs;
    if (rows * segs > 16384) rows = 16384 / segs;
    p.segs = segs;
    const int blocks = rows * segs;
    stamp(h, &y, x.B);
    return launch(h, q, "pointwise", 0, 0, [&] { hipLaunchKernelGGL(pointwise_k, dim3(blocks), dim3(256), 0, q.stream, p); });
}
// y = x normalised with the saved statistics norm[n] of state `st` (no clamp) [+ res, upsampled 2x] [* style std + style mean of entry sty]
int apply_norm(rrv_handle h, const Seq& q, const Tens& x, Tens& y, const float* st, int n, const Tens* res = nullptr, int sty = -1, long par_bstride = 0) {
    const float* m = st + SL.norm[n];
    const float* s = sty < 0 ? nullptr : st + SL.sty[sty];
    return pointwise(h, q, x, y, m, m + x.C, false, res, res ? 2 : 0, s, s ? s + x.C : nullptr, nullptr, nullptr, par_bstride);
}

// ---- folded KernelFilter weights for a state blob ------------------------------------------
// (both folded layers run the row-split transform-domain kernel everywhere — per-frame path and compute()'s frame-0
// residual alike — so only the Winograd packs are built)
// nsets > 1: the state sets q.set, q.set + 1, .. (blobs RRV_STATE_FLOATS apart, folded weights set-major) in one launch each —
// a set's packed 32-cout slabs follow the previous set's, so the pack is the pack of a layer with nsets x the couts.
int fold_filters(rrv_handle h, const Seq& q, const float* blob, int f /*0..2*/, int nsets = 1) {
    char pre[64];
    snprintf(pre, sizeof pre, "Decoder.Filter%d", f + 1);
    const ConvW& wd = h->conv[std::string(pre) + ".down_sample.0"];
    const ConvW& wu = h->conv[std::string(pre) + ".upsample.0"];
    ConvW& fd = q.set->fold_down[f];
    ConvW& fu = q.set->fold_up[f];
    h->slots[(q.set - h->sets) / rrv_ctx::MS_GROUP_MAX].set_images = 0;      // the slot's sets are being rewritten; a per-image-state launch counts its images once it is queued
    for (int i = 0; i < nsets; ++i) q.set[i].folded |= 1u << f;
    const float* F1 = blob + SL.filt[2 * f];
    const float* F2 = blob + SL.filt[2 * f + 1];
    hipLaunchKernelGGL(fold_down_k, dim3((32 * 512 * 9 + 255) / 256, nsets), dim3(256), 0, q.stream, F1, (const float*)wd.raw,
                       (const float*)wd.bias, fd.raw, fd.bias, 512 * 9, (int)RRV_STATE_FLOATS, 256);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fold_up_k, dim3((512 * 32 * 9 + 255) / 256, nsets), dim3(256), 0, q.stream, F2, (const float*)wu.raw, fu.raw, 512, (int)RRV_STATE_FLOATS);
    HIPCHK(hipGetLastError());
    if (nsets == 1) {
        RCHK(pack_wino(h, q, fd));          // 512->32 is one Winograd cout slab
        RCHK(pack_wino(h, q, fu));          // 32 input channels = two 16-channel chunks per work item
    } else {
        hipLaunchKernelGGL(pack_wino_k, dim3(4096), dim3(256), 0, q.stream, (const float*)fd.raw, fd.pk_wino, 32 * nsets, 512, 0);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pack_wino_k, dim3(4096), dim3(256), 0, q.stream, (const float*)fu.raw, fu.pk_wino, 512 * nsets, 32, 0);
        HIPCHK(hipGetLastError());
    }
    return RRV_OK;
}

// The blend step of every blended entry: state sets q.set, q.set + 1, .. of images 0..cnt-1 := sum_s w[image][s] x the computed state of
// style s (blend_sets_k), their three KernelFilters folded; the sets then hold a blend (active_src -2).  w: [cnt][ns] host weights, read
// before this returns (they travel in the kernel argument); w_dev: the same array in HBM, read by the kernel on q.stream.
int blend_sets(rrv_handle h, const Seq& q, const float* w, bool w_dev, int ns, int cnt) {
    static_assert(rrv_ctx::MS_GROUP_MAX <= 16, "BlendSetsP::w holds sixteen images");
    h->active_src = -2;      // from here on, whatever happens: the next global entry re-activates its style
    BlendSetsP bp{};
    bp.n = ns; bp.out = q.set->active; bp.count = RRV_STATE_FLOATS;
    for (int s = 0; s < ns; ++s) bp.st[s] = h->styles[s].blob;
    if (w_dev) bp.w_dev = w;
    else for (int g = 0; g < cnt; ++g) memcpy(bp.w[g], w + (size_t)g * ns, sizeof(float) * ns);
    hipLaunchKernelGGL(blend_sets_k, dim3((RRV_STATE_FLOATS + 255) / 256, cnt), dim3(256), 0, q.stream, bp);
    HIPCHK(hipGetLastError());
    for (int f = 0; f < 3; ++f) RCHK(fold_filters(h, q, q.set->active, f, cnt));
    return RRV_OK;
}

// Conditioning of a style's saved state, read off its six dynamic 32 x 32 filters (FilterPredictor outputs): every state seen
// so far with seeded or real inputs has filters of Frobenius norm 5.5 .. 5.8 (~ sqrt 32: near-orthogonal), while the weight set
// built to be ill-conditioned in float32 (every decoder weight x 4; the reference's own float32 run misses its float64 run by
// 30x the state bound) reaches 2e2 .. 3e6.  Above 4 x sqrt 32 the state counts as ill-conditioned.
int filter_conditioning(rrv_handle h, StyleState& S) {
    std::vector<float> f(6 * 1024);
    HIPCHK(hipMemcpy(f.data(), S.blob + SL.filt[0], f.size() * sizeof(float), hipMemcpyDeviceToHost));
    double worst = 0.0;
    for (int k = 0; k < 6; ++k) {
        double ss = 0.0;
        for (int i = 0; i < 1024; ++i) ss += (double)f[k * 1024 + i] * f[k * 1024 + i];
        worst = std::sqrt(ss) > worst ? std::sqrt(ss) : worst;
    }
    S.illcond = !(worst <= 4.0 * std::sqrt(32.0));      // (NaN counts as ill-conditioned)
    h->illcond = false;
    for (StyleState& t : h->styles) h->illcond = h->illcond || (t.computed && t.illcond);
    return RRV_OK;
}

int activate_state(rrv_handle h, int style_id) {
    if (h->active_src == style_id) return RRV_OK;
    RCHK(sync_all(h));
    const Seq q = base_seq(h);      // the shared set 0
    StyleState& s = h->styles[style_id];
    HIPCHK(hipMemcpyAsync(q.set->active, s.blob, RRV_STATE_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, q.stream));
    for (int f = 0; f < 3; ++f) RCHK(fold_filters(h, q, q.set->active, f));
    HIPCHK(hipStreamSynchronize(q.stream));
    h->active_src = style_id;
    h->user_style = style_id;
    return RRV_OK;
}

// Plain (non-blend) transfer entries: after a blend (-2) or an invalidation (-1) go back to the style that was
// active before it — the last one activated by compute() / set_state() — else the first computed one.
int ensure_active(rrv_handle h) {
    if (h->active_src >= 0) return RRV_OK;
    int sid = -1;
    if (h->user_style >= 0 && h->styles[h->user_style].computed) sid = h->user_style;
    else
        for (int s = 0; s < RRV_MAX_STYLES && sid < 0; ++s)
            if (h->styles[s].computed) sid = s;
    h->active_src = -1;
    if (sid < 0) return RRV_OK;        // transfer_device reports "state not computed"
    return activate_state(h, sid);
}

// ---- encoder ----------------------------------------------------------------------------
void enc_free(EncPlan& e) {
    plan_tfree(e, ENC_T);
    e.B = e.H = e.W = 0;
}

// A channel-chunk-major image of C channels spans (H+2)*(W+8)*C floats (rows pitched W + 8: conv_f43.h P8_PAD), more than the
// (H+2)*(W+2)*64 of the frame-size guards; conv_f43_k's P8 store offsets are 32-bit within an image.  A tensor has a P8 twin only
// when its image stays below 2^31 floats; otherwise the launch keeps NHWC (the same values, which run beyond the 2 GiB mark).
bool p8_fits(int H, int W, int C) { return (double)(H + 2) * (W + 8) * C < 2147483648.0; }

// A plan is either complete or empty: the geometry is recorded only after every tensor exists; a failed allocation
// releases what was built so far, and the next call with the same geometry starts over (it must never find a
// half-built plan that passes the cache test and launch kernels on null tensors).
// per_frame: a plan of the per-frame path (Slot::enc), which gets the P8 twins where the chain may run
int enc_plan(rrv_handle h, const Seq& q, EncPlan& e, int B, int H, int W, bool per_frame = false) {      // grow-only in B: a plan made for more images serves fewer
    if (e.B >= B && e.H == H && e.W == W && e.c41.p) return RRV_OK;
    RCHK(check_image_size(h, H, W, "encoder"));
    enc_free(e);
    const bool twins = per_frame && (h->p8 & 1) && p8_fits(H, W, 64) && p8_fits(H / 2, W / 2, 128) && p8_fits(H / 4, W / 4, 256);
    RCHK(plan_talloc(h, q, e, ENC_T, B, H, W, [&](const TSpec<EncPlan>& s) { return (s.flags & TS_P8) && !twins ? 0 : s.C; }));
    e.B = B; e.H = H; e.W = W;
    return RRV_OK;
}

// the plan of `slot` for (B, H, W): a resident one that fits, else the emptier / least recently used of the two
template <class Plan>
Plan& pick_plan(rrv_handle h, Plan (&v)[2], int B, int H, int W) {
    int k = -1;
    for (int i = 0; i < 2; ++i) if (v[i].H == H && v[i].W == W && v[i].B >= B) k = i;
    if (k < 0) for (int i = 0; i < 2; ++i) if (v[i].H == H && v[i].W == W) k = i;        // same size, more images: grow it
    if (k < 0) for (int i = 0; i < 2; ++i) if (v[i].B == 0) { k = i; break; }
    if (k < 0) k = v[0].stamp <= v[1].stamp ? 0 : 1;
    v[k].stamp = ++h->plan_clock;
    return v[k];
}

// vgg19.features[0:21] on a device-resident uint8 BGR image.  which: 0 Encoder (grey), 1 EncoderStyle (colour).
// norm0 != nullptr fuses Decoder.norm[0] into the last conv (per-frame path).
// unpadded source frame behind a padded geometry (ReshapeTool on the device): pad on the way in, crop on the way out
struct PadCrop { int src_H, src_W, top, left; };

// What a launch of a YUV form takes from one direction's state: the twelve coefficients, the shift between a code and a stored sample (P016
// keeps the code in the high bits) and the largest code.  wide: a uint16 form; msb: P016.
struct YuvLaunch { float m[12]; int shift; float hi; };
YuvLaunch yuv_launch_params(const YuvSide& s, bool input, bool wide, bool msb) {
    YuvLaunch l;
    const int d = wide ? s.bits : 8;      // (8 bits: shift 0, hi 255 — the 8-bit kernels read neither)
    if (!wide) memcpy(l.m, s.m8, sizeof l.m);
    else if (s.set16) memcpy(l.m, s.m16, sizeof l.m);
    else (void)(input ? rrv_yuv_input_matrix_depth : rrv_yuv_matrix_depth)(RRV_YUV_BT601, 0, d, l.m);
    l.shift = msb ? 16 - d : 0; l.hi = (float)((1 << d) - 1);
    return l;
}

// in: the format of the images at d_img.  nb: images to encode (plans are grow-only, so a plan may hold room for more)
// out41 != nullptr: the relu4_1 tensor is written THERE ([nb] ring-layout images, zero ring) instead of the plan's c41 (feature cache)
// norm0_bstride != 0: image b's Decoder.norm[0] entry is norm0 + b * norm0_bstride (per-image state sets)
// iv: where the rows of the source frames are (null: contiguous frames, whose view is built here — conv_first_k addresses every frame through one)
int run_encoder(rrv_handle h, const Seq& q, EncPlan& e, const uint8_t* d_img, InFmt in, int which, const float* norm0, const PadCrop* pc, int nb, Tens* out41 = nullptr,
                int norm0_bstride = 0, const ImgView* iv = nullptr) {
    const int H = e.H, W = e.W, B = nb;
    if (nb < 1 || nb > e.B) return fail(h, RRV_E_ARG, "run_encoder: batch does not fit the plan");
    RCHK(check_image_size(h, H, W, "encoder"));
    auto D_ = [&](int i) { return which == 0 && q.f43 && ((h->direct_layers >> i) & 1u) != 0; };
    auto call = [&](int i, bool p8) {      // the call of VGG conv i (1..8) in the NHWC or the P8 chain
        const EncLayer& l = ENC_LAYERS[i - 1];
        ConvCall k{&(e.*(p8 ? l.qin : l.in)), &(e.*(p8 ? l.qout : l.out)), &h->conv[enc_key(which, i)], H >> l.level, W >> l.level};
        k.B = B; k.epi = l.epi; k.direct = D_(i);
        if (p8) { k.in_p8 = k.enc_p8 = l.qin != l.in; k.out_p8 = l.qout != l.out; }
        return k;
    };
    // Channel-chunk-major tensors (conv_f43.h LAY) between the seven packed layers when ALL of them run conv_f43_k in this launch (the rule
    // of use_f43 says yes for every launch with enough work items: the batched entries); any other mix keeps NHWC throughout.  Where every
    // level is a multiple of 32 pixels wide the choice changes no bit of the result (conv_f43_k stages the same bytes from either layout);
    // elsewhere the edge tiles see other discarded columns (conv_f43.h P8_PAD): rounding noise, GPU test.  Only a plan with the twins
    // (enc_plan) can run the chain.
    // priced as a P8 chain first; if one layer then prefers F(2x2,3x3) the chain is NHWC and every layer is priced again as such (in conv())
    bool p8 = which == 0 && q.f43 && e.q11.p != nullptr;
    for (int i = 1; i <= 7 && p8; ++i) p8 = use_f43(h, q, call(i, true));
    const int inf = in.form;         // (the style encoder reads the same forms, in colour: rrv_prepare_style_image_device)
    FirstP fp{d_img, H, W, B, p8 ? e.q11.p : e.c11.p, h->first_w[which], h->first_b[which], which == 0 ? 1 : 0, (W + 15) / 16, (H + 15) / 16,
              which == 0 ? h->first_wg : nullptr, pc ? pc->src_H : 0, pc ? pc->src_W : 0, pc ? pc->top : 0, pc ? pc->left : 0, p8 ? 1 : 0,
              in.space};
    fp.v = iv ? *iv : contiguous_view(in_view_layout(inf), pc ? pc->src_H : H, pc ? pc->src_W : W, in.cs);
    stamp(h, p8 ? &e.q11 : &e.c11, B);
    if (in_yuv(inf)) {
        const YuvLaunch y = yuv_launch_params(h->yuv_in, true, in_yuv16(inf), inf == IN_YUV_P016);
        memcpy(fp.yuv_n, y.m, sizeof fp.yuv_n); fp.yuv_shift = y.shift;
        fp.csx = chroma_sx(in.cs); fp.csy = chroma_sy(in.cs);
    }
    static void (*const first_k[IN_FORMS])(FirstP) = {conv_first_k<IN_U8_HWC>, conv_first_k<IN_U8_CHW>, conv_first_k<IN_F32_HWC>, conv_first_k<IN_F32_CHW>,
                                                      conv_first_k<IN_YUV_I420>, conv_first_k<IN_YUV_NV12>, conv_first_k<IN_YUV_I420_16>, conv_first_k<IN_YUV_P016>};
    RCHK(launch(h, q, "conv_first", 2.0 * B * H * W * 27 * 64, ((in_yuv(inf) ? yuv_samples_per_pixel(in.cs) * in_elem(inf) : 3.0 * in_elem(inf)) + 256.0) * B * H * W, [&] {
        hipLaunchKernelGGL(first_k[inf], dim3(fp.tiles_x * fp.tiles_y * B), dim3(256), 0, q.stream, fp);
    }));
    for (int i = 1; i <= 8; ++i) {
        ConvCall c = call(i, p8);
        if (i == 8) {      // conv4_1: the caller's output, Decoder.norm[0] fused in
            if (out41) c.out = out41;
            if (norm0) { c.epi |= E_NORM1; c.n1 = norm0; c.par_bstride = norm0_bstride; }
        }
        RCHK(conv(h, q, c));
    }
    return RRV_OK;
}

// Format of a stylized frame: OUT_F32 = float32 BGR in 0..255 (tensor2numpy), OUT_U8 = the same values rounded half to even
// on the GPU (conv_last_k<true>: cv2.imwrite's / driver.to_uint8's conversion) — the rrv_*_u8 entries.  Elements per frame are
// the same; only their size differs.  rrv_transfer_image_device adds planar RGB (chw) and the UNIT / NORM spaces (float32 only).
// yuv = RRV_LAY_I420 / RRV_LAY_NV12 (else 0): 8-bit YUV 4:2:0 of the PIXEL values (conv_last_k's YUV form, the rrv_*_yuv entries); a
// frame is then Xfer::out_bytes() bytes, not elements x element size.  yuv = RRV_LAY_I420_16 / RRV_LAY_P016: the same in uint16 samples, 10 / 12 /
// 16-bit codes (conv_last_k's Y16 instantiation), two bytes per sample.
// A YUV layout value is one of the four base layouts, alone (4:2:0) or with ONE of the chroma flags RRV_LAY_422 / RRV_LAY_444.  OutFmt::yuv holds
// the BASE layout and OutFmt::cs the chroma format (CS_*); the kernels see the latter only as LastP::csx / csy and through the view.
struct OutFmt { bool u8, chw; int space; int yuv = 0; int cs = CS_420; };
constexpr int LAY_CHROMA = RRV_LAY_422 | RRV_LAY_444;
constexpr int yuv_base(int layout) { return layout & ~LAY_CHROMA; }
constexpr int yuv_chroma(int layout) { return (layout & RRV_LAY_444) ? CS_444 : (layout & RRV_LAY_422) ? CS_422 : CS_420; }      // of a layout yuv_layout() accepts
constexpr bool yuv16_layout(int layout) { return yuv_base(layout) == RRV_LAY_I420_16 || yuv_base(layout) == RRV_LAY_P016; }  // of a layout yuv_layout() accepts, or a base
constexpr bool yuv_layout(int layout) {      // both flags, a flag on a non-YUV base and every value that names nothing: false
    return (layout & LAY_CHROMA) != LAY_CHROMA &&
           (yuv_base(layout) == RRV_LAY_I420 || yuv_base(layout) == RRV_LAY_NV12 || yuv_base(layout) == RRV_LAY_I420_16 || yuv_base(layout) == RRV_LAY_P016);
}
inline size_t yuv_sample_bytes(OutFmt f) { return yuv16_layout(f.yuv) ? sizeof(uint16_t) : 1; }
constexpr OutFmt OUT_F32{false, false, SP_PIXEL}, OUT_U8{true, false, SP_PIXEL};
inline size_t out_elem(OutFmt f) { return f.u8 ? 1 : sizeof(float); }
// How one launch sequence reads and writes its frames: both formats and, for the pad geometry, the source window (nullptr: plain frames)
// iv, ov: the views of the frames as passed / as delivered (null: contiguous; run_encoder / run_last build that view)
// caller: the stream of the caller the sequence is ordered with (its work so far precedes the first launch, it waits for the last), if any
struct CallerOrder { hipStream_t stream = nullptr; bool sync = false; };
struct FrameIO { InFmt in; OutFmt out; const PadCrop* pc = nullptr; const ImgView* iv = nullptr; const ImgView* ov = nullptr; CallerOrder caller; };
inline int out_view_layout(OutFmt f) { return f.yuv ? (f.yuv == RRV_LAY_I420 || f.yuv == RRV_LAY_I420_16 ? VL_I420 : VL_NV12) : f.chw ? VL_CHW : VL_HWC; }
inline size_t out_view_elem(OutFmt f) { return f.yuv ? yuv_sample_bytes(f) : out_elem(f); }      // bytes per element of an output view
inline ImgView img_view(const rrv_image_view& v) {
    return ImgView{v.frame_stride, {v.plane_offset[0], v.plane_offset[1], v.plane_offset[2]},
                   {(uint32_t)v.pitch[0], (uint32_t)v.pitch[1], (uint32_t)v.pitch[2]}};      // (a checked view: every pitch is below 2^31)
}

int padded_size(int n) { return (n + 128 + 63) / 64 * 64; }      // ReshapeTool.process, generate_real_video.py:66-76

// One transfer as an entry states it, both formats and the caller's stream included (in, fmt, with): what the call is lives here, how its launch
// sequences run in their Seq, and the handle keeps only settings and what persists between calls.  The model is named, never inferred from which pointer is set; everything the entries derive from the request
// (kernel geometry, bytes and elements per frame, the pad and crop window) is computed here and nowhere else.
//   GLOBAL: Stylization(use_Global=True), one shared state set          FRAME: use_Global=False, statistics per frame
//   BLEND:  frame b with sum_s wts[b][s] x the state of style s         MASK:  the styles blended per pixel by float32 masks
enum class Model { GLOBAL, FRAME, BLEND, MASK };
constexpr bool PLAIN = false, PADDED = true;      // Xfer::pad
struct Xfer {
    Model model;
    int B, H, W;                    // as the caller passed them
    bool pad;                       // the _frames / RRV_TF_PAD_CROP geometry: UNPADDED frames in and out, the reference driver's reflect padding
                                    // (64 px + up to a multiple of 64) and crop (:61-83, :167) happen inside the first and last kernel
    OutFmt fmt;
    int ns = 0;                     // BLEND, MASK: styles 0..ns-1
    const float* wts = nullptr;     // BLEND: [B][ns]; in host memory unless w_dev
    const float* mask = nullptr;    // MASK: [mask_images][ns][H][W], mask_images = B, or 1 = one mask for every frame
    int mask_images = 0;
    bool w_dev = false;             // BLEND: wts is in HBM, written by work the slot's stream is ordered behind
    InFmt in = IN_BGR8;             // format of the content frames (the descriptor and _from_yuv entries set it)
    const float* const* feats = nullptr;      // BLEND: one cached relu4_1 feature per image in place of the frames (d_in may then be null)
    // Where the frames are (the view entries set these after rrv_image_view_check; null: contiguous frames).  run_xfer turns either into
    // the ImgView both kernels address by, and walks the launch groups by its frame stride.
    const rrv_image_view* vin = nullptr;
    const rrv_image_view* vout = nullptr;
    // The scaled entries: the frames as passed are SH x SW and are resampled to the H x W working frame in front of everything else
    // (run_xfer), so H, W and all that derives from them keep describing the working frame.  0: not scaled, the frames are H x W.
    int SH = 0, SW = 0;
    // A delivered size: the stylized working frame (WH x WW below) is resampled to DH x DW behind the last kernel (run_xfer), and `fmt`, `vout`
    // and everything sized by the output describe DH x DW frames.  0, or equal to the working frame: the working frame is delivered.
    int DH = 0, DW = 0;
    // Guided delivery (include/rerevst_hip.h "Guided delivery"): radius in working pixels (0: plain delivery) and eps of a 0..1 image.  The stylized
    // working frame then reaches DH x DW through gf_coeff_k / gf_apply_k with the call's own source frames as the guide, equal sizes included.
    int gr = 0; float geps = 0.f;
    // Compositing (include/rerevst_hip.h "Compositing"; set_composite): the delivered float32 frame is mixed with the call's own source at the
    // delivered size before it reaches the output form.  cstr: one strength per frame of THIS request in host memory (null: 1); cmatte:
    // [cm_frames][OH][OW] in HBM (null: none), cm_frames 1 or B.  comp unset: nothing is composited and nothing of this is read.
    bool comp = false;
    const float* cstr = nullptr; const void* cmatte = nullptr;
    int cm_dt = RRV_DT_F32, cm_frames = 0, ckeep = RRV_KEEP_NONE;
    // JPEG output (include/rerevst_hip.h "JPEG output"; set_jpeg): the delivered float32 frame is encoded where the delivery stage would
    // write the output form.  d_out is then the slots (frame b at b * jp->cap bytes) and jp_sizes the B sizes, both in HBM.
    const JpegP* jp = nullptr; int* jp_sizes = nullptr;
    // Order this call with the stream `with` (view_run's hip_stream / RRV_TF_ON_STREAM); unset: rrv_set_caller_stream's setting (order())
    bool on_stream = false; hipStream_t with = nullptr;
    // The picture area (include/rerevst_hip.h "Picture area"; the rrv_transfer_picture entries set it once, run_xfer reads it): the frames as
    // passed and as delivered are FH x FW, and everything above describes the WINDOW (py0, px0, SH x SW) of them as a compositing request
    // with DH x DW = SH x SW: vin is the window's view.  vfull / vout are the views of the whole frames, in and out.  run_xfer fills a
    // float32 canvas from the whole source, lets the request write the window of it, and delivers the canvas at equal size.
    bool pic = false;
    int py0 = 0, px0 = 0, FH = 0, FW = 0;
    const rrv_image_view* vfull = nullptr;

    bool scaled() const { return SH != 0 || SW != 0; }
    int IH() const { return scaled() ? SH : H; }              // the frame as passed
    int IW() const { return scaled() ? SW : W; }
    int WH() const { return pad ? H : H / 8 * 8; }            // the stylized working frame: what the last kernel delivers
    int WW() const { return pad ? W : W / 8 * 8; }
    bool delivering() const { return (DH != 0 || DW != 0) && (DH != WH() || DW != WW()); }
    bool guided() const { return gr != 0; }
    bool staged() const { return delivering() || guided() || comp || jp; }  // the last kernel writes the slot's buffer of working frames, not the caller's frames
    bool indirect() const { return staged() || pic; }                        // the caller's frames are written by a stage behind the model, not by its last kernel
    int OH() const { return delivering() ? DH : WH(); }       // the frame delivered
    int OW() const { return delivering() ? DW : WW(); }
    ImgView in_view() const { return vin ? img_view(*vin) : contiguous_view(in_view_layout(in.form), IH(), IW(), in.cs); }
    ImgView out_view() const { return vout ? img_view(*vout) : contiguous_view(out_view_layout(fmt), OH(), OW(), fmt.cs); }
    int KH() const { return pad ? padded_size(H) : H; }      // the geometry the kernels run
    int KW() const { return pad ? padded_size(W) : W; }
    size_t in_bytes() const { return pic ? in_frame_bytes(in.form, FH, FW, in.cs) : in_frame_bytes(in.form, IH(), IW(), in.cs); }                                              // per frame, in x.in
    size_t out_elems() const { return (size_t)OH() * OW() * 3; }                                                   // per frame (any input size: 8*(H/8) x 8*(W/8), or the delivered size)
    size_t out_bytes() const {                                                                                      // per frame, in x.fmt
        if (pic) return fmt.yuv ? yuv_frame_samples(FH, FW, fmt.cs) * yuv_sample_bytes(fmt) : (size_t)FH * FW * 3 * out_elem(fmt);      // the whole frame is delivered
        return fmt.yuv ? yuv_frame_samples(OH(), OW(), fmt.cs) * yuv_sample_bytes(fmt) : out_elems() * out_elem(fmt);
    }
    size_t mask_floats() const { return (size_t)ns * H * W; }                                                      // of one image's masks
    size_t matte_bytes() const { return (size_t)OH() * OW() * (cm_dt == RRV_DT_U8 ? 1 : 4); }                      // of one frame's matte
    bool src_is_rs() const { return scaled() && !delivering(); }      // comp: S is the resampled working input (the delivered frame is the working frame)
    PadCrop pad_crop() const { return PadCrop{H, W, 64, 64}; }
    CallerOrder order(rrv_handle h) const { return on_stream ? CallerOrder{with, true} : CallerOrder{h->caller_stream, h->caller_sync}; }
};

// grow-only device buffer of at least n elements (h->d_u8, a staging set's masks); empty after a failed allocation
template <class T>
int ensure_dev(rrv_handle h, T*& p, size_t& cap, size_t n) {
    if (cap >= n) return RRV_OK;
    if (p) (void)hipFree(p);
    cap = 0;
    RCHK(dmalloc(h, (void**)&p, n * sizeof(T)));
    cap = n;
    return RRV_OK;
}

// Staging buffers of the host entries (rrv_ctx::hstage): one pair on the device, one page-locked on the host.
void stage_free(rrv_ctx::StageBufs& b, bool pinned) {
    for (void* p : {(void*)b.in, b.out})
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    b = rrv_ctx::StageBufs{};
}
// Set `set` grows (never shrinks) to at least in_bytes of frames and out_bytes of output (float32 or uint8 frames); 0 = that
// buffer is not used.  The caller makes sure nothing in flight uses the set.  The capacities are recorded only once both
// buffers exist: a failed allocation leaves the pair empty.
int stage_reserve(rrv_handle h, int set, size_t in_bytes, size_t out_bytes, bool pinned) {
    rrv_ctx::StageBufs& b = pinned ? h->hstage[set].pin : h->hstage[set].dev;
    if (b.in_cap >= in_bytes && b.out_cap >= out_bytes) return RRV_OK;
    in_bytes = std::max(in_bytes, b.in_cap);
    out_bytes = std::max(out_bytes, b.out_cap);
    stage_free(b, pinned);
    auto get = [&](void** p, size_t bytes) -> int {      // device memory through dmalloc (rrv_debug_fail_alloc counts it)
        if (!bytes) return RRV_OK;
        if (!pinned) return dmalloc(h, p, bytes);
        if (hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess) return RRV_OK;
        *p = nullptr;
        (void)hipGetLastError();
        return fail(h, RRV_E_NOMEM, "staging: out of page-locked host memory");
    };
    int rc = get((void**)&b.in, in_bytes);
    if (rc == RRV_OK) rc = get(&b.out, out_bytes);
    if (rc != RRV_OK) { stage_free(b, pinned); return rc; }
    b.in_cap = in_bytes; b.out_cap = out_bytes;
    return RRV_OK;
}

// ---- per-frame decoder --------------------------------------------------------------------
void dec_free(rrv_handle h, DecPlan& d) {
    plan_tfree(d, DEC_T);
    if (d.pre) { if (h->last_pre == d.pre) h->last_pre = nullptr; (void)hipFree(d.pre); d.pre = nullptr; }
    d.B = d.H = d.W = 0;
}

// KernelFilter.down_sample with the folded filter F1 + LeakyReLU (filter_down).  At the relu4_1 resolution a frame has few
// 16x16 pixel tiles (25 at 512x512, 81 at 1024x1024) and the layer a single cout slab, so one launch fills a fraction of
// the chip with one long item per workgroup.  The contraction over the 512 input channels is therefore split into
// slices (split K): each slice is its own item with a raw partial output, a small kernel sums them and applies the
// LeakyReLU.  The split depends on the FRAME's relu4_1 size (H8 x W8) only, so a frame's arithmetic is the same in any batch.
int kf_split(int H8, int W8) {
    const int tiles = ((W8 + 15) / 16) * ((H8 + 15) / 16);
    // measurement knob (profiles/r05_kernelfilter.txt): RRV_KSPLIT = 1 / 2 / 4 / 8 forces the split
    static const int forced = [] { const char* e = getenv("RRV_KSPLIT"); const int v = e ? atoi(e) : 0; return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 0; }();
    if (forced) return forced;
    return tiles * 8 <= 320 ? 8 : (tiles * 4 <= 512 ? 4 : (tiles * 2 <= 256 ? 2 : 1));
}

// frame: with the batched frame mode's scratch, mask: with the level masks (a plan built without them is rebuilt, and keeps what it had)
int dec_plan(rrv_handle h, const Seq& q, DecPlan& d, int B, int H, int W, bool frame = false, bool mask = false) {       // complete or empty, as enc_plan
    if (d.B >= B && d.H == H && d.W == W && d.pre && (!frame || d.spart.p) && (!mask || d.lm[0].p)) return RRV_OK;
    if (d.H == H && d.W == W) { frame = frame || d.spart.p; mask = mask || d.lm[0].p; }
    dec_free(h, d);
    const int split = kf_split(H / 8, W / 8);
    RCHK(plan_talloc(h, q, d, DEC_T, B, H, W, [&](const TSpec<DecPlan>& s) {
        if (s.flags & TS_FRAME) return frame ? s.C : 0;
        if (s.flags & TS_MASK) return mask ? s.C : 0;
        if (s.flags & TS_P8) return (h->p8 & 2) && p8_fits(H >> s.level, W >> s.level, s.C) ? s.C : 0;
        if (s.flags & TS_SPLIT) return split > 1 ? s.C * split : 0;
        return s.C;
    }));
    const int rc = dalloc(h, q, &d.pre, (size_t)B * H * W * 3, true);
    if (rc != RRV_OK) { dec_free(h, d); return rc; }
    d.B = B; d.H = H; d.W = W;
    return RRV_OK;
}

// KernelFilter.down_sample (cur -> d.d), split K by kf_split into the plan's d.dpart
int filter_down(rrv_handle h, const Seq& q, const Tens* cur, DecPlan& d, int f, int B) {
    const int split = kf_split(cur->H, cur->W);
    if (split == 1) {
        ConvCall c{cur, &d.d, &q.set->fold_down[f], cur->H, cur->W}; c.B = B; c.epi = E_LRELU;
        if (q.state_images) { c.w_bstride = 32 * 512 * 16; c.bias_bstride = 256; }
        return conv(h, q, c);
    }
    Tens& t = d.dpart;
    ConvCall c{cur, &t, &q.set->fold_down[f], cur->H, cur->W}; c.B = B; c.epi = 0; c.ksplit = split; c.bias = q.set->fold_down[f].bias;
    if (q.state_images) { c.w_bstride = 32 * 512 * 16; c.bias_bstride = 256; }
    RCHK(conv(h, q, c));
    const long npix = (long)B * (d.d.H + 2) * (d.d.W + 2);
    stamp(h, &d.d, B);
    return launch(h, q, "sum_parts", 0, 4.0 * 32 * (split + 1) * npix, [&] {
        const long nb = (npix * 8 + 255) / 256;
        hipLaunchKernelGGL(sum_parts_lrelu_k, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, q.stream, (const float*)t.p, d.d.p, split, npix);
    });
}

// KernelFilter.upsample (d.d -> out) + the residual `cur`, with the per-image folded weights of a state_images launch.  Filter3's
// epilogue also applies Decoder.norm[1] and its AdaIN affine (frame mode: an identity entry, then * style_std + style_mean).
int filter_up(rrv_handle h, const Seq& q, const Tens* cur, DecPlan& d, Tens* out, int f, int B) {
    const float* st = q.set->active;
    ConvCall u{&d.d, out, &q.set->fold_up[f], cur->H, cur->W}; u.B = B;
    if (q.state_images) { u.w_bstride = 512 * 32 * 16; u.par_bstride = RRV_STATE_FLOATS; }
    u.epi = E_RES | (f == 2 ? E_NORM2 : 0); u.res = cur;
    if (f == 2) { u.n2 = st + SL.norm[N_DEC1]; u.sty = st + SL.sty[3]; }
    return conv(h, q, u);
}

struct Win { int y0, x0, y1, x1; };     // output window in pixels, tile aligned; y1 == 0: everything

// The decoder's three residual blocks: output channels, the saved-statistics entries of norm1 / norm2 / the AdaIN norm behind
// the block, and the style entry of that AdaIN.  Block k works on the plans' xs[k], a[k], o[k].
struct BlkDesc { const char* name; int cout, n1, n2, nada, sty; };
const BlkDesc BLKS[3] = {{"slice4", 256, N_S4N1, N_S4N2, N_DEC2, 2}, {"slice3", 128, N_S3N1, N_S3N2, N_DEC3, 1}, {"slice2", 64, N_S2N1, N_S2N2, N_DEC4, 0}};

// conv2 of block k of the per-frame path, on the NHWC a[k] (resblock_frame rebinds it to the P8 twin); wo: its output window, if any
ConvCall block_conv2(rrv_handle h, const Seq& q, int B, int k, DecPlan& d, const Win* wo) {
    const BlkDesc& b = BLKS[k];
    const float* st = q.set->active;
    ConvCall c{&d.a[k], &d.o[k], &h->conv[std::string("Decoder.") + b.name + ".conv2"], d.a[k].H, d.a[k].W}; c.B = B;
    if (q.state_images) c.par_bstride = RRV_STATE_FLOATS;
    c.epi = E_LRELU | E_NORM1 | E_RES_UPS | E_NORM2; c.n1 = st + SL.norm[b.n2]; c.res = &d.xs[k]; c.n2 = st + SL.norm[b.nada]; c.sty = st + SL.sty[b.sty];
    if (wo) { c.wy0 = wo->y0; c.wx0 = wo->x0; c.wy1 = wo->y1; c.wx1 = wo->x1; }
    return c;
}

// block k of the per-frame path, fused across its normalisation layers (saved statistics)
// mid_wait: conv2 is launched behind this event (SeqHook::tail_wait)
int resblock_frame(rrv_handle h, const Seq& q, int B, int k, const Tens& in, DecPlan& d, const Win* wa = nullptr, const Win* wo = nullptr, hipEvent_t mid_wait = nullptr) {
    const BlkDesc& b = BLKS[k];
    Tens &xs = d.xs[k], &a = d.a[k], &qa = d.qa[k];
    ConvCall c2 = block_conv2(h, q, B, k, d, wo);
    // conv2 on conv_f43_k reads its input channel-chunk-major (conv_f43.h LAY; same bits, 12 % faster): conv1 then writes the twin,
    // where the plan has one (dec_plan)
    const bool p8 = qa.p && use_f43(h, q, c2);
    if (p8) { c2.in = &qa; c2.in_p8 = true; }
    // conv1 behind the upsample and, in the same kernel, the 1x1 shortcut at the input resolution: up(conv1x1(x)) == conv1x1(up(x))
    ConvCall c{&in, p8 ? &qa : &a, &h->conv[std::string("Decoder.") + b.name + ".conv1"], a.H, a.W}; c.B = B; c.ups = true; c.epi = E_LRELU | E_NORM1;
    c.n1 = q.set->active + SL.norm[b.n1]; c.sc_out = &xs; c.out_p8 = p8;
    if (q.state_images) c.par_bstride = RRV_STATE_FLOATS;
    if (wa) { c.wy0 = wa->y0; c.wx0 = wa->x0; c.wy1 = wa->y1; c.wx1 = wa->x1; }
    RCHK(conv(h, q, c));
    if (mid_wait) HIPCHK(hipStreamWaitEvent(q.stream, mid_wait, 0));
    return conv(h, q, c2);
}

// the conv_last_k instantiation that writes `f`
typedef void (*LastFn)(LastP);
LastFn last_kernel(OutFmt f) {
    if (yuv16_layout(f.yuv)) return conv_last_k<true, false, SP_PIXEL, true, true>;
    if (f.yuv) return conv_last_k<true, false, SP_PIXEL, true>;
    if (f.u8) return f.chw ? conv_last_k<true, true> : conv_last_k<true>;
    static const LastFn k[2][3] = {{conv_last_k<false>, conv_last_k<false, false, SP_UNIT>, conv_last_k<false, false, SP_NORM>},
                                   {conv_last_k<false, true>, conv_last_k<false, true, SP_UNIT>, conv_last_k<false, true, SP_NORM>}};
    return k[f.chw][f.space];
}

// Decoder.slice1 + transform_back_image (conv_last_k) on a normalised slice2 output
// fr: launch frames [fr->first, fr->first + fr->count) of the B only (every tensor is one contiguous block per frame, the output frames are
// the view's frame stride apart); the pre-clamp tap's bookkeeping stays that of the whole batch
// ov: where the rows of the delivered frames are (null: contiguous frames, whose view is built here)
struct FrameRange { int first, count; };
int run_last(rrv_handle h, const Seq& q, const Tens& o2, int B, int H, int W, void* d_out, OutFmt fmt, float* pre, const PadCrop* pc, const ImgView* ov, const Win* wl = nullptr,
             const FrameRange* fr = nullptr) {
    LastP lp{o2.p, H, W, B, h->last_w, h->last_b, d_out, pre, (W + 15) / 16, (H + 15) / 16,
             pc ? pc->src_H : 0, pc ? pc->src_W : 0, pc ? pc->top : 0, pc ? pc->left : 0, 0, 0};
    lp.v = ov ? *ov : contiguous_view(out_view_layout(fmt), pc ? pc->src_H : H, pc ? pc->src_W : W, fmt.cs);
    if (fr) {
        lp.in += (size_t)fr->first * (size_t)(H + 2) * (size_t)(W + 2) * 64;
        lp.out_img = (char*)d_out + (size_t)fr->first * (size_t)lp.v.fs * out_view_elem(fmt);
        if (pre) lp.out_pre = pre + (size_t)fr->first * H * W * 3;
        lp.B = fr->count;
    }
    const int LB = lp.B;
    if (fmt.yuv) {
        if (pc && ((pc->top | pc->left) & 1)) return fail(h, RRV_E_ARG, "conv_last: the YUV form needs an even crop origin");
        const YuvLaunch y = yuv_launch_params(h->yuv_out, false, yuv16_layout(fmt.yuv), fmt.yuv == RRV_LAY_P016);
        memcpy(lp.yuv_m, y.m, sizeof lp.yuv_m); lp.yuv_hi = y.hi; lp.yuv_shift = y.shift;
        lp.yuv_nv12 = fmt.yuv == RRV_LAY_NV12 || fmt.yuv == RRV_LAY_P016;
        lp.csx = chroma_sx(fmt.cs); lp.csy = chroma_sy(fmt.cs);
    }
    if (wl) { lp.ty0 = wl->y0 / 16; lp.tx0 = wl->x0 / 16; lp.tiles_y = (wl->y1 - wl->y0) / 16; lp.tiles_x = (wl->x1 - wl->x0) / 16; }
    h->last_pre = pre; h->last_pre_H = H; h->last_pre_W = W; h->last_pre_B = B;
    const unsigned tiles = (unsigned)(lp.tiles_x * lp.tiles_y * LB), resident = (unsigned)h->n_cus * 4;     // persistent: 4 workgroups of 35 KB per CU
    const unsigned grid = tiles < resident ? tiles : resident;
    return launch(h, q, "conv_last", 2.0 * LB * H * W * 576 * 3, (256.0 + (fmt.yuv ? yuv_samples_per_pixel(fmt.cs) * yuv_sample_bytes(fmt) : 3.0 * out_elem(fmt))) * LB * H * W, [&] {
        hipLaunchKernelGGL(last_kernel(fmt), dim3(grid), dim3(256), 0, q.stream, lp);
    }, -1.0, grid, -1);
}

// What host_pipeline asks of one launch sequence beyond its frames.
//   tail_wait  the sequence's last two launches (slice2.conv2 and conv_last, 1.9 of the 19.7 ms of 16 frames at 640 x 640) are queued behind
//              this event, the previous sub-batch's last kernel.  The two compute streams still run side by side all the time, but consecutive
//              sub-batches finish that tail apart instead of together, which is longer than a sub-batch's D2H (1.4 ms): every D2H but the
//              call's last runs under kernels.  Measured (profiles/r09_call_timeline.txt): a wait further up (in front of the first
//              filter_down, half a sequence) loses more than the copy it hides, since a stream then runs alone for half a sequence at both
//              ends of a call, 10.4 ms in place of 9.3; a wait in front of conv_last alone (0.4 ms) hides nothing.
//   piece      > 0: conv_last runs over ranges of `piece` frames, each followed by its own D2H on `copy` (piece i's ordered by ev[i]) of
//              frame_bytes per frame from d_out to h_dst: the call's last copy starts behind the first range, not behind the sub-batch
struct SeqHook {
    hipEvent_t tail_wait = nullptr;
    int piece = 0; char* h_dst = nullptr; size_t frame_bytes = 0; hipStream_t copy = nullptr; hipEvent_t* ev = nullptr;
};

// feats != nullptr: skip the encoder and start from one cached raw relu4_1 feature per image (ring layout, [1,H/8,W/8,512])
// q.state_images: 0 = every image uses the state set q.set, B = image b uses q.set + b (frames and cached features alike)
// q.slot: the slot whose workspace the launches use; the caller chooses it (next_device_slot, sub-batch parity, ticket, group)
// Writes no state set and leaves active_src alone.
int transfer_device(rrv_handle h, const Seq& q, const uint8_t* d_in, int B, int H, int W, void* d_out, const FrameIO& io, const float* const* feats = nullptr,
                    const SeqHook* hk = nullptr) {
    const PadCrop* const pc = io.pc;
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    // Any frame size, as the reference: the three 2x2 max pools floor (H, W) to (H/8, W/8) and the decoder returns
    // 8*(H/8) x 8*(W/8) pixels (test/style_network_global.py:271-281, :111-122) — the stylized frame is [Ho][Wo][3].
    const int Ho = H / 8 * 8, Wo = W / 8 * 8;
    RCHK(check_frame(h, H, W, "transfer"));
    if (h->active_src == -1) return fail(h, RRV_E_STATE, "state not computed: call compute() (or set_state) before transfer()");
    if (B < 1 || B > 64) return fail(h, RRV_E_ARG, "transfer: batch must be in 1..64");
    rrv_ctx::Slot& sl = h->slots[q.slot];
    sl.set_images = 0;       // (the grouped multi-style entry counts its images after this returns)
    if (io.caller.sync) {    // stream-ordered against the caller: work queued on its stream so far precedes ours
        HIPCHK(hipEventRecord(sl.ev, io.caller.stream));
        HIPCHK(hipStreamWaitEvent(q.stream, sl.ev, 0));
    }
    EncPlan& e = pick_plan(h, sl.enc, B, H, W);
    DecPlan& d = pick_plan(h, sl.dec, B, Ho, Wo);
    RCHK(enc_plan(h, q, e, B, H, W, true));
    RCHK(dec_plan(h, q, d, B, Ho, Wo));
    e.gen = d.gen = ++h->launch_gen;
    const float* st = q.set->active;
    // per-image state: every image's relu4_1 is normalised with ITS set's Decoder.norm[0] entry
    if (q.state_images ? q.state_images != B : (feats && B != 1)) return fail(h, RRV_E_ARG, "transfer: per-image state needs one state set per image");
    const long stride = q.state_images ? (long)RRV_STATE_FLOATS : 0;
    if (feats) {  // cached raw relu4_1 features: Decoder.norm[0] (saved stats + clamp) as a pointwise step per image
        for (int b = 0; b < B; ++b) {
            Tens src; src.p = const_cast<float*>(feats[b]); src.B = 1; src.H = H / 8; src.W = W / 8; src.C = 512;
            Tens dst = e.c41; dst.B = 1; dst.p = e.c41.p + (size_t)b * e.c41.img_floats();
            const float* n0 = st + (size_t)b * stride + SL.norm[N_DEC0];
            RCHK(pointwise(h, q, src, dst, n0, n0 + 512, false, nullptr, 0, nullptr, nullptr, n0 + 1024, n0 + 1536));
        }
        stamp(h, &e.c41, B);      // (pointwise stamped the one-image views: the debug taps see the tensor as written)
    } else {
        RCHK(run_encoder(h, q, e, d_in, io.in, 0, st + SL.norm[N_DEC0], pc, B, nullptr, (int)stride, io.iv));
    }
    const Tens* cur = &e.c41;
    for (int f = 0; f < 3; ++f) {
        RCHK(filter_down(h, q, cur, d, f, B));
        RCHK(filter_up(h, q, cur, d, &d.f[f], f, B));
        cur = &d.f[f];
    }
    // On-device crop: nothing outside the crop window is delivered, so the full-resolution layers only compute the
    // tiles the window (plus one halo pixel per 3x3 layer) needs; results inside the window are unchanged.  One level
    // down (320^2) the tile-rounded window already covers the frame for the reference's 64-pixel pad.
    Win wl{0, 0, 0, 0}, wo{0, 0, 0, 0}, wa{0, 0, 0, 0};
    const bool roi = pc != nullptr;
    if (roi) {
        auto grow = [&](const Win& w, int halo) {
            auto lo = [&](int v) { v -= halo; return v < 0 ? 0 : (v & ~15); };
            auto hi = [&](int v, int lim) { v = (v + halo + 15) & ~15; const int l = (lim + 15) & ~15; return v > l ? l : v; };
            return Win{lo(w.y0), lo(w.x0), hi(w.y1, Ho), hi(w.x1, Wo)};
        };
        const Win crop{pc->top, pc->left, pc->top + pc->src_H, pc->left + pc->src_W};
        wl = grow(crop, 0);        // conv_last output tiles
        wo = grow(crop, 1);        // slice2.conv2 output feeding them
        if (use_f43(h, q, block_conv2(h, q, B, 2, d, nullptr))) {      // 32 x 32 pixel work items: round the window out to them (asked before the window exists: the call carries none)
            const int lh = (Ho + 31) & ~31, lw = (Wo + 31) & ~31;
            wo = Win{wo.y0 & ~31, wo.x0 & ~31, (wo.y1 + 31) & ~31, (wo.x1 + 31) & ~31};
            if (wo.y1 > lh) wo.y1 = lh;
            if (wo.x1 > lw) wo.x1 = lw;
        }
        wa = grow(wo, 1);          // slice2.conv1 output (and, halved, the shortcut) feeding that
    }
    for (int k = 0; k < 3; ++k) {       // the windows apply to the full-resolution block only
        const bool win = roi && k == 2;
        RCHK(resblock_frame(h, q, B, k, k ? d.o[k - 1] : d.f[2], d, win ? &wa : nullptr, win ? &wo : nullptr, hk && k == 2 ? hk->tail_wait : nullptr));
    }
    if (hk && hk->piece > 0 && hk->piece < B) {
        int i = 0;
        for (int b0 = 0; b0 < B; b0 += hk->piece, ++i) {
            const FrameRange fr{b0, B - b0 < hk->piece ? B - b0 : hk->piece};
            RCHK(run_last(h, q, d.o[2], B, Ho, Wo, d_out, io.out, d.pre, pc, io.ov, roi ? &wl : nullptr, &fr));
            const size_t off = (size_t)b0 * hk->frame_bytes;
            HIPCHK(hipEventRecord(hk->ev[i], q.stream));
            HIPCHK(hipStreamWaitEvent(hk->copy, hk->ev[i], 0));
            HIPCHK(hipMemcpyAsync(hk->h_dst + off, (const char*)d_out + off, (size_t)fr.count * hk->frame_bytes, hipMemcpyDeviceToHost, hk->copy));
        }
    } else {
        RCHK(run_last(h, q, d.o[2], B, Ho, Wo, d_out, io.out, d.pre, pc, io.ov, roi ? &wl : nullptr));
    }
    if (io.caller.sync) {    // ... and whatever the caller queues next sees our output
        HIPCHK(hipEventRecord(sl.ev, q.stream));
        HIPCHK(hipStreamWaitEvent(io.caller.stream, sl.ev, 0));
    }
    if (h->debug) RCHK(debug_verify(h, "transfer"));
    return RRV_OK;
}

// ---- the unfused residual blocks -----------------------------------------------------------------------------------------
// Decoder.slice4 / slice3 / slice2 where the statistics of the normalisation layers are not known yet, so the chain stops at
// each of the nine sync points 3 k + {0: norm1, 1: norm2, 2: the AdaIN norm} of block k (BLKS):
//   conv1 behind the upsample -> [stat] -> normalise -> conv2 -> [stat] -> normalise + shortcut -> [stat] -> normalise + AdaIN.
// stat(t, n, point) puts the statistics of t into norm[n] of `st` (of every image's set, par_bstride apart) — or finds them
// there — and returns RRV_OK, or WALK_STOP to end the walk at that point with nothing further launched.  B images from `in`
// through xs[k], a[k], o[k].  fused_sc: conv1's kernel also writes the 1x1 shortcut; otherwise conv_shortcut is its own launch,
// issued once norm2's statistic is taken (the first place that needs it).  last_adain: whether o[2] is normalised at the end.
enum { WALK_STOP = 1 };     // (RRV_E_* are negative)
// norm(x, y, n, res, sty) is the normalisation step: y = x normalised with entry n [+ res, upsampled 2x] [AdaIN with style entry sty].
template <class Stat, class Norm>
int unfused_blocks(rrv_handle h, const Seq& q, int B, const Tens& x, Tens (&xs)[3], Tens (&a)[3], Tens (&o)[3], bool fused_sc, bool last_adain, Stat&& stat, Norm&& norm) {
    const Tens* in = &x;
    for (int k = 0; k < 3; ++k) {
        const BlkDesc& b = BLKS[k];
        const std::string p = std::string("Decoder.") + b.name;
        const int H2 = in->H * 2, W2 = in->W * 2;
        ConvCall c;
        c = ConvCall{in, &a[k], &h->conv[p + ".conv1"], H2, W2}; c.B = B; c.ups = true; c.epi = E_LRELU;
        if (fused_sc) c.sc_out = &xs[k];
        RCHK(conv(h, q, c));
        RCHK(stat(a[k], b.n1, 3 * k));
        RCHK(norm(a[k], a[k], b.n1, (const Tens*)nullptr, -1));
        c = ConvCall{&a[k], &o[k], &h->conv[p + ".conv2"], H2, W2}; c.B = B; c.epi = E_LRELU; RCHK(conv(h, q, c));
        RCHK(stat(o[k], b.n2, 3 * k + 1));
        if (!fused_sc) { c = ConvCall{in, &xs[k], &h->conv[p + ".conv_shortcut"], in->H, in->W}; c.B = B; RCHK(conv(h, q, c)); }
        RCHK(norm(o[k], o[k], b.n2, (const Tens*)&xs[k], -1));
        RCHK(stat(o[k], b.nada, 3 * k + 2));     // (a fused pointwise + statistics pass measured slower than the two kernels)
        if (k < 2 || last_adain) RCHK(norm(o[k], o[k], b.nada, (const Tens*)nullptr, b.sty));
        in = &o[k];
    }
    return RRV_OK;
}
// the walk with the saved statistics of state `st` applied by pointwise_k (apply_norm): the preparation pass and the frame mode
template <class Stat>
int unfused_blocks(rrv_handle h, const Seq& q, int B, const Tens& x, Tens (&xs)[3], Tens (&a)[3], Tens (&o)[3], const float* st, long par_bstride, bool fused_sc,
                   bool last_adain, Stat&& stat) {
    return unfused_blocks(h, q, B, x, xs, a, o, fused_sc, last_adain, stat,
                          [&](const Tens& t, Tens& y, int n, const Tens* res, int sty) { return apply_norm(h, q, t, y, st, n, res, sty, par_bstride); });
}

// ---- preparation: Decoder.compute for one style ---------------------------------------------
void prep_free(rrv_handle h) { plan_tfree(h->prep, PREP_T); }
int prep_chans(const TSpec<PrepPlan>& s, bool streaming) { return s.flags & (streaming ? TS_RES : TS_STREAM) ? 0 : s.C; }
// rrv_compute's workspace for B frames (streaming: a group of B) of relu4_1 features hh x ww; complete or empty
int prep_plan(rrv_handle h, const Seq& q, int B, int hh, int ww, bool streaming) {
    return plan_talloc(h, q, h->prep, PREP_T, B, hh << 3, ww << 3, [&](const TSpec<PrepPlan>& s) { return prep_chans(s, streaming); });
}
// what prep_plan allocates
size_t prep_bytes(int B, int hh, int ww, bool streaming) {
    size_t n = 0;
    for (const TSpec<PrepPlan>& s : PREP_T) {
        int b = B, H = hh << 3, W = ww << 3, c = prep_chans(s, streaming);
        if (!c) continue;
        s.geo(b, H, W, c);
        n += tens_floats(b, H, W, c) * sizeof(float);
    }
    return n;
}

// the 14 sync points of the pass, in order (the streaming pass walks them one by one; rrv_debug_prep_stop ends either pass at one)
enum { ST_NORM0 = 0, ST_FILTER = 1 /* +f */, ST_NORM1 = 4, ST_BLOCKS = 5 /* +3k: n1, n2, nada */, ST_COUNT = 14 };

// on the plan's content batch (rrv_compute)
int compute_style(rrv_handle h, const Seq& q, int sid) {
    StyleState& S = h->styles[sid];
    float* st = S.blob;
    PrepPlan& P = h->prep;
    const Tens& content = P.content;
    const int B = content.B, hh = content.H, ww = content.W;
    Tens &cn = P.cn, &nxt = P.nxt, &t32 = P.t32, &d32 = P.d32, &u = P.u;
    float* cmean = h->prep_cmean;
    const int stop = h->prep_stop;
    if (stop >= 0) S.computed = false;
    auto body = [&]() -> int {
        // norm[0].compute on the batch (style_network_global.py:396); the style half of the filter predictions
        // (normalized_style :397 through F.down_sample, :161-172) was evaluated once in prepare_style (S.smean)
        RCHK(chan_stats(h, q, content, 1, st + SL.norm[N_DEC0]));
        if (stop == ST_NORM0) return WALK_STOP;
        RCHK(apply_norm(h, q, content, cn, st, N_DEC0));
        Tens* cur = &cn; Tens* other = &nxt;
        for (int f = 0; f < 3; ++f) {
            char pre[64];
            snprintf(pre, sizeof pre, "Decoder.Filter%d", f + 1);
            for (int g = 0; g < 2; ++g) {   // FilterPredictor.compute (:161-172) for F1 then F2
                const ConvW* wp = &h->conv[std::string(pre) + (g ? ".F2" : ".F1") + ".down_sample.0"];
                ConvCall c{cur, &t32, wp, hh, ww}; c.B = B; RCHK(conv(h, q, c));
                RCHK(chan_stats(h, q, t32, 0, cmean));
                hipLaunchKernelGGL(fc_filter_k, dim3(4), dim3(256), 0, q.stream, (const float*)h->fc_w[2 * f + g],
                                   (const float*)h->fc_b[2 * f + g], (const float*)cmean, (const float*)(S.smean + (2 * f + g) * 32), st + SL.filt[2 * f + g]);
                HIPCHK(hipGetLastError());
            }
            RCHK(fold_filters(h, q, st, f));
            // KernelFilter.compute (:223-230): only frame 0 passes through apply_filter (Q1)
            Tens cur0 = *cur; cur0.B = 1;
            ConvCall c{&cur0, &d32, &q.set->fold_down[f], hh, ww}; c.epi = E_LRELU; RCHK(conv(h, q, c));
            ConvCall cu{&d32, &u, &q.set->fold_up[f], hh, ww}; RCHK(conv(h, q, cu));
            RCHK(pointwise(h, q, *cur, *other, nullptr, nullptr, false, &u, 1, nullptr, nullptr));
            if (stop == ST_FILTER + f) return WALK_STOP;
            Tens* t = cur; cur = other; other = t;
        }
        h->active_src = -1;   // folded weights now belong to this style's blob; re-activate below
        // AdaIN_compute(1) (style_network_global.py:428)
        RCHK(chan_stats(h, q, *cur, 1, st + SL.norm[N_DEC1]));
        if (stop == ST_NORM1) return WALK_STOP;
        RCHK(apply_norm(h, q, *cur, *cur, st, N_DEC1, nullptr, 3));
        // AdaIN_compute(k + 2) ends block k; nothing reads the last block's normalised output
        return unfused_blocks(h, q, B, *cur, P.xs, P.a, P.o, st, 0, false, false, [&](const Tens& t, int n, int point) -> int {
            RCHK(chan_stats(h, q, t, 1, st + SL.norm[n]));
            return stop == ST_BLOCKS + point && stop != ST_COUNT - 1 ? WALK_STOP : RRV_OK;
        });
    };
    int rc = body();
    const bool stopped = rc == WALK_STOP;      // rrv_debug_prep_stop: the state is left as far as it got, not computed
    if (stopped) { rc = RRV_OK; h->active_src = -1; }
    if (rc == RRV_OK && h->debug) rc = debug_verify(h, "Decoder.compute");
    (void)hipStreamSynchronize(q.stream);
    if (rc == RRV_OK && !stopped) S.computed = true;
    if (rc == RRV_OK && !stopped) rc = filter_conditioning(h, S);
    return rc;
}

// ---- frame mode (Stylization(use_Global=False), test/style_network_frame.py) ----------------------------------------
// Per-frame InstanceNorm statistics (:39-43: mean / biased variance over (H,W), no clamp) and per-frame filter prediction
// (:53-62, :97-105).  Every frame is a batch of its own, so Q1's batch collapse does not arise and the fused per-frame kernels run
// wherever no statistic separates producer and consumer: encoder -> [stats] -> normalise -> per filter {rectangle sums ->
// predicted means -> FC -> fold -> 512->32 (LReLU) -> 32->512 + residual} (the last one also applies the AdaIN affine,
// :326-339 ends with * style_std + style_mean and no norm) -> per block {conv1 behind the upsample with the fused
// shortcut (raw) -> [stats] -> normalise -> conv2 (raw) -> [stats] -> normalise + shortcut -> [stats] -> normalise +
// AdaIN} -> slice1.  [stats] = ONE read of the tensor (chan_stat1_k) + a merge; the filter predictors' conv + mean is
// replaced by nine rectangle sums and a 64 x 4608 product (prep_kernels.h), their style half is cached per style.

// ---- batched frame mode: B <= MS_GROUP_MAX frames per launch sequence ----------------------------------------------------
// The chain above for B frames at once (the one-frame entry is B = 1).  Every frame's statistics, predicted filters and folded KernelFilter weights go
// to its own state set (q.set + b: the sets MS_GROUP_MAX * slot .., initialised from style 0's blob), and every per-frame kernel
// runs over the B images with image b's result in set b or in row b of the plan's scratch (DecPlan::spart ..).  The statistics
// kernels partition every image on its own (chan_stats1_images) and the convolutions are F(2x2,3x3) (Seq::f43 is false), so
// an image's bits do not depend on the batch it rides in.  Style 0's blob is only read.

// interior row b of a TS_FRAME scratch tensor (ring layout, B = 1, H = images): contiguous, frame_row_stride floats apart
float* frame_row(const Tens& t) { return t.p + (size_t)(t.W + 3) * t.C; }
long frame_row_stride(const Tens& t) { return (long)(t.W + 2) * t.C; }

// per-image statistics of the t.B images of t into norm entry `n` of each image's state set: ONE read of the tensor + a merge
int chan_stats1_images(rrv_handle h, const Seq& q, const Tens& t, const DecPlan& d, int n) {
    const int nblk = t.H < 512 ? t.H : 512;        // per image min(H, 512) blocks of whole rows (~2 blocks per CU keep the merge short), whatever the batch
    if ((size_t)nblk * 6 * t.C > (size_t)d.spart.W * d.spart.C || t.B > d.spart.H) return fail(h, RRV_E_ARG, "chan_stats1_images: scratch too small");
    double* part = (double*)frame_row(d.spart);
    const long pbs = frame_row_stride(d.spart) / 2;
    float* out = q.set->active + SL.norm[n];
    StatP sp{t.p, t.B, t.H, t.W, t.C, nullptr, part, 0, 0, 1, pbs};
    stamp(h, &d.spart, t.B);
    RCHK(launch(h, q, "chan_stat1", 0, 4.0 * t.B * t.H * t.W * t.C, [&] { hipLaunchKernelGGL(chan_stat1_k, dim3(nblk, t.B), dim3(256), 0, q.stream, sp); }));
    return launch(h, q, "chan_stat1_final", 0, 0, [&] {
        hipLaunchKernelGGL(chan_stat1_final_k, dim3((t.C + 3) / 4, t.B), dim3(256), 0, q.stream, (const double*)part, nblk, t.C, out, pbs, (long)RRV_STATE_FLOATS);
    });
}

// B frames ([B][H][W][3] uint8; with pc: [B][src_H][src_W][3], padded on the way in, cropped on the way out) on q.slot, with the slot's own sets (q.set)
int frame_mode_device(rrv_handle h, const Seq& q, const uint8_t* d_in, int B, int H, int W, void* d_out, const FrameIO& io) {
    const PadCrop* const pc = io.pc;
    if (B < 1 || B > rrv_ctx::MS_GROUP_MAX || q.slot < 0 || q.slot > 1) return fail(h, RRV_E_ARG, "frame mode: batch must be in 1..16 on slot 0 or 1");
    StyleState& S = h->styles[0];
    const int Ho = H / 8 * 8, Wo = W / 8 * 8;
    rrv_ctx::Slot& sl = h->slots[q.slot];
    h->active_src = -1;                                   // the slot's sets (q.set ..; slot 0: set 0) are overwritten: a later global entry re-activates its state
    EncPlan& e = pick_plan(h, sl.enc, B, H, W);
    DecPlan& d = pick_plan(h, sl.dec, B, Ho, Wo);
    RCHK(enc_plan(h, q, e, B, H, W, true));
    RCHK(dec_plan(h, q, d, B, Ho, Wo, true));
    e.gen = d.gen = ++h->launch_gen;
    float* st = q.set->active;                          // image b: st + b * RRV_STATE_FLOATS
    const long PS = RRV_STATE_FLOATS;
    RCHK(launch(h, q, "frame_sets_init", 0, 8.0 * B * RRV_STATE_FLOATS, [&] {
        hipLaunchKernelGGL(frame_sets_init_k, dim3((RRV_STATE_FLOATS + 255) / 256, B), dim3(256), 0, q.stream, (const float*)S.blob, st, (int)RRV_STATE_FLOATS,
                           SL.norm[N_DEC1], 512);
    }));
    RCHK(run_encoder(h, q, e, d_in, io.in, 0, nullptr, pc, B, nullptr, 0, io.iv));
    Tens c41 = e.c41; c41.B = B;                         // views of B images (plans are grow-only)
    const int hh = c41.H, ww = c41.W;
    // Decoder.norm[0] with each frame's statistics
    RCHK(chan_stats1_images(h, q, c41, d, N_DEC0));
    RCHK(apply_norm(h, q, c41, c41, st, N_DEC0, nullptr, -1, PS));
    Tens fo[3], xs[3], a[3], o[3];
    for (int k = 0; k < 3; ++k) {
        fo[k] = d.f[k]; xs[k] = d.xs[k]; a[k] = d.a[k]; o[k] = d.o[k];
        fo[k].B = xs[k].B = a[k].B = o[k].B = B;
    }
    // per image: rect_sums_k's sums and pred_mean_k's means in rows of the scratch, the FC into its state set; one fold launch per
    // step for all sets (fold_filters nsets), the KernelFilter convs with per-image weights (state_images; one image: the shared ones)
    float* const Sr = frame_row(d.srect);
    float* const cm = frame_row(d.scm);
    const long Sbs = frame_row_stride(d.srect), cbs = frame_row_stride(d.scm);
    stamp(h, &d.srect, B); stamp(h, &d.scm, B);
    Seq qf = q;      // the KernelFilter convs alone read per-image state
    qf.state_images = B > 1 ? B : 0;
    const Tens* cur = &c41;
    for (int f = 0; f < 3; ++f) {
        // (one part: splitting an image's pixels over several blocks per channel quad measured slower, the merge in pred_mean_k costs more)
        RCHK(launch(h, q, "rect_sums", 0, 4.0 * B * hh * ww * 512, [&] {
            hipLaunchKernelGGL(rect_sums_k, dim3(128, 1, B), dim3(256), 0, q.stream, (const float*)cur->p, hh, ww, 512, Sr, Sbs);
        }));
        for (int g = 0; g < 2; ++g) {
            char key[96];
            snprintf(key, sizeof key, "Decoder.Filter%d.F%d.down_sample.0", f + 1, g + 1);
            const ConvW& wp = h->conv[key];
            RCHK(launch(h, q, "pred_mean", 2.0 * B * 32 * 4608, 0, [&] {
                hipLaunchKernelGGL(pred_mean_k, dim3(32, B), dim3(256), 0, q.stream, (const float*)wp.raw, (const float*)wp.bias, (const float*)Sr, 1, 512,
                                   1.0 / ((double)hh * ww), cm + 32 * g, Sbs, cbs);
            }));
            RCHK(launch(h, q, "fc_filter", 2.0 * B * 1024 * 64, 0, [&] {
                hipLaunchKernelGGL(fc_filter_k, dim3(4, B), dim3(256), 0, q.stream, (const float*)h->fc_w[2 * f + g], (const float*)h->fc_b[2 * f + g],
                                   (const float*)(cm + 32 * g), (const float*)(S.smean + (2 * f + g) * 32), st + SL.filt[2 * f + g], (int)cbs, (int)RRV_STATE_FLOATS);
            }));
        }
        RCHK(fold_filters(h, q, st, f, B));
        RCHK(filter_down(h, qf, cur, d, f, B));
        RCHK(filter_up(h, qf, cur, d, &fo[f], f, B));
        cur = &fo[f];
    }
    // full tensors: each frame's statistics cover its whole (padded) frame, as in the reference
    RCHK(unfused_blocks(h, q, B, *cur, xs, a, o, st, PS, true, true, [&](const Tens& t, int n, int) { return chan_stats1_images(h, q, t, d, n); }));
    RCHK(run_last(h, q, o[2], B, Ho, Wo, d_out, io.out, d.pre, pc, io.ov));
    // the launches above wrote views; the debug taps (rrv_debug_copy_tensor_ex) read the plan's own tensors
    stamp(h, &e.c41, B);
    for (int k = 0; k < 3; ++k)
        for (Tens* t : {&d.f[k], &d.xs[k], &d.a[k], &d.o[k]}) stamp(h, t, B);
    sl.set_images = B;
    if (h->debug) RCHK(debug_verify(h, "transfer (batched frame mode)"));
    return RRV_OK;
}

// ---- masked multi-style transfer: the saved state blended per pixel ---------------------------------------------------------
// "Multi-style Interpolation/stylization.py":94-100 blends every saved quantity q as sum_s w_s q_s once per frame
// (style_network.py:35-53,135-139,348-360) and runs the forward pass :432-460.  Here w is a mask at the frame's resolution: at a
// tensor pixel p of a decoder level q(p) = sum_s m_s(p) q_s, m the mean of the mask over the input pixels p covers (mask_kernels.h).
// The state cannot be folded into weights or fused epilogues, so the decoder runs the unfused walk of the frame mode with the
// saved statistics of the S styles in place of per-frame ones: encoder (raw relu4_1) -> mask pyramid -> masked norm[0] -> per
// filter {down_sample raw (split K as filter_down) -> mask_filter_k (F1(p), LeakyReLU, F2(p)) -> upsample + residual} -> masked
// norm[1] + AdaIN -> per block {conv1 + shortcut -> masked norm1 -> conv2 -> masked norm2 + shortcut -> masked AdaIN} -> slice1.
// F(2x2,3x3) throughout (Seq::f43 is false) and a split that follows the frame size: an image's bits do not depend on its batch.
// The styles' blobs are only read and no state set is written: the entries around a masked call keep their bits.

LevelMask level_mask(const Tens& t, int S, bool one) {
    return LevelMask{t.p + (size_t)(t.W + 3) * t.C, one ? 0 : (long)t.img_floats(), (t.W + 2) * t.C, S};
}

int mask_norm(rrv_handle h, const Seq& q, const Tens& x, Tens& y, const MaskStates& ms, int S, int n, const Tens* res, int sty, const LevelMask& m) {
    if (x.C % 64) return fail(h, RRV_E_ARG, "mask_norm: channels must be a multiple of 64");
    MaskNormP p{x.p, y.p, x.B, x.H, x.W, x.C, ms, S, SL.norm[n], sty < 0 ? -1 : SL.sty[sty], res ? res->p : nullptr, res ? res->H : 0, res ? res->W : 0, m, 1};
    // one block per image row and group of 64 channels; small tensors split their rows so that a few hundred blocks exist
    const long rows = (long)x.B * x.H * (x.C / 64);
    int segs = rows >= 1024 ? 1 : (int)((1024 + rows - 1) / rows);
    const int max_segs = (x.W + 15) / 16;
    p.segs = segs > max_segs ? max_segs : segs;
    stamp(h, &y, x.B);
    return launch(h, q, "mask_norm", 0, 8.0 * x.B * x.H * x.W * x.C, [&] { hipLaunchKernelGGL(mask_norm_k, dim3((unsigned)(rows * p.segs)), dim3(256), 0, q.stream, p); });
}

typedef void (*PyrFn)(const MaskPyrP&, dim3, hipStream_t);
template <int S> void pyr_launch(const MaskPyrP& p, dim3 grid, hipStream_t s) { hipLaunchKernelGGL(mask_pyramid_k<S>, grid, dim3(256), 0, s, p); }

// B <= MS_GROUP_MAX frames on q.slot (geometry as frame_mode_device); d_mask: [Bm][S][mH][mW] float32 in HBM, Bm = B or 1, at the
// resolution of the frames as the caller passed them (pc: the unpadded frame)
int mask_mode_device(rrv_handle h, const Seq& q, const uint8_t* d_in, int B, int H, int W, const float* d_mask, int S, bool one_mask, void* d_out,
                     const FrameIO& io) {
    const PadCrop* const pc = io.pc;
    if (B < 1 || B > rrv_ctx::MS_GROUP_MAX || q.slot < 0 || q.slot > 1) return fail(h, RRV_E_ARG, "masked transfer: batch must be in 1..16 on slot 0 or 1");
    const int Ho = H / 8 * 8, Wo = W / 8 * 8;
    rrv_ctx::Slot& sl = h->slots[q.slot];
    sl.set_images = 0;                                    // this launch keeps no per-image state set
    EncPlan& e = pick_plan(h, sl.enc, B, H, W);
    DecPlan& d = pick_plan(h, sl.dec, B, Ho, Wo);
    RCHK(enc_plan(h, q, e, B, H, W, true));
    RCHK(dec_plan(h, q, d, B, Ho, Wo, false, true));
    e.gen = d.gen = ++h->launch_gen;
    MaskStates ms{};
    for (int s = 0; s < S; ++s) ms.blob[s] = h->styles[s].blob;
    {   // the four level masks
        MaskPyrP pp{d_mask, pc ? pc->src_H : H, pc ? pc->src_W : W, pc ? 1 : 0, pc ? pc->top : 0, pc ? pc->left : 0, Ho / 8, Wo / 8, {}, {}, {}};
        for (int l = 0; l < 4; ++l) {
            const LevelMask m = level_mask(d.lm[l], S, false);
            pp.lv[l] = const_cast<float*>(m.p); pp.bstride[l] = m.bstride; pp.pitch[l] = m.pitch;
            stamp(h, &d.lm[l], one_mask ? 1 : B);
        }
        static const PyrFn pyr[8] = {pyr_launch<1>, pyr_launch<2>, pyr_launch<3>, pyr_launch<4>, pyr_launch<5>, pyr_launch<6>, pyr_launch<7>, pyr_launch<8>};
        const int nm = one_mask ? 1 : B;
        RCHK(launch(h, q, "mask_pyramid", 0, 8.0 * nm * S * Ho * Wo, [&] {
            pyr[S - 1](pp, dim3((unsigned)(((Ho / 8) * (Wo / 8) + 255) / 256), (unsigned)nm), q.stream);
        }));
    }
    LevelMask lm[4];
    for (int l = 0; l < 4; ++l) lm[l] = level_mask(d.lm[l], S, one_mask);
    RCHK(run_encoder(h, q, e, d_in, io.in, 0, nullptr, pc, B, nullptr, 0, io.iv));
    Tens c41 = e.c41; c41.B = B;                         // views of B images (plans are grow-only)
    Tens fo[3], xs[3], a[3], o[3], dd = d.d, dpart = d.dpart;
    dd.B = dpart.B = B;
    for (int k = 0; k < 3; ++k) {
        fo[k] = d.f[k]; xs[k] = d.xs[k]; a[k] = d.a[k]; o[k] = d.o[k];
        fo[k].B = xs[k].B = a[k].B = o[k].B = B;
    }
    // Decoder.norm[0], clamped, with the statistics blended at every relu4_1 pixel
    RCHK(mask_norm(h, q, c41, c41, ms, S, N_DEC0, nullptr, -1, lm[3]));
    const int split = kf_split(c41.H, c41.W);
    const Tens* cur = &c41;
    for (int f = 0; f < 3; ++f) {
        char pre[64];
        snprintf(pre, sizeof pre, "Decoder.Filter%d", f + 1);
        const ConvW& wd = h->conv[std::string(pre) + ".down_sample.0"];
        const ConvW& wu = h->conv[std::string(pre) + ".upsample.0"];
        // down_sample, raw: its bias is added by mask_filter_k (split K: the slabs' partial sums are summed there, in order)
        Tens& raw = split > 1 ? dpart : dd;
        ConvCall c{cur, &raw, &wd, cur->H, cur->W}; c.B = B; c.epi = 0; c.bias = h->zero_bias;
        if (split > 1) c.ksplit = split;
        RCHK(conv(h, q, c));
        MaskFilterP fp{raw.p, split, dd.p, wd.bias, ms, S, SL.filt[2 * f], SL.filt[2 * f + 1], lm[3], B, dd.H, dd.W};
        const long npix = (long)B * dd.H * dd.W;
        stamp(h, &dd, B);
        RCHK(launch(h, q, "mask_filter", 2.0 * npix * 2048 * (S + 1), 4.0 * npix * 32 * (split + 1), [&] {
            hipLaunchKernelGGL(mask_filter_k, dim3((unsigned)((npix + 63) / 64)), dim3(256), mask_filter_smem(S), q.stream, fp);
        }));
        ConvCall u{&dd, &fo[f], &wu, cur->H, cur->W}; u.B = B; u.epi = E_RES; u.res = cur;
        RCHK(conv(h, q, u));
        cur = &fo[f];
    }
    // Decoder.norm[1] + the relu4_1 AdaIN affine
    RCHK(mask_norm(h, q, *cur, fo[2], ms, S, N_DEC1, nullptr, 3, lm[3]));
    RCHK(unfused_blocks(h, q, B, *cur, xs, a, o, true, true, [](const Tens&, int, int) { return (int)RRV_OK; },
                        [&](const Tens& t, Tens& y, int n, const Tens* res, int sty) {
                            const int l = t.H == d.lm[0].H ? 0 : t.H == d.lm[1].H ? 1 : 2;
                            return mask_norm(h, q, t, y, ms, S, n, res, sty, lm[l]);
                        }));
    RCHK(run_last(h, q, o[2], B, Ho, Wo, d_out, io.out, d.pre, pc, io.ov));
    stamp(h, &e.c41, B); stamp(h, &d.d, B);
    if (split > 1) stamp(h, &d.dpart, B);
    for (int k = 0; k < 3; ++k)
        for (Tens* t : {&d.f[k], &d.xs[k], &d.a[k], &d.o[k]}) stamp(h, t, B);
    if (h->debug) RCHK(debug_verify(h, "transfer (masked multi-style)"));
    return RRV_OK;
}

// ---- streaming preparation pass ------------------------------------------------------------------------------
// Decoder.compute keeps every sampled frame's activations resident: O(B * 64 * H * W) at the last level (the reference
// authors' own long-sequence sketch streams them through a disk cache layer by layer: test/style_network.py:597-624).
// Here the pass is re-ordered by SYNC POINT instead: the 11 normalisation layers and the 3 filter predictions are the
// only places where frames interact (a mean / centred square sum / min / max over (B,H,W)), and quirk Q1 — only
// frame 0's KernelFilter residual exists and is broadcast to every frame — means nothing else crosses frames.  For
// each of the 14 sync points every GROUP of G frames re-runs the decoder prefix from its relu4_1 features with the
// statistics already known, contributes its partial (chan_merge_k) and is dropped.  Workspace = one group, whatever B.

// one group's partial statistics of tensor t merged into accumulator `slot` (n_a elements per channel seen before)
int chan_stats_group(rrv_handle h, const Seq& q, const Tens& t, bool want_m2, int slot, double n_a) {
    const long npix = (long)t.B * t.H * t.W;
    int nblk = (int)((npix + 255) / 256);
    if (nblk > 1024) nblk = 1024;
    if (nblk < 1) nblk = 1;
    const int ppb = (int)((npix + nblk - 1) / nblk);
    if (t.C > 512) return fail(h, RRV_E_ARG, "chan_stats: more than 512 channels");
    double* acc = h->stat_acc + (size_t)slot * 4 * 512;
    StatP sp{t.p, t.B, t.H, t.W, t.C, nullptr, h->stat_part, 0, ppb};
    const int fb = (t.C + 15) / 16;
    hipLaunchKernelGGL(chan_stat_k, dim3(nblk), dim3(256), 0, q.stream, sp);
    if (want_m2) {
        hipLaunchKernelGGL(chan_final_k, dim3(fb), dim3(256), 0, q.stream, (const double*)h->stat_part, nblk, t.C, (double)npix, 0, (const float*)nullptr, h->stat_mean);
        sp.pass = 1; sp.mean = h->stat_mean; sp.part = h->stat_part2;
        hipLaunchKernelGGL(chan_stat_k, dim3(nblk), dim3(256), 0, q.stream, sp);
    }
    hipLaunchKernelGGL(chan_merge_k, dim3(fb), dim3(256), 0, q.stream, (const double*)h->stat_part, want_m2 ? (const double*)h->stat_part2 : (const double*)nullptr,
                       nblk, t.C, (double)npix, (const float*)h->stat_mean, acc, n_a);
    HIPCHK(hipGetLastError());
    return RRV_OK;
}
int chan_stats_finish(rrv_handle h, const Seq& q, int slot, int C, double N, int mode, float* out) {
    hipLaunchKernelGGL(chan_finish_k, dim3((C + 255) / 256), dim3(256), 0, q.stream, (const double*)(h->stat_acc + (size_t)slot * 4 * 512), C, N, mode, out);
    HIPCHK(hipGetLastError());
    return RRV_OK;
}

// Decoder.compute prefix of one group (`grp`: nb raw relu4_1 features) up to sync point `stage`, whose partial
// statistics are merged (n_a = elements per channel already merged at that stage's resolution: frames_before * H * W).
int stream_prefix(rrv_handle h, const Seq& q, int sid, const Tens& grp, int nb, int stage, int frames_before) {
    StyleState& S = h->styles[sid];
    float* st = S.blob;
    PrepPlan& P = h->prep;
    const int hh = grp.H, ww = grp.W;
    auto view = [&](Tens& t) { Tens v = t; v.B = nb; return v; };
    Tens g = grp; g.B = nb;
    if (stage == ST_NORM0) return chan_stats_group(h, q, g, true, 0, (double)frames_before * hh * ww);
    Tens cn = view(P.cn), nxt = view(P.nxt), t32 = view(P.t32);
    RCHK(apply_norm(h, q, g, cn, st, N_DEC0));
    Tens* cur = &cn; Tens* other = &nxt;
    for (int f = 0; f < 3; ++f) {
        if (stage == ST_FILTER + f) {
            char pre[64];
            snprintf(pre, sizeof pre, "Decoder.Filter%d", f + 1);
            for (int gi = 0; gi < 2; ++gi) {       // FilterPredictor.compute (:161-172): mean over (B,HW) of down_sample(content)
                ConvCall c{cur, &t32, &h->conv[std::string(pre) + (gi ? ".F2" : ".F1") + ".down_sample.0"], hh, ww}; c.B = nb; RCHK(conv(h, q, c));
                RCHK(chan_stats_group(h, q, t32, false, gi, (double)frames_before * hh * ww));
            }
            return RRV_OK;
        }
        RCHK(pointwise(h, q, *cur, *other, nullptr, nullptr, false, &P.su[f], 1, nullptr, nullptr));   // + frame 0's residual (Q1)
        Tens* t = cur; cur = other; other = t;
    }
    if (stage == ST_NORM1) return chan_stats_group(h, q, *cur, true, 0, (double)frames_before * hh * ww);
    RCHK(apply_norm(h, q, *cur, *cur, st, N_DEC1, nullptr, 3));
    Tens xs[3], a[3], o[3];
    for (int k = 0; k < 3; ++k) { xs[k] = view(P.xs[k]); a[k] = view(P.a[k]); o[k] = view(P.o[k]); }
    // the statistics before `stage` are known; at `stage` the group's partial is merged and nothing further is launched
    const int rc = unfused_blocks(h, q, nb, *cur, xs, a, o, st, 0, false, true, [&](const Tens& t, int, int point) -> int {
        if (ST_BLOCKS + point != stage) return RRV_OK;
        RCHK(chan_stats_group(h, q, t, true, 0, (double)frames_before * t.H * t.W));
        return WALK_STOP;
    });
    if (rc != RRV_OK) return rc == WALK_STOP ? RRV_OK : rc;
    return fail(h, RRV_E_ARG, "stream_prefix: no such stage");
}

// Decoder.compute for one style over h->patches in groups of the plan's P.grp.B frames (rrv_compute)
int compute_style_streaming(rrv_handle h, const Seq& q, int sid) {
    StyleState& S = h->styles[sid];
    float* st = S.blob;
    PrepPlan& P = h->prep;
    const int B = (int)h->patches.size(), G = P.grp.B, hh = h->patch_h, ww = h->patch_w;
    const size_t img = P.grp.img_floats();
    const int stop = h->prep_stop;
    if (stop >= 0) S.computed = false;
    auto body = [&]() -> int {
        for (int stage = 0; stage < ST_COUNT; ++stage) {
            for (int g0 = 0; g0 < B; g0 += G) {
                const int nb = B - g0 < G ? B - g0 : G;
                for (int b = 0; b < nb; ++b)
                    HIPCHK(hipMemcpyAsync(P.grp.p + (size_t)b * img, h->patches[g0 + b], img * sizeof(float), hipMemcpyDeviceToDevice, q.stream));
                RCHK(stream_prefix(h, q, sid, P.grp, nb, stage, g0));
            }
            // the sync point: every frame has contributed
            if (stage == ST_NORM0) {
                RCHK(chan_stats_finish(h, q, 0, 512, (double)B * hh * ww, 1, st + SL.norm[N_DEC0]));
            } else if (stage >= ST_FILTER && stage < ST_FILTER + 3) {
                const int f = stage - ST_FILTER;
                for (int gi = 0; gi < 2; ++gi) {
                    RCHK(chan_stats_finish(h, q, gi, 32, (double)B * hh * ww, 0, h->prep_cmean));
                    hipLaunchKernelGGL(fc_filter_k, dim3(4), dim3(256), 0, q.stream, (const float*)h->fc_w[2 * f + gi], (const float*)h->fc_b[2 * f + gi],
                                       (const float*)h->prep_cmean, (const float*)(S.smean + (2 * f + gi) * 32), st + SL.filt[2 * f + gi]);
                    HIPCHK(hipGetLastError());
                }
                RCHK(fold_filters(h, q, st, f));
                h->active_src = -1;
                // KernelFilter.compute (:223-230): frame 0 alone passes through apply_filter; its residual u_f is what every frame receives (Q1)
                HIPCHK(hipMemcpyAsync(P.f0.p, h->patches[0], img * sizeof(float), hipMemcpyDeviceToDevice, q.stream));
                Tens cn0 = P.cn; cn0.B = 1;
                RCHK(apply_norm(h, q, P.f0, cn0, st, N_DEC0));
                for (int f2 = 0; f2 < f; ++f2) RCHK(pointwise(h, q, cn0, cn0, nullptr, nullptr, false, &P.su[f2], 1, nullptr, nullptr));
                ConvCall c{&cn0, &P.d32, &q.set->fold_down[f], hh, ww}; c.epi = E_LRELU; RCHK(conv(h, q, c));
                ConvCall cu{&P.d32, &P.su[f], &q.set->fold_up[f], hh, ww}; RCHK(conv(h, q, cu));
            } else if (stage == ST_NORM1) {
                RCHK(chan_stats_finish(h, q, 0, 512, (double)B * hh * ww, 1, st + SL.norm[N_DEC1]));
            } else {
                const int k = (stage - ST_BLOCKS) / 3, w = (stage - ST_BLOCKS) % 3;
                const BlkDesc& b = BLKS[k];
                const double N = (double)B * (hh << (k + 1)) * (ww << (k + 1));
                RCHK(chan_stats_finish(h, q, 0, b.cout, N, 1, st + SL.norm[w == 0 ? b.n1 : (w == 1 ? b.n2 : b.nada)]));
            }
            if (stage == stop && stop != ST_COUNT - 1) return WALK_STOP;
        }
        return RRV_OK;
    };
    int rc = body();
    const bool stopped = rc == WALK_STOP;      // rrv_debug_prep_stop
    if (stopped) rc = RRV_OK;
    if (rc == RRV_OK && h->debug) rc = debug_verify(h, "Decoder.compute (streaming)");
    (void)hipStreamSynchronize(q.stream);
    h->active_src = -1;
    if (rc == RRV_OK && !stopped) S.computed = true;
    if (rc == RRV_OK && !stopped) rc = filter_conditioning(h, S);
    return rc;
}

}  // namespace

// =============================================================================================
extern "C" {

// CUs that HSA_CU_MASK ("<gpu ids>:<cu ranges>[;...]", e.g. "0:0-127" or "0,1:0-31,64-95") leaves to `device`; 0 = not masked.
static int cu_mask_count(const char* env, int device, int n_cus) {
    if (!env || !*env) return 0;
    auto parse_list = [](const char* b, const char* e, int limit, std::vector<char>& hit) {     // "a-b,c" -> hit[]
        hit.assign((size_t)limit, 0);
        while (b < e) {
            char* q = nullptr;
            long lo = strtol(b, &q, 10), hi = lo;
            if (q == b) return false;
            if (q < e && *q == '-') { const char* r = q + 1; hi = strtol(r, &q, 10); if (q == r) return false; }
            for (long v = lo; v <= hi; ++v) if (v >= 0 && v < limit) hit[(size_t)v] = 1;
            b = (q < e && *q == ',') ? q + 1 : q;
            if (b < e && q == b) return false;
        }
        return true;
    };
    const char* p = env;
    while (*p) {
        const char* semi = strchr(p, ';');
        const char* end = semi ? semi : p + strlen(p);
        const char* colon = (const char*)memchr(p, ':', (size_t)(end - p));
        if (colon) {
            std::vector<char> gpus, cus;
            if (parse_list(p, colon, 64, gpus) && device < 64 && gpus[(size_t)device] && parse_list(colon + 1, end, n_cus, cus)) {
                int n = 0;
                for (char c : cus) n += c;
                return n;
            }
        }
        p = semi ? semi + 1 : end;
    }
    return 0;
}

int rrv_create(int device, rrv_handle* out) {
    if (!out) return RRV_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RRV_E_HIP;
    rrv_ctx* h = new rrv_ctx();
    h->dev = device;
    (void)rrv_yuv_input_matrix(RRV_YUV_BT601, 0, h->yuv_in.m8);
    (void)rrv_yuv_matrix(RRV_YUV_BT601, 0, h->yuv_out.m8);      // what players assume for untagged yuv420p
    bool ok = hipSetDevice(device) == hipSuccess;
    for (rrv_ctx::Slot& sl : h->slots) ok = ok && hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        delete h;
        return RRV_E_HIP;
    }
    ok = ok && hipStreamCreateWithFlags(&h->copy_in, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&h->copy_out, hipStreamNonBlocking) == hipSuccess;
    for (rrv_ctx::Slot& sl : h->slots) ok = ok && hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) == hipSuccess;
    for (auto& st : h->hstage)
        for (hipEvent_t* e : {&st.in_done, &st.k_done, &st.out_done}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    for (auto& st : h->hstage)
        for (hipEvent_t& e : st.piece_ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (const char* e = getenv("RRV_HOST_PHASE")) h->host_phase = atoi(e) != 0;
    if (const char* e = getenv("RRV_HOST_PIECE")) { const long n = atol(e); h->host_piece_px = (n < 0 ? 0 : n > 64 ? 64 : n) * 640L * 640L; }      // in 640 x 640 frames
    if (const char* e = getenv("RRV_TIMELINE")) h->tl.on = atoi(e) != 0;
    if (h->tl.on) {
        ok = ok && hipEventCreate(&h->tl.entry) == hipSuccess && hipEventCreate(&h->tl.first) == hipSuccess;
        for (int i = 0; i < rrv_ctx::Timeline::N; ++i) ok = ok && hipEventCreate(&h->tl.k_end[i]) == hipSuccess && hipEventCreate(&h->tl.d_end[i]) == hipSuccess;
    }
    // the dynamic-LDS opt-in is a per-device function attribute: set it for THIS device, whatever other handles did
    for (const ConvRow& e : CONV_ROWS)
        if (ok && e.attr) ok = e.attr() == hipSuccess;
    if (!ok) {
        delete h;
        return RRV_E_HIP;
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->n_cus = prop.multiProcessorCount;
        // The runtime reports the physical CU count also when HSA_CU_MASK leaves this process fewer: persistent grids and the
        // rounds arithmetic of use_f43 follow the CUs the process can actually run on (RRV_CUS overrides both).
        const int masked = cu_mask_count(getenv("HSA_CU_MASK"), device, h->n_cus);
        if (masked > 0 && masked < h->n_cus) h->n_cus = masked;
        if (const char* e = getenv("RRV_CUS")) { const int n = atoi(e); if (n >= 1 && n <= 1024) h->n_cus = n; }
    }
    if (const char* e = getenv("RRV_F43_LAYERS")) h->f43_layers = (unsigned)strtoul(e, nullptr, 0);
    if (const char* e = getenv("RRV_DIRECT_LAYERS")) h->direct_layers = (unsigned)strtoul(e, nullptr, 0);
    if (const char* e = getenv("RRV_P8")) h->p8 = atoi(e) & 3;
    if (const char* e = getenv("RRV_F43")) h->f43_mode = atoi(e) < 0 ? 0 : (atoi(e) > 2 ? 2 : atoi(e));
    if (const char* e = getenv("RRV_DEBUG")) h->debug = atoi(e) < 0 ? 0 : (atoi(e) > 2 ? 2 : atoi(e));
    *out = h;
    return RRV_OK;
}

static void free_plans(rrv_handle h) {
    for (rrv_ctx::Slot& sl : h->slots) for (EncPlan& e : sl.enc) enc_free(e);
    enc_free(h->enc_add); enc_free(h->enc_style);
    for (rrv_ctx::Slot& sl : h->slots) for (DecPlan& d : sl.dec) dec_free(h, d);
    prep_free(h);
}

int rrv_set_debug(rrv_handle h, int level) {
    if (!h || level < 0 || level > 2) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    free_plans(h);          // workspaces are re-allocated with (or without) guard bands on next use; styles keep their maps
    h->debug = level;
    return RRV_OK;
}

int rrv_debug_fail_alloc(rrv_handle h, int nth) {
    if (!h || nth < 0) return RRV_E_ARG;
    h->fail_alloc_in = nth;
    return RRV_OK;
}

__global__ void dbg_poke_k(float* p, long off) { p[off] = 1.0f; }
// the checker checks itself: one store into a ring pixel and one into a guard band must both be reported
int rrv_debug_selftest(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    const int saved = h->debug;
    h->debug = 2;
    const Seq q = base_seq(h);
    Tens t;
    int rc = talloc(h, q, &t, 2, 8, 8, 64);
    if (rc == RRV_OK) rc = debug_verify(h, "selftest (clean)");
    int caught = 0;
    if (rc == RRV_OK) {
        hipLaunchKernelGGL(dbg_poke_k, dim3(1), dim3(1), 0, q.stream, t.p, (long)t.img_floats() + 5);       // ring pixel (0,0) of image 1
        if (debug_verify(h, "selftest (ring)") == RRV_E_DEBUG) ++caught;
        HIPCHK(hipMemsetAsync(t.p + t.img_floats(), 0, 64 * sizeof(float), q.stream));
        hipLaunchKernelGGL(dbg_poke_k, dim3(1), dim3(1), 0, q.stream, t.p, -3L);                            // guard band in front
        if (debug_verify(h, "selftest (guard)") == RRV_E_DEBUG) ++caught;
    }
    tfree(&t);
    h->debug = saved;
    if (rc != RRV_OK) return rc;
    if (caught != 2) return fail(h, RRV_E_DEBUG, "debug selftest: a deliberate out-of-bounds store was not detected");
    h->err.clear();
    return RRV_OK;
}

int rrv_destroy(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    (void)hipSetDevice(h->dev);
    (void)hipDeviceSynchronize();
    // device memory is released with the process / context; free the big pieces explicitly
    for (auto& kv : h->conv) {
        if (kv.second.raw) (void)hipFree(kv.second.raw);
        if (kv.second.pk) (void)hipFree(kv.second.pk);
        if (kv.second.pk_ups) (void)hipFree(kv.second.pk_ups);
        if (kv.second.pk_ups_sc) (void)hipFree(kv.second.pk_ups_sc);
        if (kv.second.pk_wino) (void)hipFree(kv.second.pk_wino);
        if (kv.second.pk_f43) (void)hipFree(kv.second.pk_f43);
        if (kv.second.bias && kv.second.bias != h->zero_bias) (void)hipFree(kv.second.bias);
    }
    if (h->zero_bias) (void)hipFree(h->zero_bias);
    // the state sets live in one allocation per kind; set 0 holds the base pointers (rrv_finalize_weights)
    for (int f = 0; f < 3; ++f) {
        const ConvW &fd = h->sets[0].fold_down[f], &fu = h->sets[0].fold_up[f];
        for (float* q : {fd.raw, fd.bias, fd.pk_wino, fu.raw, fu.pk_wino}) if (q) (void)hipFree(q);
    }
    if (h->sets[0].active) (void)hipFree(h->sets[0].active);
    for (int i = 0; i < 6; ++i) { if (h->fc_w[i]) (void)hipFree(h->fc_w[i]); if (h->fc_b[i]) (void)hipFree(h->fc_b[i]); }
    if (h->fold_tmp) (void)hipFree(h->fold_tmp);
    for (float* p : h->patches) (void)hipFree(p);
    for (auto& f : h->features) if (f.owned) { if (f.p) (void)hipFree(f.p); if (f.u8) (void)hipFree(f.u8); }
    for (void* b : h->feat_blocks) (void)hipFree(b);
    free_plans(h);
    for (StyleState& s : h->styles) { if (s.blob) (void)hipFree(s.blob); if (s.smean) (void)hipFree(s.smean); tfree(&s.map); }
    if (h->d_u8) (void)hipFree(h->d_u8);
    if (h->pend_u8) (void)hipFree(h->pend_u8);
    for (rrv_ctx::Slot& sl : h->slots) if (sl.rs_buf) (void)hipFree(sl.rs_buf);
    for (rrv_ctx::Slot& sl : h->slots) if (sl.dl_buf) (void)hipFree(sl.dl_buf);
    for (rrv_ctx::Slot& sl : h->slots)
        for (float* q : {sl.gd_xhi, sl.gd_ab, sl.gd_q, sl.pc_canvas}) if (q) (void)hipFree(q);
    for (float* q : {h->gd_ab, h->gd_q, h->cm_buf}) if (q) (void)hipFree(q);
    for (void* q : {(void*)h->jp_coef, (void*)h->jp_idx, (void*)h->jd_frames, (void*)h->jd_ivl, (void*)h->jd_coef, (void*)h->jd_planes, (void*)h->jd_streams,
                    (void*)h->jd_status, (void*)h->jd_out, (void*)h->jd_matte, (void*)h->sg_thumb, (void*)h->sg_in, (void*)h->sg_sig,
                    (void*)h->pc_frames, (void*)h->pc_part, (void*)h->pc_in, (void*)h->pc_prof}) if (q) (void)hipFree(q);
    if (h->jd_pin) (void)hipHostFree(h->jd_pin);
    if (h->jd_ev) (void)hipEventDestroy(h->jd_ev);
    for (rrv_ctx::Slot& sl : h->slots)
        for (void* q : {(void*)sl.jp_coef, (void*)sl.jp_idx}) if (q) (void)hipFree(q);
    for (auto& kv : h->rs_tabs) if (kv.second.block) (void)hipFree(kv.second.block);
    if (h->stat_part) (void)hipFree(h->stat_part);
    for (float* q : {h->first_w[0], h->first_w[1], h->first_b[0], h->first_b[1], h->first_wg}) if (q) (void)hipFree(q);
    for (auto& st : h->hstage) {
        stage_free(st.pin, true);
        stage_free(st.dev, false);
        if (st.mask) (void)hipFree(st.mask);
        if (st.mask_pin) (void)hipHostFree(st.mask_pin);
        for (hipEvent_t e : {st.in_done, st.k_done, st.out_done}) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : st.piece_ev) if (e) (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : {h->tl.entry, h->tl.first}) if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < rrv_ctx::Timeline::N; ++i)
        for (hipEvent_t e : {h->tl.k_end[i], h->tl.d_end[i]}) if (e) (void)hipEventDestroy(e);
    if (h->copy_in) (void)hipStreamDestroy(h->copy_in);
    if (h->copy_out) (void)hipStreamDestroy(h->copy_out);
    for (ProfEntry& e : h->prof) { (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); }
    for (rrv_ctx::Slot& sl : h->slots) { (void)hipStreamDestroy(sl.stream); if (sl.ev) (void)hipEventDestroy(sl.ev); }
    delete h;
    return RRV_OK;
}

const char* rrv_last_error(rrv_handle h) { return h ? h->err.c_str() : "null handle"; }

int rrv_load_weight(rrv_handle h, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!h || !key || !data || !shape || ndim < 1 || ndim > 4) return RRV_E_ARG;
    if (h->finalized) return fail(h, RRV_E_WEIGHTS, "weights already finalized");
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    h->hostw[key].assign(data, data + n);
    h->hostshape[key].assign(shape, shape + ndim);
    return RRV_OK;
}

int rrv_finalize_weights(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    if (h->finalized) return RRV_OK;
    HIPCHK(hipSetDevice(h->dev));
    const Seq q = base_seq(h);
    RCHK(dalloc(h, q, &h->zero_bias, 512, true));
    {   // the fixed-size scratch (rrv_ctx::stat_part ..): 1024 partial blocks x 3 x 512 channels at most per partial buffer
        constexpr size_t PART = (size_t)1024 * 3 * 512, ACC = (size_t)2 * 4 * 512, FLOATS = 512 + 64;
        float* base;
        RCHK(dalloc(h, q, &base, (2 * PART + ACC) * 2 + FLOATS));
        h->stat_part = (double*)base; h->stat_part2 = h->stat_part + PART; h->stat_acc = h->stat_part2 + PART;
        h->stat_mean = (float*)(h->stat_acc + ACC); h->prep_cmean = h->stat_mean + 512;
    }
    for (int which = 0; which < 2; ++which) {
        for (int i = 0; i < 9; ++i) {
            const std::string k = enc_key(which, i);
            if (i == 0) {
                float* raw = nullptr;
                RCHK(upload(h, q, k + ".weight", &raw, 64 * 27));
                RCHK(dalloc(h, q, &h->first_w[which], 27 * 64, false));
                hipLaunchKernelGGL(pack_first_k, dim3(7), dim3(256), 0, q.stream, (const float*)raw, h->first_w[which]);
                HIPCHK(hipGetLastError());
                RCHK(upload(h, q, k + ".bias", &h->first_b[which], 64));
                if (which == 0) {
                    RCHK(dalloc(h, q, &h->first_wg, 1216, false));
                    hipLaunchKernelGGL(pack_first_grey_k, dim3(3), dim3(256), 0, q.stream, (const float*)raw, (const float*)h->first_b[0], h->first_wg);
                    HIPCHK(hipGetLastError());
                }
                HIPCHK(hipStreamSynchronize(q.stream));
                (void)hipFree(raw);
            } else {
                RCHK(make_conv(h, q, k, VGG_COUT[i], VGG_CIN[i], 9, true));
                // per-frame encoder, conv1_2 .. conv3_4 (conv4_1 = 256 -> 512 stays on F(2x2,3x3): alone it costs more of the
                // parity margin than the other ten layers together, profiles/r03_f43_numerics.txt, for 3.5 % of the frame)
                if (which == 0 && i < 8) { h->conv[k].f43_bit = i - 1; RCHK(pack_f43(h, q, h->conv[k])); }
            }
        }
    }
    for (int b = 0; b < 3; ++b) {
        const std::string p = std::string("Decoder.") + BLKS[b].name;
        const int cout = BLKS[b].cout, cin = 2 * cout;      // (each block halves the channels)
        RCHK(make_conv(h, q, p + ".conv1", cout, cin, 9, true, false));
        RCHK(pack_ups(h, q, h->conv[p + ".conv1"]));
        RCHK(make_conv(h, q, p + ".conv2", cout, cout, 9, true));
        h->conv[p + ".conv2"].f43_bit = 7 + b;
        RCHK(pack_f43(h, q, h->conv[p + ".conv2"]));
        RCHK(make_conv(h, q, p + ".conv_shortcut", cout, cin, 1, false));
        RCHK(pack_ups_sc(h, q, h->conv[p + ".conv1"], h->conv[p + ".conv_shortcut"]));
    }
    {
        float* raw = nullptr;
        RCHK(upload(h, q, "Decoder.slice1.weight", &raw, 3 * 64 * 9));
        RCHK(dalloc(h, q, &h->last_w, 2 * 4 * 64 * 4, false));
        hipLaunchKernelGGL(pack_last_k, dim3(8), dim3(256), 0, q.stream, (const float*)raw, h->last_w);
        HIPCHK(hipGetLastError());
        RCHK(dalloc(h, q, &h->last_b, 4, true));
        auto it = h->hostw.find("Decoder.slice1.bias");
        if (it == h->hostw.end() || it->second.size() != 3) return fail(h, RRV_E_WEIGHTS, "missing weight Decoder.slice1.bias");
        HIPCHK(hipMemcpyAsync(h->last_b, it->second.data(), 3 * sizeof(float), hipMemcpyHostToDevice, q.stream));
        HIPCHK(hipStreamSynchronize(q.stream));
        (void)hipFree(raw);
    }
    for (int f = 0; f < 3; ++f) {
        char pre[64];
        snprintf(pre, sizeof pre, "Decoder.Filter%d", f + 1);
        RCHK(make_conv(h, q, std::string(pre) + ".down_sample.0", 32, 512, 9, true, false));
        RCHK(make_conv(h, q, std::string(pre) + ".upsample.0", 512, 32, 9, true, false));
        // the masked multi-style entries run both layers unfolded, around mask_filter_k, on the row-split transform-domain kernel
        RCHK(pack_wino(h, q, h->conv[std::string(pre) + ".down_sample.0"]));
        RCHK(pack_wino(h, q, h->conv[std::string(pre) + ".upsample.0"]));
        for (int g = 0; g < 2; ++g) {
            const std::string fp = std::string(pre) + (g ? ".F2" : ".F1");
            RCHK(make_conv(h, q, fp + ".down_sample.0", 32, 512, 9, true));
            RCHK(upload(h, q, fp + ".FC.weight", &h->fc_w[2 * f + g], 1024 * 64));
            RCHK(upload(h, q, fp + ".FC.bias", &h->fc_b[2 * f + g], 1024));
        }
        {   // folded KernelFilter weights of every state set, set-major inside one allocation per kind
            constexpr int NS = rrv_ctx::N_SETS;
            float *fd_raw, *fd_bias, *fd_pkw, *fu_raw, *fu_pkw;
            RCHK(dalloc(h, q, &fd_raw, (size_t)NS * 32 * 512 * 9)); RCHK(dalloc(h, q, &fd_bias, (size_t)NS * 256));      // bias[32], then zeros: the split-K slabs' bias
            RCHK(dalloc(h, q, &fd_pkw, (size_t)NS * 32 * 512 * 16));
            RCHK(dalloc(h, q, &fu_raw, (size_t)NS * 512 * 32 * 9)); RCHK(dalloc(h, q, &fu_pkw, (size_t)NS * 512 * 32 * 16));
            for (int i = 0; i < NS; ++i) {
                ConvW& fd = h->sets[i].fold_down[f];
                fd.Cout = 32; fd.Cin = 512; fd.taps = 9; fd.BN = 32;
                fd.raw = fd_raw + (size_t)i * 32 * 512 * 9; fd.bias = fd_bias + (size_t)i * 256; fd.pk_wino = fd_pkw + (size_t)i * 32 * 512 * 16;
                ConvW& fu = h->sets[i].fold_up[f];
                fu.Cout = 512; fu.Cin = 32; fu.taps = 9; fu.BN = 128;
                fu.raw = fu_raw + (size_t)i * 512 * 32 * 9; fu.pk_wino = fu_pkw + (size_t)i * 512 * 32 * 16;
                fu.bias = h->conv[std::string(pre) + ".upsample.0"].bias;
            }
        }
    }
    {
        float* act;
        RCHK(dalloc(h, q, &act, (size_t)rrv_ctx::N_SETS * RRV_STATE_FLOATS));
        for (int i = 0; i < rrv_ctx::N_SETS; ++i) h->sets[i].active = act + (size_t)i * RRV_STATE_FLOATS;
    }
    HIPCHK(hipStreamSynchronize(q.stream));
    h->hostw.clear();
    h->finalized = true;
    return RRV_OK;
}

// ---- descriptors and layouts -> formats: one parser each way, used by every entry.  A parser says what was wrong; each entry family
// words its own refusal (the texts are part of what callers see).
enum class DescErr { OK, UNKNOWN /* a dtype, layout or space that does not exist here */, U8_SPACE /* uint8 outside PIXEL */,
                     YUV_TYPE /* a YUV layout with another dtype or space than its own */, LAYOUT /* not a YUV 4:2:0 layout */ };
static bool desc_known(const rrv_image_desc& d, bool yuv) {
    return (d.dtype == RRV_DT_U8 || d.dtype == RRV_DT_F32 || (d.dtype == RRV_DT_U16 && yuv)) &&
           (d.layout == RRV_LAY_HWC_BGR || d.layout == RRV_LAY_CHW_RGB || yuv) && d.space >= RRV_SP_PIXEL && d.space <= RRV_SP_NORM;
}
// an input descriptor (the torch-pipeline entries, the style image, the sampled frames): conv_first_k's form and value space
static DescErr parse_in(const rrv_image_desc& d, InFmt* in) {
    if (!desc_known(d, false)) return DescErr::UNKNOWN;      // (a YUV input goes through the _from_yuv entries)
    if (d.dtype == RRV_DT_U8 && d.space != RRV_SP_PIXEL) return DescErr::U8_SPACE;
    *in = InFmt{(d.dtype == RRV_DT_F32 ? IN_F32_HWC : IN_U8_HWC) | (d.layout == RRV_LAY_CHW_RGB ? 1 : 0), d.space};
    return DescErr::OK;
}
// a layout / in_layout of the _yuv / _from_yuv entries: 8-bit YUV 4:2:0 or uint16 samples, integer codes of the PIXEL values (the depth and the
// matrix are read when the kernel is launched)
// The chroma format (RRV_LAY_422 / RRV_LAY_444 on the layout) travels next to the form / base layout, in InFmt::cs / OutFmt::cs.
static DescErr parse_in_yuv(int layout, InFmt* in) {
    if (!yuv_layout(layout)) return DescErr::LAYOUT;
    const int base = yuv_base(layout);
    *in = InFmt{base == RRV_LAY_I420 ? IN_YUV_I420 : base == RRV_LAY_NV12 ? IN_YUV_NV12 : base == RRV_LAY_I420_16 ? IN_YUV_I420_16 : IN_YUV_P016, SP_PIXEL,
                yuv_chroma(layout)};
    return DescErr::OK;
}
static DescErr parse_out_yuv(int layout, OutFmt* out) {
    if (!yuv_layout(layout)) return DescErr::LAYOUT;
    *out = OutFmt{true, false, SP_PIXEL, yuv_base(layout), yuv_chroma(layout)};
    return DescErr::OK;
}
// an output descriptor: HWC BGR / CHW RGB, or YUV as uint8 I420 / NV12 or uint16 RRV_LAY_I420_16 / RRV_LAY_P016 (each 4:2:0, or 4:2:2 / 4:4:4 by its flag) in the PIXEL space
static DescErr parse_out(const rrv_image_desc& d, OutFmt* out) {
    const bool is_yuv = parse_out_yuv(d.layout, out) == DescErr::OK;
    if (!desc_known(d, is_yuv)) return DescErr::UNKNOWN;
    if (is_yuv && (d.dtype != (yuv16_layout(d.layout) ? RRV_DT_U16 : RRV_DT_U8) || d.space != RRV_SP_PIXEL)) return DescErr::YUV_TYPE;
    if (d.dtype == RRV_DT_U8 && d.space != RRV_SP_PIXEL) return DescErr::U8_SPACE;
    if (!is_yuv) *out = OutFmt{d.dtype == RRV_DT_U8, d.layout == RRV_LAY_CHW_RGB, d.space};
    return DescErr::OK;
}
static int refuse_layout(rrv_handle h, const char* what) {      // what: "<entry family>: in_layout" / "<entry family>: layout"
    return fail(h, RRV_E_ARG, std::string(what) + " must be RRV_LAY_I420, RRV_LAY_NV12, RRV_LAY_I420_16 or RRV_LAY_P016, alone or with one of RRV_LAY_422 / RRV_LAY_444");
}

// ---- image views (include/rerevst_hip.h rrv_image_view): pure arithmetic, no handle and no GPU
// rule 3: a dtype / layout / space combination the descriptor entries accept, on either side
static bool view_desc_ok(const rrv_image_desc& d) {
    if (yuv_layout(d.layout)) return d.dtype == (yuv16_layout(d.layout) ? RRV_DT_U16 : RRV_DT_U8) && d.space == RRV_SP_PIXEL;
    if (d.layout != RRV_LAY_HWC_BGR && d.layout != RRV_LAY_CHW_RGB) return false;
    if (d.dtype == RRV_DT_U8) return d.space == RRV_SP_PIXEL;
    return d.dtype == RRV_DT_F32 && d.space >= RRV_SP_PIXEL && d.space <= RRV_SP_NORM;
}
static int view_layout(const rrv_image_desc& d) {
    return d.layout == RRV_LAY_HWC_BGR ? VL_HWC : d.layout == RRV_LAY_CHW_RGB ? VL_CHW :
           yuv_base(d.layout) == RRV_LAY_I420 || yuv_base(d.layout) == RRV_LAY_I420_16 ? VL_I420 : VL_NV12;
}
static int view_chroma(const rrv_image_desc& d) { return yuv_layout(d.layout) ? yuv_chroma(d.layout) : CS_420; }      // (of a known descriptor)
// the planes of an H x W frame: how many, and the row length (elements) and row count of each
struct Planes { int n; int64_t len[3], rows[3]; };
static Planes view_planes(int vl, int64_t H, int64_t W, int cs) {      // cs: the chroma format of the two YUV structures (CS_*)
    const int64_t CH = (H + chroma_sy(cs)) >> chroma_sy(cs), CW = (W + chroma_sx(cs)) >> chroma_sx(cs);
    switch (vl) {
    case VL_HWC:  return Planes{1, {3 * W, 0, 0}, {H, 0, 0}};
    case VL_CHW:  return Planes{3, {W, W, W}, {H, H, H}};
    case VL_I420: return Planes{3, {W, CW, CW}, {H, CH, CH}};
    default:      return Planes{2, {W, 2 * CW, 0}, {H, CH, 0}};
    }
}
// the contiguous view of a known descriptor; sizes are not judged here (the entries refuse a frame size in their own words)
static rrv_image_view contiguous_of(const rrv_image_desc& d, int H, int W) {
    const ImgView c = contiguous_view(view_layout(d), H > 0 ? H : 0, W > 0 ? W : 0, view_chroma(d));
    return rrv_image_view{d, c.fs, {c.off[0], c.off[1], c.off[2]}, {(int64_t)c.pitch[0], (int64_t)c.pitch[1], (int64_t)c.pitch[2]}};
}
// the four rules; *why (optional) receives the offending field and what is wrong with it
static bool view_check(const rrv_image_view& v, int B, int H, int W, bool output, std::string* why) {
    auto no = [&](const std::string& field, const char* what) { if (why) *why = field + " " + what; return false; };
    auto idx = [](const char* name, int k) { return std::string(name) + "[" + std::to_string(k) + "]"; };
    if (!view_desc_ok(v.desc)) return no("desc", "is not a dtype, layout and space combination the descriptor entries accept");
    if (B < 1 || H < 1 || W < 1) return no("B, H, W", "must be at least 1");
    const Planes pl = view_planes(view_layout(v.desc), H, W, view_chroma(v.desc));
    // upper bounds, so that nothing below (and no address in the kernels) can wrap: a pitch fits 31 bits, an offset or a frame stride 40
    const int64_t PITCH_MAX = INT32_MAX, SPAN_MAX = (int64_t)1 << 40;
    if (v.frame_stride < 0) return no("frame_stride", "is negative");
    if (v.frame_stride > SPAN_MAX) return no("frame_stride", "is above 2^40 elements");
    for (int k = 0; k < pl.n; ++k) {
        if (v.plane_offset[k] < 0) return no(idx("plane_offset", k), "is negative");
        if (v.plane_offset[k] > SPAN_MAX) return no(idx("plane_offset", k), "is above 2^40 elements");
        if (v.pitch[k] < 0) return no(idx("pitch", k), "is negative");
        if (v.pitch[k] > PITCH_MAX) return no(idx("pitch", k), "is above 2^31 - 1 elements");
        if (v.pitch[k] < pl.len[k]) return no(idx("pitch", k), "is shorter than a row of the plane");
    }
    if (!output) return true;
    int64_t end[3], last = 0;
    for (int k = 0; k < pl.n; ++k) {
        end[k] = v.plane_offset[k] + (pl.rows[k] - 1) * v.pitch[k] + pl.len[k];
        last = std::max(last, end[k]);
    }
    for (int k = 1; k < pl.n; ++k)
        for (int j = 0; j < k; ++j)
            if (v.plane_offset[k] < end[j] && v.plane_offset[j] < end[k]) return no(idx("plane_offset", k), "overlaps another plane of the output frame");
    if (B > 1 && v.frame_stride < last) return no("frame_stride", "is smaller than the extent of one output frame");
    return true;
}
int rrv_image_view_contiguous(rrv_image_desc d, int H, int W, rrv_image_view* v) {
    if (!v || !view_desc_ok(d) || H < 1 || W < 1) return RRV_E_ARG;
    *v = contiguous_of(d, H, W);
    return RRV_OK;
}
int rrv_image_view_check(const rrv_image_view* v, int B, int H, int W, int output) {
    return v && view_check(*v, B, H, W, output != 0, nullptr) ? RRV_OK : RRV_E_ARG;
}

// slot 0's stream waits for what `stream` (NULL: the null stream) holds so far
static int wait_for_stream(rrv_handle h, hipStream_t stream) {
    HIPCHK(hipEventRecord(h->slots[0].ev, stream));
    HIPCHK(hipStreamWaitEvent(h->slots[0].stream, h->slots[0].ev, 0));
    return RRV_OK;
}

// device: `style` is in HBM in the format `in`, complete once `stream` has run what it holds now; else host uint8 BGR HWC
static int prepare_style(rrv_handle h, const void* style, bool device, InFmt in, hipStream_t stream, int Hs, int Ws, int sid) {
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    const Seq q = base_seq(h);
    StyleState& S = h->styles[sid];
    if (!S.blob) RCHK(dalloc(h, q, &S.blob, RRV_STATE_FLOATS));
    if (device) {
        RCHK(wait_for_stream(h, stream));
    } else {
        RCHK(ensure_dev(h, h->d_u8, h->d_u8_cap, (size_t)Hs * Ws * 3));
        HIPCHK(hipMemcpyAsync(h->d_u8, style, (size_t)Hs * Ws * 3, hipMemcpyHostToDevice, q.stream));
    }
    RCHK(enc_plan(h, q, h->enc_style, 1, Hs, Ws));
    EncPlan& e = h->enc_style;
    const int rc_enc = run_encoder(h, q, e, device ? (const uint8_t*)style : h->d_u8, in, 1, nullptr, nullptr, 1);
    if (rc_enc != RRV_OK) { (void)hipStreamSynchronize(q.stream); return rc_enc; }      // (the caller's image is not read after the call returns)
    // cal_mean_std at relu1_1..relu4_1 (style_network_global.py:304-331)
    const Tens* taps[4] = {&e.c11, &e.c21, &e.c31, &e.c41};
    for (int k = 0; k < 4; ++k) RCHK(chan_stats(h, q, *taps[k], 2, S.blob + SL.sty[k]));
    RCHK(talloc(h, q, &S.map, 1, e.c41.H, e.c41.W, 512));
    HIPCHK(hipMemcpyAsync(S.map.p, e.c41.p, e.c41.img_floats() * sizeof(float), hipMemcpyDeviceToDevice, q.stream));
    {   // FilterPredictor's style half (:161-172 with normalized_style :397): mean_{HW} F.down_sample((map - mean)/std), 6 x 32 values
        if (!S.smean) RCHK(dalloc(h, q, &S.smean, 6 * 32));
        Tens sn, ts32;
        int rc = talloc(h, q, &sn, 1, S.map.H, S.map.W, 512);
        if (rc == RRV_OK) rc = talloc(h, q, &ts32, 1, S.map.H, S.map.W, 32);
        if (rc == RRV_OK) rc = pointwise(h, q, S.map, sn, S.blob + SL.sty[3], S.blob + SL.sty[3] + 512, true, nullptr, 0, nullptr, nullptr);
        for (int f = 0; f < 3 && rc == RRV_OK; ++f)
            for (int g = 0; g < 2 && rc == RRV_OK; ++g) {
                char key[96];
                snprintf(key, sizeof key, "Decoder.Filter%d.F%d.down_sample.0", f + 1, g + 1);
                ConvCall cs{&sn, &ts32, &h->conv[key], sn.H, sn.W};
                rc = conv(h, q, cs);
                if (rc == RRV_OK) rc = chan_stats(h, q, ts32, 0, S.smean + (2 * f + g) * 32);
            }
        (void)hipStreamSynchronize(q.stream);
        tfree(&sn); tfree(&ts32);
        if (rc != RRV_OK) return rc;
    }
    HIPCHK(hipStreamSynchronize(q.stream));
    if (h->debug) RCHK(debug_verify(h, "prepare_style"));
    S.prepared = true; S.computed = false;
    if (h->active_src == sid) h->active_src = -1;
    return RRV_OK;
}

int rrv_prepare_style(rrv_handle h, const uint8_t* style, int Hs, int Ws, int sid) {
    if (!h || !style || Hs < 8 || Ws < 8 || sid < 0 || sid >= RRV_MAX_STYLES) return RRV_E_ARG;
    return prepare_style(h, style, false, IN_BGR8, nullptr, Hs, Ws, sid);
}
int rrv_prepare_style_image_device(rrv_handle h, const void* d_style, rrv_image_desc in, int Hs, int Ws, int sid, void* hip_stream) {
    if (!h || !d_style || Hs < 8 || Ws < 8 || sid < 0 || sid >= RRV_MAX_STYLES) return RRV_E_ARG;
    InFmt fmt;
    if (parse_in(in, &fmt) != DescErr::OK) return fail(h, RRV_E_ARG, "prepare_style: unknown dtype, layout or space (uint8 is PIXEL only)");
    return prepare_style(h, d_style, true, fmt, (hipStream_t)hip_stream, Hs, Ws, sid);
}

int rrv_clean(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    (void)hipSetDevice(h->dev);
    (void)sync_all(h);
    for (float* p : h->patches) (void)hipFree(p);
    h->patches.clear();
    prep_free(h);      // (a plan kept by rrv_debug_prep_stop)
    h->pend_n = 0;
    h->patch_h = h->patch_w = h->add_H = h->add_W = 0;
    for (StyleState& s : h->styles) s.computed = false;
    h->illcond = false;
    h->active_src = -1;
    h->user_style = -1;
    return RRV_OK;
}

// encode the frames collected by rrv_add (all H x W = add_H x add_W) and append their relu4_1 features to h->patches
static int flush_pending(rrv_handle h) {
    if (!h->pend_n) return RRV_OK;
    const Seq q = base_seq(h);
    const int H = h->add_H, W = h->add_W;
    const size_t fb = in_frame_bytes(h->pend_in.form, H, W, h->pend_in.cs);
    const int PB = h->pend_n < 8 ? h->pend_n : 8;        // one plan; the last group may use fewer of its images
    RCHK(enc_plan(h, q, h->enc_add, PB, H, W));
    for (int k0 = 0; k0 < h->pend_n; k0 += PB) {
        const int nb = h->pend_n - k0 < PB ? h->pend_n - k0 : PB;
        RCHK(run_encoder(h, q, h->enc_add, h->pend_u8 + (size_t)k0 * fb, h->pend_in, 0, nullptr, nullptr, nb));      // the pending frames are kept in the format they arrived in
        const Tens& f = h->enc_add.c41;
        for (int b = 0; b < nb; ++b) {
            float* keep = nullptr;
            RCHK(dalloc(h, q, &keep, f.img_floats(), false));
            HIPCHK(hipMemcpyAsync(keep, f.p + (size_t)b * f.img_floats(), f.img_floats() * sizeof(float), hipMemcpyDeviceToDevice, q.stream));
            h->patches.push_back(keep);
        }
        h->patch_h = f.H; h->patch_w = f.W;
    }
    HIPCHK(hipStreamSynchronize(q.stream));
    h->pend_n = 0;
    return RRV_OK;
}

// `frame` is in the format `in`.  device: in HBM, complete once `stream` has run what it holds now; else in host memory
// view (device frames only): the frame's rows are where it says; they are compacted into the pending buffer, one 2-D copy per plane
static int add_frame(rrv_handle h, const void* frame, bool device, InFmt in, hipStream_t stream, int H, int W, const rrv_image_view* view = nullptr) {
    RCHK(check_frame(h, H, W, "add"));
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    HIPCHK(hipSetDevice(h->dev));
    if ((!h->patches.empty() || h->pend_n) && (H != h->add_H || W != h->add_W))
        return fail(h, RRV_E_ARG, "add: all sampled frames must have the same size");
    if (h->pend_n && in != h->pend_in) {      // one encoder launch reads one format: encode the pending ones first
        RCHK(sync_all(h));
        RCHK(flush_pending(h));
    }
    h->pend_in = in;
    const size_t fb = in_frame_bytes(in.form, H, W, in.cs);
    if ((size_t)(h->pend_n + 1) * fb > h->pend_cap) {      // grow (x2) keeping the frames already collected
        const size_t cap = ((size_t)(h->pend_n + 1) * fb) * 2 > 16 * fb ? ((size_t)(h->pend_n + 1) * fb) * 2 : 16 * fb;
        uint8_t* nw = nullptr;
        RCHK(dmalloc(h, (void**)&nw, cap));
        if (h->pend_n) HIPCHK(hipMemcpy(nw, h->pend_u8, (size_t)h->pend_n * fb, hipMemcpyDeviceToDevice));
        if (h->pend_u8) (void)hipFree(h->pend_u8);
        h->pend_u8 = nw; h->pend_cap = cap;
    }
    if (device) {      // in the order of the caller's stream, and consumed before the call returns
        RCHK(wait_for_stream(h, stream));
        uint8_t* const dst = h->pend_u8 + (size_t)h->pend_n * fb;
        const hipStream_t s0 = h->slots[0].stream;
        if (view) {
            const int vl = in_view_layout(in.form);
            const size_t el = in_elem(in.form);
            const ImgView c = contiguous_view(vl, H, W, in.cs);
            const Planes pl = view_planes(vl, H, W, in.cs);
            for (int k = 0; k < pl.n; ++k)
                HIPCHK(hipMemcpy2DAsync(dst + (size_t)c.off[k] * el, (size_t)c.pitch[k] * el, (const char*)frame + (size_t)view->plane_offset[k] * el,
                                        (size_t)view->pitch[k] * el, (size_t)pl.len[k] * el, (size_t)pl.rows[k], hipMemcpyDeviceToDevice, s0));
        } else {
            HIPCHK(hipMemcpyAsync(dst, frame, fb, hipMemcpyDeviceToDevice, s0));
        }
        HIPCHK(hipStreamSynchronize(s0));
    } else {
        HIPCHK(hipMemcpy(h->pend_u8 + (size_t)h->pend_n * fb, frame, fb, hipMemcpyHostToDevice));
    }
    h->pend_n += 1;
    h->add_H = H; h->add_W = W;
    return RRV_OK;
}

int rrv_add(rrv_handle h, const uint8_t* frame, int H, int W) {
    if (!h || !frame) return RRV_E_ARG;
    return add_frame(h, frame, false, IN_BGR8, nullptr, H, W);
}
int rrv_add_image_device(rrv_handle h, const void* d_frame, rrv_image_desc in, int H, int W, void* hip_stream) {
    if (!h || !d_frame) return RRV_E_ARG;
    InFmt fmt;
    if (parse_in(in, &fmt) != DescErr::OK) return fail(h, RRV_E_ARG, "add: unknown dtype, layout or space (uint8 is PIXEL only)");
    return add_frame(h, d_frame, true, fmt, (hipStream_t)hip_stream, H, W);
}

// a view's descriptor as conv_first_k's form: every layout, the YUV ones included
static bool parse_in_view(const rrv_image_desc& d, InFmt* in) {
    if (!view_desc_ok(d)) return false;
    return (yuv_layout(d.layout) ? parse_in_yuv(d.layout, in) : parse_in(d, in)) == DescErr::OK;
}
int rrv_add_view_device(rrv_handle h, const void* d_frame, const rrv_image_view* in, int H, int W, void* hip_stream) {
    if (!h || !d_frame || !in) return RRV_E_ARG;
    InFmt fmt;
    if (!parse_in_view(in->desc, &fmt)) return fail(h, RRV_E_ARG, "add_view: in.desc is not a dtype, layout and space combination the descriptor entries accept");
    RCHK(check_frame(h, H, W, "add"));
    std::string why;
    if (!view_check(*in, 1, H, W, false, &why)) return fail(h, RRV_E_ARG, "add_view: in." + why);
    return add_frame(h, d_frame, true, fmt, (hipStream_t)hip_stream, H, W, in);
}

// sampled frames as YUV 4:2:0 (conv_first_k<IN_YUV_*>); the input matrix (the uint16 forms: and the depth) is read when the deferred encoding runs
static int add_from_yuv(rrv_handle h, const void* frame, bool device, int in_layout, hipStream_t stream, int H, int W) {
    if (!h || !frame) return RRV_E_ARG;
    InFmt in;
    if (parse_in_yuv(in_layout, &in) != DescErr::OK) return refuse_layout(h, "add_from_yuv: in_layout");
    return add_frame(h, frame, device, in, stream, H, W);
}
int rrv_add_from_yuv(rrv_handle h, const uint8_t* frame, int in_layout, int H, int W) { return add_from_yuv(h, frame, false, in_layout, nullptr, H, W); }
int rrv_add_from_yuv_device(rrv_handle h, const void* d_frame, int in_layout, int H, int W, void* hip_stream) {
    return add_from_yuv(h, d_frame, true, in_layout, (hipStream_t)hip_stream, H, W);
}

int rrv_compute(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    RCHK(flush_pending(h));
    if (h->patches.empty()) return fail(h, RRV_E_STATE, "compute: no frames added");
    int nprep = 0;
    for (StyleState& s : h->styles) nprep += s.prepared ? 1 : 0;
    if (!nprep) return fail(h, RRV_E_STATE, "compute: prepare_style has not been called");
    const int B = (int)h->patches.size(), hh = h->patch_h, ww = h->patch_w;
    // everything resident (Decoder.compute as written) if it fits the cap, else groups of G frames, one sync point at a time
    const bool streaming = prep_bytes(B, hh, ww, false) > h->ws_cap;
    int G = B;
    if (streaming) {
        G = 1;
        while (G < B && prep_bytes(G + 1, hh, ww, true) <= h->ws_cap) ++G;
    }
    h->last_groups = (B + G - 1) / G; h->last_group_size = G; h->last_ws_bytes = prep_bytes(G, hh, ww, streaming);
    prep_free(h);      // (a plan kept by rrv_debug_prep_stop; empty otherwise)
    const Seq q = base_seq(h);      // the preparation pass: F(2x2,3x3) on set 0, whatever ran before
    RCHK(prep_plan(h, q, G, hh, ww, streaming));
    int first = -1;
    auto body = [&]() -> int {
        const Tens& content = h->prep.content;
        for (int b = 0; b < B && !streaming; ++b)
            HIPCHK(hipMemcpyAsync(content.p + (size_t)b * content.img_floats(), h->patches[b], content.img_floats() * sizeof(float),
                                  hipMemcpyDeviceToDevice, q.stream));
        for (int s = 0; s < RRV_MAX_STYLES; ++s)
            if (h->styles[s].prepared) {
                if (first < 0) first = s;
                RCHK(streaming ? compute_style_streaming(h, q, s) : compute_style(h, q, s));
            }
        return RRV_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(q.stream);
    if (h->prep_stop < 0 || rc != RRV_OK) prep_free(h);      // several GB for a video's sampled frames
    if (rc != RRV_OK) return rc;
    if (h->debug) RCHK(debug_verify(h, "compute"));
    h->active_src = -1;
    if (!h->styles[first].computed) return RRV_OK;      // rrv_debug_prep_stop ended the pass early: no state to activate
    return activate_state(h, first);
}

int rrv_get_state(rrv_handle h, float* out, int n, int sid) {
    if (!h || !out || n != RRV_STATE_FLOATS || sid < 0 || sid >= RRV_MAX_STYLES) return RRV_E_ARG;
    StyleState& S = h->styles[sid];
    if (!S.blob || !S.computed) return fail(h, RRV_E_STATE, "get_state: state not computed for this style");
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    HIPCHK(hipMemcpy(out, S.blob, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return RRV_OK;
}

int rrv_set_state(rrv_handle h, const float* in, int n, int sid) {
    if (!h || !in || n != RRV_STATE_FLOATS || sid < 0 || sid >= RRV_MAX_STYLES) return RRV_E_ARG;
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    HIPCHK(hipSetDevice(h->dev));
    StyleState& S = h->styles[sid];
    if (!S.blob) RCHK(dalloc(h, base_seq(h), &S.blob, RRV_STATE_FLOATS));
    RCHK(sync_all(h));
    HIPCHK(hipMemcpy(S.blob, in, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    S.computed = true;
    RCHK(filter_conditioning(h, S));
    // the style set last is the one the plain transfer entries use next: re-fold now unless another style's folded
    // state is live (after a blend, -2, nothing of the old fold is worth keeping either)
    if (h->active_src == sid || h->active_src < 0) { h->active_src = -1; RCHK(activate_state(h, sid)); }
    return RRV_OK;
}

// ---- RCCL from the C ABI: the one collective of the path --------------------------------------------
// After compute() on the root rank every rank needs the 17 536-float state of each style; frames are independent from
// there on.  librccl is opened lazily (no link-time dependency: a single-GPU user never loads it).  The communicator is
// an ordinary ncclComm_t: pass one the application already has (e.g. built with MPI / torch), or build one with the
// three helpers below — the 128-byte unique id travels between processes by whatever means the caller has.
namespace {
struct Rccl {
    struct UId { char b[128]; };      // ncclUniqueId (passed by value)
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, UId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
typedef decltype(Rccl::CommInitRank) rccl_init_fn;
Rccl g_rccl;
std::mutex g_rccl_mu;
const char* rccl_load() {      // nullptr on success, else what went wrong
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return nullptr;
    void* l = nullptr;
    if (const char* e = getenv("RRV_RCCL_PATH")) l = dlopen(e, RTLD_NOW | RTLD_LOCAL);
    for (const char* n : {"librccl.so.1", "librccl.so"})
        if (!l) l = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);          // a copy the process already has (torch's)
    for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"})
        if (!l) l = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!l) return "librccl.so not found (set RRV_RCCL_PATH)";
    Rccl r;
    r.lib = l;
    r.GetUniqueId = (int (*)(void*))dlsym(l, "ncclGetUniqueId");
    r.CommInitRank = (rccl_init_fn)dlsym(l, "ncclCommInitRank");
    r.CommDestroy = (int (*)(void*))dlsym(l, "ncclCommDestroy");
    r.Broadcast = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(l, "ncclBroadcast");
    r.GetErrorString = (const char* (*)(int))dlsym(l, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.Broadcast) return "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclBroadcast";
    g_rccl = r;
    return nullptr;
}
}  // namespace

int rrv_comm_unique_id(char id[128]) {
    if (!id) return RRV_E_ARG;
    if (rccl_load()) return RRV_E_COMM;
    return g_rccl.GetUniqueId(id) == 0 ? RRV_OK : RRV_E_COMM;
}

int rrv_comm_init_rank(rrv_handle h, const char id[128], int nranks, int rank, void** comm) {
    if (!h || !id || !comm || nranks < 1 || rank < 0 || rank >= nranks) return RRV_E_ARG;
    if (const char* e = rccl_load()) return fail(h, RRV_E_COMM, e);
    HIPCHK(hipSetDevice(h->dev));
    Rccl::UId u;
    memcpy(u.b, id, 128);
    *comm = nullptr;
    const int rc = g_rccl.CommInitRank(comm, nranks, u, rank);
    if (rc != 0) return fail(h, RRV_E_COMM, std::string("ncclCommInitRank failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?"));
    return RRV_OK;
}

int rrv_comm_destroy(void* comm) {
    if (!comm) return RRV_E_ARG;
    if (rccl_load()) return RRV_E_COMM;
    return g_rccl.CommDestroy(comm) == 0 ? RRV_OK : RRV_E_COMM;
}

// ncclBroadcast of the style's state blob from `root` over `comm` on the handle's stream; every other rank then owns
// the state exactly as after rrv_set_state (filters folded locally).  One 70 KB message per style and video.
int rrv_broadcast_state(rrv_handle h, void* comm, int root, int my_rank, int sid) {
    if (!h || !comm || sid < 0 || sid >= RRV_MAX_STYLES || root < 0 || my_rank < 0) return RRV_E_ARG;
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    if (const char* e = rccl_load()) return fail(h, RRV_E_COMM, e);
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    StyleState& S = h->styles[sid];
    if (my_rank == root && (!S.blob || !S.computed)) return fail(h, RRV_E_STATE, "broadcast_state: the root has no computed state for this style");
    if (!S.blob) RCHK(dalloc(h, base_seq(h), &S.blob, RRV_STATE_FLOATS));
    const int rc = g_rccl.Broadcast(S.blob, S.blob, RRV_STATE_FLOATS, /* ncclFloat32 */ 7, root, comm, h->slots[0].stream);
    if (rc != 0) return fail(h, RRV_E_COMM, std::string("ncclBroadcast failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?"));
    HIPCHK(hipStreamSynchronize(h->slots[0].stream));
    if (my_rank != root) {
        S.computed = true;
        RCHK(filter_conditioning(h, S));
        if (h->active_src == sid || h->active_src < 0) { h->active_src = -1; RCHK(activate_state(h, sid)); }
    }
    return RRV_OK;
}

// ---- scaling (include/rerevst_hip.h "Scaling"): the axis tables of the resampler, on the host in double, and its launch
// One axis, S source and D destination samples: s = S / D, support = max(s, 1); output i has its centre at c = s (i + 0.5), first tap
// lo = max(int(c - support + 0.5), 0), n = min(int(c + support + 0.5), S) - lo taps, weight j = tri((lo + j - c + 0.5) / support) with
// tri(t) = max(0, 1 - |t|), divided by the row's sum; everything in double, each weight rounded once to float32.  s > 1: the antialiased
// triangle filter (PIL's, torch's interpolate(mode="bilinear", antialias=True)); s <= 1: half-pixel bilinear with edge clamp; S == D: {1, 0}.
static bool rs_ratio_ok(int S, int D) { return S >= 1 && D >= 1 && (int64_t)S <= 8 * (int64_t)D && (int64_t)D <= 8 * (int64_t)S; }
struct RsTaps { std::vector<int> first, count; std::vector<float> w; int taps = 0; };      // w: [D][RS_TAPS], zero beyond count; taps: the largest count
static RsTaps rs_build(int S, int D) {
    RsTaps t;
    t.first.resize(D); t.count.resize(D); t.w.assign((size_t)D * RS_TAPS, 0.f);
    const double s = (double)S / (double)D, support = s > 1.0 ? s : 1.0;
    for (int i = 0; i < D; ++i) {
        const double c = s * (i + 0.5);
        int lo = (int)(c - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(c + support + 0.5);
        if (hi > S) hi = S;
        int n = hi - lo;
        if (n > RS_TAPS) n = RS_TAPS;      // (cannot happen within the ratio limits: 2 * support + 1 samples at most, 16 at ratio 8)
        double wt[RS_TAPS], sum = 0.0;
        for (int j = 0; j < n; ++j) {
            const double u = std::fabs(((double)(lo + j) - c + 0.5) / support);
            wt[j] = u < 1.0 ? 1.0 - u : 0.0;
            sum += wt[j];
        }
        for (int j = 0; j < n; ++j) t.w[(size_t)i * RS_TAPS + j] = (float)(wt[j] / sum);
        t.first[i] = lo; t.count[i] = n;
        t.taps = std::max(t.taps, n);
    }
    return t;
}
int rrv_resample_taps(int S, int D, int* first, int* count, float* w, int cap) {
    if (!first || !count || !w || !rs_ratio_ok(S, D)) return RRV_E_ARG;
    const RsTaps t = rs_build(S, D);
    if (cap < t.taps) return RRV_E_ARG;
    for (int i = 0; i < D; ++i) {
        first[i] = t.first[i]; count[i] = t.count[i];
        for (int j = 0; j < cap; ++j) w[(size_t)i * cap + j] = j < RS_TAPS ? t.w[(size_t)i * RS_TAPS + j] : 0.f;
    }
    return RRV_OK;
}
// the tables of an axis pair in HBM: built once per (S, D) and handle, uploaded before the call's first launch (a synchronous copy)
static int rs_tables(rrv_handle h, int S, int D, const rrv_ctx::RsTab** out) {
    const auto key = std::make_pair(S, D);
    auto it = h->rs_tabs.find(key);
    if (it == h->rs_tabs.end()) {
        RsTaps t = rs_build(S, D);
        // The kernel's tables drop a trailing tap of weight 0 (the only place one occurs: |t| = 1 at a row's last tap, e.g. the 0 of an
        // identity row {1, 0}), so no product 0 x sample enters a sum and the kernel needs no per-tap test.  rrv_resample_taps reports it.
        for (int i = 0; i < D; ++i)
            while (t.count[i] > 1 && t.w[(size_t)i * RS_TAPS + t.count[i] - 1] == 0.f) --t.count[i];
        rrv_ctx::RsTab tab;
        const size_t ib = (size_t)D * sizeof(int), wb = (size_t)D * RS_TAPS * sizeof(float);
        RCHK(dmalloc(h, &tab.block, 2 * ib + wb));
        char* const base = (char*)tab.block;
        hipError_t e = hipMemcpy(base, t.first.data(), ib, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(base + ib, t.count.data(), ib, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(base + 2 * ib, t.w.data(), wb, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(tab.block); HIPCHK(e); }
        tab.axis = RsAxis{(const int*)base, (const int*)(base + ib), (const float*)(base + 2 * ib)};
        for (int i0 = 0; i0 < D; i0 += RS_TH) {
            const int i1 = std::min(i0 + RS_TH, D) - 1;
            tab.span = std::max(tab.span, t.first[i1] + t.count[i1] - t.first[i0]);
        }
        it = h->rs_tabs.emplace(key, tab).first;
    }
    *out = &it->second;
    return RRV_OK;
}
// both axes' tables of a request.  A caller that keeps changing sizes starts over at 64 tables, once nothing in flight reads the old
// ones and before either pointer is handed out (a map's entries stay where they are while others are added).
static int rs_pair(rrv_handle h, int SH, int SW, int H, int W, const rrv_ctx::RsTab** ty, const rrv_ctx::RsTab** tx) {
    const bool have = h->rs_tabs.count(std::make_pair(SH, H)) && h->rs_tabs.count(std::make_pair(SW, W));
    if (!have && h->rs_tabs.size() >= 64) {
        RCHK(sync_all(h));
        HIPCHK(hipDeviceSynchronize());      // (rrv_resample_view_device queues on the caller's stream)
        for (auto& kv : h->rs_tabs) (void)hipFree(kv.second.block);
        h->rs_tabs.clear();
    }
    RCHK(rs_tables(h, SH, H, ty));
    RCHK(rs_tables(h, SW, W, tx));
    // (cannot happen within the ratio limits; judged here, where every request passes before its first launch)
    if ((*ty)->span > RS_ROWS_MAX) return fail(h, RRV_E_ARG, "resample: the vertical taps of a tile span more rows than the kernel stages");
    return RRV_OK;
}
// What a stage's launch over tiles of RS_TH x RS_TW pixels of an H x W destination starts from: both axes' tables (they exist already or
// are built here), the tiles per frame, and the largest span of a tile's taps on either axis (rows: what a tile stages in LDS).
struct RsGrid { RsAxis ay, ax; int tiles_x, tiles_y, rows, cols; };
static int rs_grid(rrv_handle h, int SH, int SW, int H, int W, RsGrid* g) {
    const rrv_ctx::RsTab *ty, *tx;
    RCHK(rs_pair(h, SH, SW, H, W, &ty, &tx));
    *g = RsGrid{ty->axis, tx->axis, (W + RS_TW - 1) / RS_TW, (H + RS_TH - 1) / RS_TH, ty->span, tx->span};
    return RRV_OK;
}
// everything a scaled request allocates, before its first launch: both axes' tables and room for `frames` working frames in the slot's buffer
static int rs_reserve(rrv_handle h, int slot, int frames, int SH, int SW, int H, int W) {
    const rrv_ctx::RsTab *ty, *tx;
    RCHK(rs_pair(h, SH, SW, H, W, &ty, &tx));
    rrv_ctx::Slot& sl = h->slots[slot];
    return ensure_dev(h, sl.rs_buf, sl.rs_cap, (size_t)frames * H * W * 3);
}
static int check_deliver(rrv_handle h, const char* who, int H, int W, int DH, int DW) {      // H x W: the stylized working frame
    if (DH < 1 || DW < 1) return fail(h, RRV_E_ARG, std::string(who) + ": DH, DW must be at least 1");
    if (H < 1 || W < 1) return fail(h, RRV_E_ARG, std::string(who) + ": the working frame must be at least 1 x 1 pixels");
    if (!rs_ratio_ok(H, DH)) return fail(h, RRV_E_ARG, std::string(who) + ": DH / the working frame's height must be within 1/8 .. 8");
    if (!rs_ratio_ok(W, DW)) return fail(h, RRV_E_ARG, std::string(who) + ": DW / the working frame's width must be within 1/8 .. 8");
    return RRV_OK;
}
static int check_scale(rrv_handle h, const char* who, int SH, int SW, int H, int W) {
    if (SH < 1 || SW < 1) return fail(h, RRV_E_ARG, std::string(who) + ": SH, SW must be at least 1");
    if (H < 1 || W < 1) return fail(h, RRV_E_ARG, std::string(who) + ": H, W must be at least 1");
    if (!rs_ratio_ok(SH, H)) return fail(h, RRV_E_ARG, std::string(who) + ": SH / H must be within 1/8 .. 8");
    if (!rs_ratio_ok(SW, W)) return fail(h, RRV_E_ARG, std::string(who) + ": SW / W must be within 1/8 .. 8");
    return RRV_OK;
}
// B frames of SH x SW in the format `in` through `vi` -> contiguous [B][H][W][3] float32 BGR PIXEL at d_out, queued on q.stream.  The tables
// exist already or are built here (reserve_stages has run for the entries that promise no allocation between launches).
static int resample_launch(rrv_handle h, const Seq& q, const void* d_in, InFmt in, const ImgView& vi, int B, int SH, int SW, int H, int W, float* d_out) {
    RsGrid g;
    RCHK(rs_grid(h, SH, SW, H, W, &g));
    ResampleP p{};
    p.img = d_in; p.v = vi; p.SH = SH; p.SW = SW; p.H = H; p.W = W; p.B = B; p.out = d_out;
    p.ay = g.ay; p.ax = g.ax; p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y; p.rows = g.rows;
    p.space = in.space;
    if (in_yuv(in.form)) {
        const YuvLaunch y = yuv_launch_params(h->yuv_in, true, in_yuv16(in.form), in.form == IN_YUV_P016);
        memcpy(p.yuv_n, y.m, sizeof p.yuv_n); p.yuv_shift = y.shift;
        p.csx = chroma_sx(in.cs); p.csy = chroma_sy(in.cs);
    }
    int e = 0;
    // for the profile log: bytes from the shapes; operations two per tap, channel and pass, a row's taps taken as span / RS_TH
    const double src_bytes = (in_yuv(in.form) ? yuv_samples_per_pixel(in.cs) : 3.0) * in_elem(in.form) * SH * SW;
    RCHK(launch(h, q, "resample", 2.0 * B * 3 * ((double)g.cols / RS_TH * SH * W + (double)g.rows / RS_TH * H * W), (src_bytes + 12.0 * H * W) * B, [&] {
        e = rrv_scale_launch(&p, in.form, q.stream);
    }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("resample: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}

// ---- output size (include/rerevst_hip.h "Scaling, output size"): the delivery stage behind the last kernel
// the deliver_k instantiation that writes `f`
static int deliver_form(OutFmt f) { return f.yuv ? (yuv16_layout(f.yuv) ? DL_YUV16 : DL_YUV8) : f.u8 ? (f.chw ? DL_U8_CHW : DL_U8_HWC) : (f.chw ? DL_F32_CHW : DL_F32_HWC); }
// B contiguous float32 [H][W][3] BGR PIXEL frames at d_in -> DH x DW frames in the format `fmt` through `vo` at d_out, queued on q.stream.  The
// tables exist already or are built here (reserve_stages has run for the entries that promise no allocation between launches).
static int deliver_launch(rrv_handle h, const Seq& q, const float* d_in, int B, int H, int W, int DH, int DW, void* d_out, OutFmt fmt, const ImgView& vo) {
    RsGrid g;
    RCHK(rs_grid(h, H, W, DH, DW, &g));
    DeliverP p{};
    p.in = d_in; p.H = H; p.W = W; p.B = B; p.DH = DH; p.DW = DW; p.out = d_out; p.v = vo;
    p.ay = g.ay; p.ax = g.ax; p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y; p.rows = g.rows;
    p.space = fmt.space;
    if (fmt.yuv) {
        const YuvLaunch y = yuv_launch_params(h->yuv_out, false, yuv16_layout(fmt.yuv), fmt.yuv == RRV_LAY_P016);
        memcpy(p.yuv_m, y.m, sizeof p.yuv_m); p.yuv_hi = y.hi; p.yuv_shift = y.shift;
        p.nv12 = fmt.yuv == RRV_LAY_NV12 || fmt.yuv == RRV_LAY_P016;
        p.csx = chroma_sx(fmt.cs); p.csy = chroma_sy(fmt.cs);
    }
    int e = 0;
    // for the profile log: bytes from the shapes (12 per working pixel read, the delivered frame written); operations as the resampler's
    const double out_bytes = (fmt.yuv ? yuv_samples_per_pixel(fmt.cs) * yuv_sample_bytes(fmt) : 3.0 * out_elem(fmt)) * DH * DW;
    RCHK(launch(h, q, "deliver", 2.0 * B * 3 * ((double)g.cols / RS_TH * H * DW + (double)g.rows / RS_TH * DH * DW), (12.0 * H * W + out_bytes) * B, [&] {
        e = rrv_deliver_launch(&p, deliver_form(fmt), q.stream);
    }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("deliver: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}

// ---- guided delivery (include/rerevst_hip.h "Guided delivery"): the stylized working frame upsampled along the source's edges
// H x W: the stylized working frame.  Radius, eps and the sizes, judged before any GPU work.
static int check_guided(rrv_handle h, const char* who, int H, int W, int DH, int DW, int r, float eps) {
    if (r < 1 || r > GF_R_MAX) return fail(h, RRV_E_ARG, std::string(who) + ": r must be in 1..16");
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(h, RRV_E_ARG, std::string(who) + ": eps must be a positive number");
    if (H < 1 || W < 1) return fail(h, RRV_E_ARG, std::string(who) + ": the working frame must be at least 1 x 1 pixels");
    if (DH < H || (int64_t)DH > 8 * (int64_t)H) return fail(h, RRV_E_ARG, std::string(who) + ": DH / the working frame's height must be within 1 .. 8");
    if (DW < W || (int64_t)DW > 8 * (int64_t)W) return fail(h, RRV_E_ARG, std::string(who) + ": DW / the working frame's width must be within 1 .. 8");
    return RRV_OK;
}
// the tile guided_launch gives gf_apply_k for these sizes and the dynamic LDS of both kernels; the sizes and the radius are check_guided's
int rrv_guided_tile(int H, int W, int DH, int DW, int r, int* tw, int* sy, int* sx, int* apply_lds_bytes, int* coeff_lds_bytes) {
    if (!tw || !sy || !sx || !apply_lds_bytes || !coeff_lds_bytes) return RRV_E_ARG;
    if (r < 1 || r > GF_R_MAX || H < 1 || W < 1) return RRV_E_ARG;
    if (DH < H || (int64_t)DH > 8 * (int64_t)H || DW < W || (int64_t)DW > 8 * (int64_t)W) return RRV_E_ARG;
    GuidedP p{};
    p.H = H; p.W = W; p.DH = DH; p.DW = DW; p.r = r;
    if (!guided_tile(&p)) return RRV_E_ARG;      // (cannot happen within the radius limit)
    *tw = p.tw; *sy = p.sy; *sx = p.sx;
    *apply_lds_bytes = (int)guided_apply_lds_bytes(r, p.sy, p.sx);
    *coeff_lds_bytes = (int)guided_coeff_lds_bytes(r);
    return RRV_OK;
}
// the tables the stage and the equal-size passes around it read: (H, W) -> (DH, DW), and the identity of the delivered size
static int gd_tables(rrv_handle h, int H, int W, int DH, int DW) {
    const rrv_ctx::RsTab *ty, *tx;
    RCHK(rs_pair(h, H, W, DH, DW, &ty, &tx));
    return rs_pair(h, DH, DW, DH, DW, &ty, &tx);
}
// Everything the stages of request `x` allocate on `slot` for `frames` frames at a time, before the request's first launch.  Scaled: both
// axes' tables and the slot's buffer of working frames.  Then guided: its tables, the stylized working frames and the stage's three buffers;
// or delivering: the tables and the stylized working frames.
static int reserve_stages(rrv_handle h, int slot, int frames, const Xfer& x) {
    if (x.scaled()) RCHK(rs_reserve(h, slot, frames, x.SH, x.SW, x.H, x.W));
    if (x.pic) {      // the equal-size tables of the whole frame (the resampler in, the delivery stage out) and the canvas
        const rrv_ctx::RsTab *fy, *fx;
        RCHK(rs_pair(h, x.FH, x.FW, x.FH, x.FW, &fy, &fx));
        RCHK(ensure_dev(h, h->slots[slot].pc_canvas, h->slots[slot].pc_canvas_cap, (size_t)frames * x.FH * x.FW * 3));
    }
    if (!x.staged()) return RRV_OK;
    const int H = x.WH(), W = x.WW();
    const rrv_ctx::RsTab *ty, *tx;
    if (x.guided()) RCHK(gd_tables(h, H, W, x.DH, x.DW));
    else if (x.delivering()) RCHK(rs_pair(h, H, W, x.DH, x.DW, &ty, &tx));
    rrv_ctx::Slot& sl = h->slots[slot];
    RCHK(ensure_dev(h, sl.dl_buf, sl.dl_cap, (size_t)frames * H * W * 3));
    if (x.comp) {      // the equal-size tables of the delivered frame, S where the source is resampled for it, P where the working frame is not it
        const int OH = x.OH(), OW = x.OW();
        RCHK(rs_pair(h, OH, OW, OH, OW, &ty, &tx));
        if (!x.guided() && !x.src_is_rs()) {
            RCHK(rs_pair(h, x.IH(), x.IW(), OH, OW, &ty, &tx));
            RCHK(ensure_dev(h, sl.gd_xhi, sl.gd_xhi_cap, (size_t)frames * OH * OW * 3));
        }
        if (!x.guided() && x.delivering()) RCHK(ensure_dev(h, sl.gd_q, sl.gd_q_cap, (size_t)frames * OH * OW * 3));
    }
    if (x.jp) {      // the blocks and the interval index; the float32 frame at the delivered size where nothing else has made one
        RCHK(ensure_dev(h, sl.jp_coef, sl.jp_coef_cap, (size_t)frames * x.jp->blocks * 64));
        RCHK(ensure_dev(h, sl.jp_idx, sl.jp_idx_cap, 2 * (size_t)frames * x.jp->n_int));
        if (!x.guided() && !x.comp && x.delivering()) RCHK(ensure_dev(h, sl.gd_q, sl.gd_q_cap, (size_t)frames * x.OH() * x.OW() * 3));
    }
    if (!x.guided()) return RRV_OK;
    RCHK(ensure_dev(h, sl.gd_xhi, sl.gd_xhi_cap, (size_t)frames * x.DH * x.DW * 3));
    RCHK(ensure_dev(h, sl.gd_ab, sl.gd_ab_cap, (size_t)frames * H * W * 6));
    return ensure_dev(h, sl.gd_q, sl.gd_q_cap, (size_t)frames * x.DH * x.DW * 3);
}
// B frames: P, x_lo [H][W][3] and x_hi [DH][DW][3] -> q [DH][DW][3], all contiguous float32 BGR PIXEL, through the planes `ab` ([B][6][H][W]);
// queued on q.stream.  The tables exist already or are built here.
static int guided_launch(rrv_handle h, const Seq& q, const float* P, const float* x_lo, const float* x_hi, int B, int H, int W, int DH, int DW, int r,
                         float eps, float* ab, float* out) {
    RsGrid g;      // (its tiles are guided_tile's: only the axes are taken)
    RCHK(rs_grid(h, H, W, DH, DW, &g));
    GuidedP p{};
    p.P = P; p.xlo = x_lo; p.xhi = x_hi; p.ab = ab; p.q = out;
    p.H = H; p.W = W; p.B = B; p.DH = DH; p.DW = DW; p.r = r; p.e = eps * 65025.0f;
    p.ay = g.ay; p.ax = g.ax;
    if (!guided_tile(&p)) return fail(h, RRV_E_ARG, "guided: no tile of the apply kernel fits the LDS");      // (cannot happen within the radius limit)
    int e = 0;
    // for the profile log: bytes from the shapes (P, X_lo read, the planes written and read with their halo counted once, X_hi read, Q written);
    // operations two per window term, moment and pass, and two per tap and plane
    const double win = 2.0 * r + 1.0;
    RCHK(launch(h, q, "guided", (2.0 * 2 * 8 * win * H * W + 2.0 * 2 * 6 * win * H * W + 2.0 * 6 * 4 * DH * DW) * B,
                ((12.0 + 12.0 + 24.0 + 24.0) * H * W + 24.0 * DH * DW) * B, [&] { e = rrv_guided_launch(&p, q.stream); }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("guided: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}

// ---- compositing (include/rerevst_hip.h "Compositing"): the delivered float32 frame mixed with the source at the delivered size
int rrv_composite_grid(int B, int DH, int DW, unsigned* grid, int* pixels_per_pass) {
    if (!grid || !pixels_per_pass || B < 1 || DH < 1 || DW < 1) return RRV_E_ARG;
    *grid = compose_grid((size_t)B * (size_t)DH * (size_t)DW);
    *pixels_per_pass = (int)(*grid * 1024u);
    return RRV_OK;
}
// A request as an entry got it -> the fields of `x`, judged before any GPU work; B: the frames `c->strength` holds.  A request that composites
// nothing (null; no matte, every strength 1, keep none) leaves x as it is: the call is then the one without a request.
static int set_composite(rrv_handle h, const char* who, const rrv_composite* c, int B, Xfer* x) {
    if (!c) return RRV_OK;
    const std::string w = std::string(who) + ": ";
    if (c->keep != RRV_KEEP_NONE && c->keep != RRV_KEEP_COLOUR && c->keep != RRV_KEEP_LUMA) return fail(h, RRV_E_ARG, w + "keep must be one of RRV_KEEP_NONE, RRV_KEEP_COLOUR, RRV_KEEP_LUMA");
    if (B < 1) return fail(h, RRV_E_ARG, w + "batch must be at least 1");
    bool ones = true;
    if (c->strength)
        for (int b = 0; b < B; ++b) {
            const float v = c->strength[b];
            if (!(v >= 0.f && v <= 1.f)) return fail(h, RRV_E_ARG, w + "strength must lie in 0..1 for every frame");      // (NaN fails both comparisons)
            ones = ones && v == 1.f;
        }
    if (c->matte) {
        if (c->matte_dtype != RRV_DT_F32 && c->matte_dtype != RRV_DT_U8) return fail(h, RRV_E_ARG, w + "matte_dtype must be RRV_DT_F32 or RRV_DT_U8");
        if (c->matte_frames != 1 && c->matte_frames != B) return fail(h, RRV_E_ARG, w + "matte_frames must be 1 or B");
    }
    if (!c->matte && ones && c->keep == RRV_KEEP_NONE) return RRV_OK;
    x->comp = true;
    x->cstr = c->strength; x->cmatte = c->matte; x->cm_dt = c->matte_dtype; x->cm_frames = c->matte ? c->matte_frames : 0; x->ckeep = c->keep;
    return RRV_OK;
}
// B frames P and S -> out (may be P), all contiguous [OH][OW][3] float32 BGR PIXEL; str: B strengths in host memory (null: 1); queued on q.stream
static int composite_launch(rrv_handle h, const Seq& q, const float* P, const float* S, int B, int OH, int OW, const float* str, const void* matte, int matte_dt,
                            int matte_frames, int keep, float* out) {
    ComposeP p{};
    p.P = P; p.S = S; p.matte = matte; p.out = out;
    p.frame_px = (size_t)OH * (size_t)OW; p.B = B; p.matte_frames = matte_frames; p.keep = keep;
    for (int b = 0; b < B; ++b) p.strength[b] = str ? str[b] : 1.0f;
    const int form = !matte ? CM_NONE : matte_dt == RRV_DT_U8 ? CM_U8 : CM_F32;
    int e = 0;
    // for the profile log: bytes from the shapes (P and S read, the result written, the matte read once per frame); two products and a sum per value, the lumas
    const double px = (double)B * OH * OW;
    RCHK(launch(h, q, "composite", (9.0 + (keep ? 14.0 : 0.0) + (matte ? 2.0 : 1.0)) * px, (36.0 + (form == CM_F32 ? 4.0 : form == CM_U8 ? 1.0 : 0.0)) * px, [&] {
        e = rrv_compose_launch(&p, form, q.stream);
    }, -1.0, compose_grid((size_t)B * p.frame_px)));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("composite: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}

// ---- JPEG output (include/rerevst_hip.h "JPEG output"): the delivered float32 frame encoded in place of the output form
// The request and the sizes of a JPEG entry -> the kernels' parameters, judged before any GPU work.  entropy: the call writes streams (cap counts).
static int set_jpeg(rrv_handle h, const char* who, const rrv_jpeg* j, int B, int H, int W, bool entropy, size_t cap, JpegP* p) {
    const std::string w = std::string(who) + ": ";
    if (!j) return fail(h, RRV_E_ARG, w + "null rrv_jpeg");
    if (B < 1 || B > JP_B_MAX) return fail(h, RRV_E_ARG, w + "batch must be in 1..64");
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return fail(h, RRV_E_ARG, w + "H, W must be in 1..65535");
    if (j->quality < 1 || j->quality > 100) return fail(h, RRV_E_ARG, w + "quality must be in 1..100");
    if (!jpeg_chroma_ok(j->chroma)) return fail(h, RRV_E_ARG, w + "chroma must be 420, 422 or 444");
    if (j->restart < 0 || j->restart > 65535) return fail(h, RRV_E_ARG, w + "restart must be in 0..65535 (0: one MCU row per interval)");
    if (!jpeg_fill(p, H, W, j->chroma, j->quality, j->restart)) return fail(h, RRV_E_ARG, w + "quality, chroma or restart out of range");
    p->B = B; p->cap = cap;
    if (entropy) {
        if (jpeg_bound(*p) > (size_t)0x7fffffff) return fail(h, RRV_E_ARG, w + "the frame is too large: rrv_jpeg_bound must stay below 2^31 bytes");
        if (cap < (size_t)p->header_len + 2) return fail(h, RRV_E_ARG, w + "cap must hold at least the header and EOI (rrv_jpeg_plan's header bytes + 2)");
    }
    return RRV_OK;
}
static int jpeg_blocks_launch(rrv_handle h, const Seq& q, const JpegP& p) {
    int e = 0;
    // for the profile log: 12 bytes per pixel read, the blocks written; the two 8-point passes at 29 operations each per 8 samples
    RCHK(launch(h, q, "jpeg_blocks", 2.0 * 29.0 / 8.0 * 64.0 * p.blocks * p.B, (12.0 * p.H * p.W + 128.0 * p.blocks) * p.B, [&] { e = rrv_jpeg_blocks_launch(&p, q.stream); }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("jpeg_blocks: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}
static int jpeg_entropy_launch(rrv_handle h, const Seq& q, const JpegP& p) {
    int e = 0;
    // for the profile log: the blocks read twice by each of the two passes; the bytes written are device results and not counted
    RCHK(launch(h, q, "jpeg_entropy", 0.0, 4.0 * 128.0 * p.blocks * p.B, [&] { e = rrv_jpeg_entropy_launch(&p, q.stream); }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("jpeg_entropy: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}
// The alternating device entries: consecutive calls cycle over n_slots (stream, workspace) pairs so that the tail / store
// burst of one batch's kernels overlaps the next batch's kernels (frames are independent).  Profiled launches stay on slot 0.
static int next_device_slot(rrv_handle h) {
    const int slot = (h->n_slots > 1 && !h->profiling) ? h->next_slot : 0;
    h->next_slot = (slot + 1) % h->n_slots;
    return slot;
}

// Every argument and state check of a transfer, once per API call, before anything is staged or launched.  host: the pipeline cuts
// sub-batches itself, so any B >= 1 is served; the device and image entries take 1..64 frames.  state_first: see below.
static int check_xfer(rrv_handle h, const Xfer& x, bool host = false, bool state_first = false) {
    const bool blend = x.model == Model::BLEND, mask = x.model == Model::MASK;
    if (x.B < 1 || (!host && x.B > 64)) return fail(h, RRV_E_ARG, "transfer: batch must be in 1..64");
    if (x.pad && (x.H < 1 || x.W < 1)) return fail(h, RRV_E_ARG, "transfer: frames must be at least 1 x 1 pixels");
    RCHK(check_frame(h, x.KH(), x.KW(), "transfer"));      // the geometry the kernels run, refused before any staging is sized for it
    if (x.scaled()) RCHK(check_scale(h, "transfer", x.SH, x.SW, x.H, x.W));
    if (x.DH != 0 || x.DW != 0) RCHK(check_deliver(h, "transfer", x.WH(), x.WW(), x.DH, x.DW));
    if (x.guided()) {      // the guide is the call's own source: it has the delivered size, and the frame the model delivers the working size
        RCHK(check_guided(h, "transfer_guided", x.WH(), x.WW(), x.DH, x.DW, x.gr, x.geps));
        if (x.model != Model::GLOBAL && x.model != Model::FRAME) return fail(h, RRV_E_ARG, "transfer_guided: blended and masked guided delivery are not offered");
        if (x.DH != x.IH() || x.DW != x.IW()) return fail(h, RRV_E_ARG, "transfer_guided: DH x DW must be the size of the frames as passed (SH x SW; H x W with SH = SW = 0)");
        if (x.WH() != x.H || x.WW() != x.W) return fail(h, RRV_E_ARG, "transfer_guided: H and W must be multiples of 8 without RRV_TF_PAD_CROP (the stylized working frame is then H x W)");
    }
    if (x.comp) {      // (the request itself: set_composite)
        if (x.model != Model::GLOBAL && x.model != Model::FRAME) return fail(h, RRV_E_ARG, "transfer_composite: blended and masked compositing are not offered");
        if (x.WH() != x.H || x.WW() != x.W) return fail(h, RRV_E_ARG, "transfer_composite: H and W must be multiples of 8 without RRV_TF_PAD_CROP (the stylized working frame is then H x W)");
        if (!x.guided() && !x.src_is_rs()) RCHK(check_scale(h, "transfer_composite: the source against the delivered frame", x.IH(), x.IW(), x.OH(), x.OW()));
    }
    if ((blend || mask) && (x.ns < 1 || x.ns > RRV_MAX_STYLES)) return fail(h, RRV_E_ARG, "transfer: n_styles must be in 1..RRV_MAX_STYLES");
    if (blend && !x.wts) return fail(h, RRV_E_ARG, "transfer: null style weights");
    if (mask && !x.mask) return fail(h, RRV_E_ARG, "transfer: null mask");
    if (mask && x.mask_images != 1 && x.mask_images != x.B) return fail(h, RRV_E_ARG, "transfer: mask_images must be 1 or B");
    // A handle without weights has no state either.  Every entry reports the weights, except rrv_transfer_mask_batch and the one-frame
    // blended entries (rrv_transfer_blend[_device][_u8]: state_first), which have always answered RRV_E_STATE: kept as it is.
    if (!h->finalized && !(mask && host) && !state_first) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    if (x.model == Model::FRAME && !h->styles[0].prepared) return fail(h, RRV_E_STATE, "prepare_style has not been called");
    for (int s = 0; s < x.ns; ++s)
        if (!h->styles[s].computed) return fail(h, RRV_E_STATE, "transfer: state not computed for every style");
    if (x.model == Model::GLOBAL && h->active_src < 0) {      // what ensure_active would find nothing to activate for
        bool any = false;
        for (const StyleState& S : h->styles) any = any || S.computed;
        if (!any) return fail(h, RRV_E_STATE, "state not computed: call compute() (or set_state) before transfer()");
    }
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    return RRV_OK;
}

// Runs a checked request from d_in to d_out on `slot` (the grouped models: 0 or 1, the slots that own sixteen state sets each).
// GLOBAL is one launch sequence for all B frames; the others walk launch sequences of up to MS_GROUP_MAX frames:
//   FRAME  frame_mode_device: every frame with its own statistics, written to the slot's state sets
//   BLEND  the group's state sets := sum_s w[b][s] x state_s with their KernelFilters folded (blend_sets: host weights in the kernel
//          argument, a group's rows at a time; only w_dev weights are read from HBM), then encoder AND decoder with per-image state
//          (transfer_device, state_images) -- or, with x.feats, the decoder alone on the group's cached features.  One frame is a group
//          of one on the shared-state kernels: with a fixed kernel mode a frame's arithmetic does not depend on its group, bit for bit.
//   MASK   mask_mode_device; it touches no state set
// hk (host_pipeline, a request of one launch sequence): handed to transfer_device
static int run_xfer(rrv_handle h, int slot, const void* d_in, void* d_out, const Xfer& x, const SeqHook* hk = nullptr) {
    // What is in flight and reads the state sets this request rewrites drains first: a global entry's work reads state set 0, which
    // slot 0's sets include (frame-mode and blended launches write a slot's sets on that slot's own stream, in order)
    switch (x.model) {
    case Model::GLOBAL: RCHK(ensure_active(h)); break;
    case Model::FRAME:  if (h->active_src != -1) RCHK(sync_all(h)); break;
    case Model::BLEND:  if (h->active_src >= 0) RCHK(sync_all(h)); break;
    case Model::MASK:   break;
    }
    // Against the caller's stream: what it holds so far (the frames, device-resident weights, the masks) precedes the first launch,
    // and it waits for the last one.  transfer_device brackets its own launches, which is all the global model needs.
    // A scaled request resamples each launch group's frames in front of its model (the resampler reads the caller's frames, so it is
    // bracketed here for every model); what the request allocates for that exists before the first launch.
    const bool scaled = x.scaled();
    // A delivering request runs each launch group's model into the slot's buffer of working frames (float32 HWC BGR PIXEL) and the delivery
    // stage from there to the caller's frames, on the same sequence; the bracket covers it, so the caller's stream waits for deliver_k.
    // A guided request does the same and then runs the source through the resampler at its own size (X_hi), the guided stage from the
    // working frames, the working-size source (the scaled request's resampled frames, else X_hi itself) and X_hi to Q, and the delivery
    // stage at equal size from Q to the caller's frames.
    const bool delivering = x.delivering(), guided = x.guided(), staged = x.staged();
    const int group_frames = x.model == Model::GLOBAL ? x.B : std::min(x.B, (int)rrv_ctx::MS_GROUP_MAX);
    RCHK(reserve_stages(h, slot, group_frames, x));
    rrv_ctx::Slot& sl = h->slots[slot];
    const CallerOrder caller = x.order(h);
    const bool pic = x.pic;
    const bool bracket = caller.sync && (x.model != Model::GLOBAL || scaled || staged || pic);
    if (bracket) {
        HIPCHK(hipEventRecord(sl.ev, caller.stream));
        HIPCHK(hipStreamWaitEvent(sl.stream, sl.ev, 0));
    }
    const int KH = x.KH(), KW = x.KW(), G = x.model == Model::GLOBAL ? x.B : (int)rrv_ctx::MS_GROUP_MAX;
    const ImgView vi = x.in_view(), vo = x.out_view();      // the one addressing path: contiguous frames are a view like any other
    const size_t fb = (size_t)vi.fs * in_elem(x.in.form), fo = (size_t)vo.fs * out_view_elem(x.fmt);      // bytes from a frame to the next
    const PadCrop crop = x.pad_crop();
    const ImgView vw = contiguous_view(VL_HWC, x.H, x.W);      // a scaled request's working frames: float32 HWC BGR PIXEL in the slot's buffer
    const ImgView vd = contiguous_view(VL_HWC, x.WH(), x.WW());    // a delivering request's stylized working frames, the same form in the slot's other buffer
    // a picture request: the whole source frames, the canvas of a group, and the window of the canvas as an output view with the canvas's pitch
    const ImgView vf = pic ? img_view(*x.vfull) : vi;
    const ImgView vc = contiguous_view(VL_HWC, x.FH, x.FW);
    const ImgView vcw{vc.fs, {((int64_t)x.py0 * x.FW + x.px0) * 3, 0, 0}, {vc.pitch[0], 0, 0}};
    const FrameIO io{scaled ? InFmt{IN_F32_HWC, SP_PIXEL} : x.in, staged || pic ? OUT_F32 : x.fmt, x.pad ? &crop : nullptr, scaled ? &vw : &vi,
                     staged ? &vd : pic ? &vcw : &vo, caller};
    for (int b0 = 0; b0 < x.B; b0 += G) {
        const int cnt = x.B - b0 < G ? x.B - b0 : G;
        const uint8_t* in = (const uint8_t*)d_in + (size_t)b0 * fb;
        void* const dst = (char*)d_out + (size_t)b0 * fo;      // the group's frames as the caller gets them
        void* const out = staged ? (void*)sl.dl_buf : pic ? (void*)sl.pc_canvas : dst;
        const uint8_t* const src = in;                         // the group's frames as the caller passed them
        // the group's sequence: GLOBAL and MASK read no set of the slot's own, FRAME writes and BLEND blends into them (image g: set g of the slot's);
        // GLOBAL and BLEND are the per-frame path (transfer_device), where F(4x4,3x3) may run
        Seq q = slot_seq(h, slot, x.model == Model::FRAME || x.model == Model::BLEND);
        q.f43 = x.model == Model::GLOBAL || x.model == Model::BLEND;
        // a picture request: the canvas first, every source pixel as the first kernel's float32 value; the window of it is overwritten below
        if (pic) RCHK(resample_launch(h, q, src, x.in, vf, cnt, x.FH, x.FW, x.FH, x.FW, sl.pc_canvas));
        if (scaled) {
            RCHK(resample_launch(h, q, in, x.in, vi, cnt, x.SH, x.SW, x.H, x.W, sl.rs_buf));
            in = (const uint8_t*)sl.rs_buf;
        }
        switch (x.model) {
        case Model::GLOBAL:
            RCHK(transfer_device(h, q, in, cnt, KH, KW, out, io, nullptr, hk));
            break;
        case Model::FRAME:
            RCHK(frame_mode_device(h, q, in, cnt, KH, KW, out, io));
            break;
        case Model::MASK:
            RCHK(mask_mode_device(h, q, in, cnt, KH, KW, x.mask + (x.mask_images == 1 ? 0 : (size_t)b0 * x.mask_floats()), x.ns, x.mask_images == 1, out,
                                  io));
            break;
        case Model::BLEND:
            RCHK(blend_sets(h, q, x.wts + (size_t)b0 * x.ns, x.w_dev, x.ns, cnt));      // (the sets count as blends from here on: active_src -2)
            q.state_images = cnt > 1 ? cnt : 0;      // one frame: its state set is simply the sequence's (shared-state kernels)
            RCHK(transfer_device(h, q, in, cnt, KH, KW, out, io, x.feats ? x.feats + b0 : nullptr, hk));      // (a host sub-batch is one group: the hook's sequence)
            sl.set_images = cnt;
            break;
        }
        // What leaves through the delivery stage: the staged working frames (PH x PW = the working size), or the guided stage's Q at the
        // delivered size.  A compositing request brings P to the delivered size first -- Q, or the delivery stage's float32 PIXEL result in
        // Q's buffer, or the working frame itself -- and mixes it in place with S: the guided stage's X_hi, the scaled request's working
        // input when that frame is the one delivered, else the source through the resampler into X_hi's buffer.
        if (!staged && !pic) continue;
        if (!staged) {      // the last kernel has written the window of the canvas
            RCHK(deliver_launch(h, q, sl.pc_canvas, cnt, x.FH, x.FW, x.FH, x.FW, dst, x.fmt, vo));
            continue;
        }
        const int OH = x.OH(), OW = x.OW();
        float* P = sl.dl_buf;
        int PH = x.WH(), PW = x.WW();
        if (guided) {
            RCHK(resample_launch(h, q, src, x.in, vi, cnt, x.DH, x.DW, x.DH, x.DW, sl.gd_xhi));
            RCHK(guided_launch(h, q, sl.dl_buf, scaled ? sl.rs_buf : sl.gd_xhi, sl.gd_xhi, cnt, x.WH(), x.WW(), x.DH, x.DW, x.gr, x.geps, sl.gd_ab, sl.gd_q));
            P = sl.gd_q; PH = OH; PW = OW;
        }
        if (x.comp) {
            const float* S = sl.gd_xhi;
            if (!guided && delivering) {
                RCHK(deliver_launch(h, q, sl.dl_buf, cnt, PH, PW, OH, OW, sl.gd_q, OUT_F32, contiguous_view(VL_HWC, OH, OW)));
                P = sl.gd_q; PH = OH; PW = OW;
            }
            if (!guided && x.src_is_rs()) S = sl.rs_buf;
            else if (!guided) RCHK(resample_launch(h, q, src, x.in, vi, cnt, x.IH(), x.IW(), OH, OW, sl.gd_xhi));
            const void* const matte = x.cmatte && x.cm_frames != 1 ? (const char*)x.cmatte + (size_t)b0 * x.matte_bytes() : x.cmatte;
            RCHK(composite_launch(h, q, P, S, cnt, OH, OW, x.cstr ? x.cstr + b0 : nullptr, matte, x.cm_dt, x.cm_frames == 1 ? 1 : cnt, x.ckeep, P));
        }
        if (x.jp) {      // the encoder takes the place of the delivery into the output form; it reads the float32 frame at the delivered size
            if (!guided && !x.comp && delivering) {
                RCHK(deliver_launch(h, q, sl.dl_buf, cnt, PH, PW, OH, OW, sl.gd_q, OUT_F32, contiguous_view(VL_HWC, OH, OW)));
                P = sl.gd_q;
            }
            JpegP p = *x.jp;
            p.B = cnt; p.in = P; p.coef = sl.jp_coef;
            p.out = (uint8_t*)d_out + (size_t)b0 * p.cap; p.sizes = x.jp_sizes + b0;
            p.lens = sl.jp_idx; p.offs = sl.jp_idx + (size_t)cnt * p.n_int;
            RCHK(jpeg_blocks_launch(h, q, p));
            RCHK(jpeg_entropy_launch(h, q, p));
            continue;
        }
        if (pic) {      // the request's float32 frame into the window of the canvas, the canvas at equal size into the output form
            RCHK(deliver_launch(h, q, P, cnt, PH, PW, OH, OW, sl.pc_canvas, OUT_F32, vcw));
            RCHK(deliver_launch(h, q, sl.pc_canvas, cnt, x.FH, x.FW, x.FH, x.FW, dst, x.fmt, vo));
            continue;
        }
        RCHK(deliver_launch(h, q, P, cnt, PH, PW, OH, OW, dst, x.fmt, vo));
    }
    if (bracket) {
        HIPCHK(hipEventRecord(sl.ev, sl.stream));
        HIPCHK(hipStreamWaitEvent(caller.stream, sl.ev, 0));
    }
    return RRV_OK;
}

// the grouped models alternate over slots 0 and 1 only: each slot's launches use its own sixteen state sets
static int next_frame_slot(rrv_handle h) { return next_device_slot(h) & 1; }
static int next_slot(rrv_handle h, const Xfer& x) { return x.model == Model::GLOBAL ? next_device_slot(h) : next_frame_slot(h); }

// the device entries (float32 and _u8 forms): [B][H][W][3] uint8 in HBM -> stylized frames in HBM, asynchronous on the slot's stream
static int device_entry(rrv_handle h, const void* d_in, void* d_out, const Xfer& x) {
    if (!h || !d_in || !d_out) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(check_xfer(h, x));
    return run_xfer(h, next_slot(h, x), d_in, d_out, x);
}

int rrv_transfer_batch_device(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::GLOBAL, B, H, W, PLAIN, OUT_F32});
}
int rrv_transfer_batch_device_u8(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::GLOBAL, B, H, W, PLAIN, OUT_U8});
}

int rrv_transfer_frames_device(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::GLOBAL, B, H, W, PADDED, OUT_F32});
}
int rrv_transfer_frames_device_u8(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::GLOBAL, B, H, W, PADDED, OUT_U8});
}

int rrv_transfer_device(rrv_handle h, const void* d_in, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::GLOBAL, 1, H, W, PLAIN, OUT_F32});
}
int rrv_transfer_device_u8(rrv_handle h, const void* d_in, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::GLOBAL, 1, H, W, PLAIN, OUT_U8});
}

int rrv_transfer_frame_mode_batch_device(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::FRAME, B, H, W, PLAIN, OUT_F32});
}
int rrv_transfer_frame_mode_batch_device_u8(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::FRAME, B, H, W, PLAIN, OUT_U8});
}

int rrv_transfer_frame_mode_frames_device(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::FRAME, B, H, W, PADDED, OUT_F32});
}
int rrv_transfer_frame_mode_frames_device_u8(rrv_handle h, const void* d_in, int B, int H, int W, void* d_out) {
    return device_entry(h, d_in, d_out, Xfer{Model::FRAME, B, H, W, PADDED, OUT_U8});
}

// rrv_transfer_image_device: the device entries above with the content frames read as `in` (conv_first_k<IN>) and the
// stylized frames written as `out` (conv_last_k<U8, CHW, SPACE>); hip_stream orders this call only.  x: the model, B, H, W and what
// the model blends with; the flags and `out` supply the rest (RRV_TF_FRAME_MODE turns GLOBAL into FRAME)
static int refuse_image(rrv_handle h, DescErr e, const char* side) {
    if (e == DescErr::U8_SPACE) return fail(h, RRV_E_ARG, std::string("transfer_image: a uint8 ") + side + " is in the PIXEL space");
    if (e == DescErr::YUV_TYPE) return fail(h, RRV_E_ARG, "transfer_image: an I420 / NV12 output is uint8, an I420_16 / P016 output uint16, in the PIXEL space");
    return fail(h, RRV_E_ARG, "transfer_image: unknown dtype, layout or space");
}
// The view entries: frames read through `in` (conv_first_k<IN>, every layout) and written through `out` (conv_last_k's store forms).  x: the model,
// B, H, W and what the model blends with; the views, the flags and hip_stream supply the rest (RRV_TF_FRAME_MODE turns GLOBAL into FRAME).
// who: the entry family in the refusal texts.  Everything is checked before any GPU work.
static int view_run(rrv_handle h, const char* who, const void* d_in, const rrv_image_view* in, void* d_out, const rrv_image_view* out, int flags,
                    void* hip_stream, Xfer x) {
    if (!h) return RRV_E_ARG;
    const std::string w = std::string(who) + ": ";
    if (!in || !out) return fail(h, RRV_E_ARG, w + "null view");
    if (!parse_in_view(in->desc, &x.in)) return fail(h, RRV_E_ARG, w + "in.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (!view_desc_ok(out->desc) || parse_out(out->desc, &x.fmt) != DescErr::OK)      // (a descriptor entry has refused its own in its own words)
        return fail(h, RRV_E_ARG, w + "out.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (flags & ~(RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE | RRV_TF_ON_STREAM | (x.model == Model::BLEND ? RRV_TF_WEIGHTS_DEVICE : 0)))
        return fail(h, RRV_E_ARG, w + "unknown flags");
    if (!d_in || !d_out) return fail(h, RRV_E_ARG, w + "null buffer");
    if (flags & RRV_TF_FRAME_MODE) {
        if (x.model != Model::GLOBAL) return fail(h, RRV_E_ARG, w + "the frame-mode model has no blended state (style weights need the global model)");
        x.model = Model::FRAME;
    }
    x.pad = flags & RRV_TF_PAD_CROP;
    x.w_dev = flags & RRV_TF_WEIGHTS_DEVICE;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(check_xfer(h, x));
    std::string why;
    if (!view_check(*in, x.B, x.IH(), x.IW(), false, &why)) return fail(h, RRV_E_ARG, w + "in." + why);      // (a scaled request: the source frame)
    if (!view_check(*out, x.B, x.OH(), x.OW(), true, &why)) return fail(h, RRV_E_ARG, w + "out." + why);      // (the view's geometry alone: with x.jp, d_out holds byte slots, not this view's frames)
    x.vin = in; x.vout = out;
    if (hip_stream || (flags & RRV_TF_ON_STREAM)) { x.on_stream = true; x.with = (hipStream_t)hip_stream; }      // hip_stream orders this call only
    return run_xfer(h, next_slot(h, x), d_in, d_out, x);
}
int rrv_transfer_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int H, int W, void* d_out, const rrv_image_view* out,
                             int flags, void* hip_stream) {
    return view_run(h, "transfer_view", d_in, in, d_out, out, flags, hip_stream, Xfer{Model::GLOBAL, B, H, W});
}
int rrv_transfer_view_blend_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int H, int W, const float* style_weight,
                                   int n_styles, void* d_out, const rrv_image_view* out, int flags, void* hip_stream) {
    return view_run(h, "transfer_view", d_in, in, d_out, out, flags, hip_stream, Xfer{Model::BLEND, B, H, W, PLAIN, OUT_F32, n_styles, style_weight});
}
int rrv_transfer_view_mask_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int H, int W, const float* d_mask, int n_styles,
                                  int mask_images, void* d_out, const rrv_image_view* out, int flags, void* hip_stream) {
    return view_run(h, "transfer_view", d_in, in, d_out, out, flags, hip_stream,
                    Xfer{Model::MASK, B, H, W, PLAIN, OUT_F32, n_styles, /* wts */ nullptr, d_mask, mask_images});
}
// The descriptor entries are the view entries on contiguous views.  Each family refuses a descriptor or layout in its own words first (the
// texts are part of what callers see); a frame size is judged by the shared checks, so the views are built for whatever size was passed.
static int image_run(rrv_handle h, const void* d_in, rrv_image_desc in, void* d_out, rrv_image_desc out, int flags, void* hip_stream, const Xfer& x) {
    OutFmt f;
    if (const DescErr e = parse_out(out, &f); e != DescErr::OK) return refuse_image(h, e, "output");
    const bool pad = flags & RRV_TF_PAD_CROP;
    const rrv_image_view vi = contiguous_of(in, x.H, x.W), vo = contiguous_of(out, pad ? x.H : x.H / 8 * 8, pad ? x.W : x.W / 8 * 8);
    return view_run(h, "transfer_image", d_in, &vi, d_out, &vo, flags, hip_stream, x);
}
static int image_entry(rrv_handle h, const void* d_in, rrv_image_desc in, void* d_out, rrv_image_desc out, int flags, void* hip_stream, const Xfer& x) {
    if (!h) return RRV_E_ARG;
    InFmt f;
    if (const DescErr e = parse_in(in, &f); e != DescErr::OK) return refuse_image(h, e, "input");
    return image_run(h, d_in, in, d_out, out, flags, hip_stream, x);
}
// the same entries reading YUV 4:2:0 frames (conv_first_k<IN_YUV_*>): [B][H*W + 2*CH*CW] uint8 (uint16 for the two 16-bit layouts) in HBM
static int from_yuv_device(rrv_handle h, const void* d_in, int in_layout, void* d_out, rrv_image_desc out, int flags, void* hip_stream, const Xfer& x) {
    if (!h) return RRV_E_ARG;
    InFmt f;
    if (parse_in_yuv(in_layout, &f) != DescErr::OK) return refuse_layout(h, "transfer_from_yuv: in_layout");
    if (x.H < 8 || x.W < 8) return fail(h, RRV_E_ARG, "transfer_from_yuv: frames must be at least 8 x 8 pixels");
    return image_run(h, d_in, rrv_image_desc{yuv16_layout(in_layout) ? RRV_DT_U16 : RRV_DT_U8, in_layout, RRV_SP_PIXEL}, d_out, out, flags, hip_stream, x);
}
int rrv_transfer_from_yuv_device(rrv_handle h, const void* d_in, int in_layout, int B, int H, int W, void* d_out, rrv_image_desc out, int flags,
                                 void* hip_stream) {
    return from_yuv_device(h, d_in, in_layout, d_out, out, flags, hip_stream, Xfer{Model::GLOBAL, B, H, W});
}
int rrv_transfer_blend_from_yuv_device(rrv_handle h, const void* d_in, int in_layout, int B, int H, int W, const float* style_weight, int n_styles,
                                       void* d_out, rrv_image_desc out, int flags, void* hip_stream) {
    return from_yuv_device(h, d_in, in_layout, d_out, out, flags, hip_stream, Xfer{Model::BLEND, B, H, W, PLAIN, OUT_F32, n_styles, style_weight});
}
int rrv_transfer_mask_from_yuv_device(rrv_handle h, const void* d_in, int in_layout, int B, int H, int W, const float* d_mask, int n_styles,
                                      int mask_images, void* d_out, rrv_image_desc out, int flags, void* hip_stream) {
    return from_yuv_device(h, d_in, in_layout, d_out, out, flags, hip_stream,
                           Xfer{Model::MASK, B, H, W, PLAIN, OUT_F32, n_styles, /* wts */ nullptr, d_mask, mask_images});
}
int rrv_transfer_image_device(rrv_handle h, const void* d_in, rrv_image_desc in, int B, int H, int W, void* d_out, rrv_image_desc out,
                              int flags, void* hip_stream) {
    return image_entry(h, d_in, in, d_out, out, flags, hip_stream, Xfer{Model::GLOBAL, B, H, W});
}
// one weight vector per image ([B][ns]; in HBM with RRV_TF_WEIGHTS_DEVICE)
int rrv_transfer_image_blend_device(rrv_handle h, const void* d_in, rrv_image_desc in, int B, int H, int W, const float* style_weight, int n_styles,
                                    void* d_out, rrv_image_desc out, int flags, void* hip_stream) {
    return image_entry(h, d_in, in, d_out, out, flags, hip_stream, Xfer{Model::BLEND, B, H, W, PLAIN, OUT_F32, n_styles, style_weight});
}
// the styles blended per pixel by [mask_images][ns][H][W] float32 masks in HBM
int rrv_transfer_image_mask_device(rrv_handle h, const void* d_in, rrv_image_desc in, int B, int H, int W, const float* d_mask, int n_styles,
                                   int mask_images, void* d_out, rrv_image_desc out, int flags, void* hip_stream) {
    return image_entry(h, d_in, in, d_out, out, flags, hip_stream, Xfer{Model::MASK, B, H, W, PLAIN, OUT_F32, n_styles, /* wts */ nullptr, d_mask, mask_images});
}

// The one-frame blended device entries are serialised (one call at a time, on slot 0 and its state set 0); the next alternating
// call starts there.  A group of one frame of run_xfer.
static int serial_blend_entry(rrv_handle h, const void* d_in, void* d_out, const Xfer& x) {
    if (!h || !d_in || !d_out) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    h->next_slot = 0;
    RCHK(check_xfer(h, x, false, true));
    return run_xfer(h, 0, d_in, d_out, x);
}
int rrv_transfer_blend_device(rrv_handle h, const void* d_in, int H, int W, const float* wts, int ns, void* d_out) {
    return serial_blend_entry(h, d_in, d_out, Xfer{Model::BLEND, 1, H, W, PLAIN, OUT_F32, ns, wts});
}
int rrv_transfer_blend_device_u8(rrv_handle h, const void* d_in, int H, int W, const float* wts, int ns, void* d_out) {
    return serial_blend_entry(h, d_in, d_out, Xfer{Model::BLEND, 1, H, W, PLAIN, OUT_U8, ns, wts});
}

// B frames in sub-batches of up to 8 through four staging sets.  Three engines run concurrently: the H2D copy of
// sub-batch k+1.. (copy_in stream), the kernels of k and k+1 (the two compute streams), the D2H copy of k-1 (copy_out
// stream); events order a set's H2D -> kernels -> D2H and its re-use four sub-batches later.  With pageable caller
// arrays the host additionally copies into / out of the pinned staging buffers while all of that runs.
// Pixels per sub-batch of the host entries: 16 frames at the 512x512 configuration's padded size (32 at 384 x 384, 4 at 1152 x 1152).
// Round 4: 8 -> 16.  conv_f43_k's work items are 32 x 32 pixels, so at 8 frames the 160 x 160 layers have 1600 items = 6.25 rounds
// of the 256 persistent workgroups (a seventh, quarter-filled round: 11 % lost), at 16 frames 12.5; measured 678 -> 698 frames/s
// at 512 x 512, 1 800 -> 1 939 at 256 x 256 (RRV_SUB_BATCH_FRAMES_640 = 8 / 12 / 16 / 32: 678 / 692 / 698 / 687, the last one
// too coarse for the copy / kernel overlap of a 64-frame call).
static long host_sub_pixels() {
    static const long v = [] { const char* e = getenv("RRV_SUB_BATCH_FRAMES_640"); const long n = e ? atol(e) : 16; return (n < 1 ? 1 : n > 64 ? 64 : n) * 640L * 640L; }();
    return v;
}
#define HOST_SUB_PIXELS host_sub_pixels()
constexpr int HOST_SETS = 4;
static int host_sub(int B, int H, int W) {              // frames per sub-batch: small frames are grouped, large ones split finer
    long s = HOST_SUB_PIXELS / ((long)H * W);
    if (s > 32) s = 32;
    if (s < 1) s = 1;
    return B < s ? B : (int)s;
}
// copies between the caller's pageable arrays and the pinned staging buffers: first-touch page faults of a fresh
// output array make a single thread slower than the GPU, so large copies are split over a few threads
// A small persistent pool does the slices (round 5): creating std::threads per copy cost more than the 1.2 MB input frame of
// a one-frame transfer() takes to copy, so that copy ran on one thread at ~10 GB/s = 0.12 ms of a 1.96 ms call.  The pool is
// created on first use and never destroyed (its workers block on a condition variable; a static object torn down at exit
// under them would be a crash); a second caller at the same time (another handle on another thread) copies by itself.
namespace {
struct CopyPool {
    static constexpr int NW = 3;
    std::mutex mu, call_mu;
    std::condition_variable cv, done_cv;
    struct Job { char* dst; const char* src; size_t n; } jobs[NW];
    unsigned long gen = 0;
    int pending = 0;
    CopyPool() {
        for (int i = 0; i < NW; ++i)
            std::thread([this, i] {
                unsigned long seen = 0;
                for (;;) {
                    Job j;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return gen != seen; });
                        seen = gen;
                        j = jobs[i];
                    }
                    if (j.n) memcpy(j.dst, j.src, j.n);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (--pending == 0) done_cv.notify_one();
                    }
                }
            }).detach();
    }
    // copies [slice, bytes) on the workers in nt - 1 slices while the caller copies [0, slice)
    void run(char* dst, const char* src, size_t bytes, int nt, size_t slice) {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (int t = 0; t < NW; ++t) {
                const size_t o = (size_t)(t + 1) * slice;
                jobs[t] = Job{dst + o, src + o, (t + 1 < nt && o < bytes) ? (bytes - o < slice ? bytes - o : slice) : 0};
            }
            pending = NW;
            ++gen;
        }
        cv.notify_all();
        memcpy(dst, src, slice < bytes ? slice : bytes);
        std::unique_lock<std::mutex> lk(mu);
        done_cv.wait(lk, [&] { return pending == 0; });
    }
};
}  // namespace
static void host_copy(void* dst, const void* src, size_t bytes) {
    constexpr size_t MIN_SLICE = (size_t)256 << 10;
    int nt = (int)(bytes / MIN_SLICE);
    if (nt > 4) nt = 4;
    if (nt < 2) { memcpy(dst, src, bytes); return; }
    static CopyPool* const pool = new CopyPool();
    std::unique_lock<std::mutex> call(pool->call_mu, std::try_to_lock);
    if (!call.owns_lock()) { memcpy(dst, src, bytes); return; }
    const size_t slice = ((bytes / nt) + 4095) & ~(size_t)4095;
    pool->run((char*)dst, (const char*)src, bytes, nt, slice);
}
// caller buffers that are page-locked (rrv_host_alloc / rrv_host_register, or any hipHostMalloc'ed / registered range)
// are DMA'd directly: no staging copy through the library's pinned buffers
static std::mutex g_pin_mu;
static std::map<const char*, size_t> g_pin_ranges;      // blocks handed out by rrv_host_alloc (the Python class's output pool): known page-locked without asking the runtime
static bool is_pinned(const void* ptr, size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_ranges.upper_bound((const char*)ptr);
        if (it != g_pin_ranges.begin()) {
            --it;
            if ((const char*)ptr + bytes <= it->first + it->second) return true;
        }
    }
    hipPointerAttribute_t a;
    for (const char* q : {(const char*)ptr, (const char*)ptr + (bytes ? bytes - 1 : 0)}) {      // (a pageable array fails at its first byte: one query)
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}
static int retire_ticket(rrv_handle h, int set);
// RRV_TIMELINE: one line per call of a pipelined host entry, every time in ms after the entry event (recorded on an idle stream once the
// staging is claimed, `setup` ms of host time into the call): the start of the first kernel, the end of each sub-batch's last kernel and
// of its D2H, and the host's wall time from entry to return.  tools/call_timeline.py reads these lines.
static int timeline_print(rrv_handle h, const char* who, int frames, int H, int W, int n, double setup_ms, double wall_ms) {
    auto& tl = h->tl;
    auto at = [&](hipEvent_t e) { float ms = -1.f; if (hipEventElapsedTime(&ms, tl.entry, e) != hipSuccess) { (void)hipGetLastError(); ms = -1.f; } return ms; };
    std::string line;
    char b[96];
    snprintf(b, sizeof b, "rrv_timeline %s frames=%d size=%dx%d subs=%d", who, frames, H, W, n); line += b;
    snprintf(b, sizeof b, " setup=%.3f wall=%.3f first_kernel=%.3f k_end=", setup_ms, wall_ms, at(tl.first)); line += b;
    for (int k = 0; k < n; ++k) { snprintf(b, sizeof b, "%s%.3f", k ? "," : "", at(tl.k_end[k])); line += b; }
    line += " d2h_end=";
    for (int k = 0; k < n; ++k) { snprintf(b, sizeof b, "%s%.3f", k ? "," : "", at(tl.d_end[k])); line += b; }
    fprintf(stderr, "%s\n", line.c_str());
    return RRV_OK;
}
static double host_ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
// frames per piece of a last sub-batch of nb frames of H x W (0: delivered whole): h->host_piece_px pixels, at most PIECES_MAX pieces
static int tail_piece(rrv_handle h, int nb, int H, int W) {
    if (h->host_piece_px <= 0) return 0;
    long p = h->host_piece_px / ((long)H * W);
    const long least = (nb + rrv_ctx::HostStage::PIECES_MAX - 1) / rrv_ctx::HostStage::PIECES_MAX;
    if (p < least) p = least;
    if (p < 1) p = 1;
    return p < nb ? (int)p : 0;
}
// The entries that use all staging sets: open look-ahead tickets own sets, so retire them and wait for everything; the
// entry then runs its own slots, and the alternating device entries start again at slot 0 after it.
static int claim_staging(rrv_handle h) {
    for (int i = 0; i < HOST_SETS; ++i) RCHK(retire_ticket(h, i));
    RCHK(sync_all(h));
    h->next_slot = 0;
    return RRV_OK;
}
// The host entries: x.B frames from `frames` to `out` (float32, uint8 or 8-bit YUV 4:2:0 by x.fmt, x.out_bytes() per frame), any B >= 1.  The grouped models run sub-batches of at
// most MS_GROUP_MAX frames, one launch sequence each; the blended one takes the sub-batch's rows of x.wts, the masked one the set's
// staged mask block.  state_first: check_xfer's.
static int host_pipeline(rrv_handle h, const uint8_t* frames, void* out, const Xfer& x, bool state_first = false) {
    if (!h || !frames || !out) return RRV_E_ARG;
    const auto t_entry = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(h->dev));
    RCHK(check_xfer(h, x, true, state_first));
    const int B = x.B;
    // what rides the staging beside the frames: the MASK model's style masks, or a compositing request's matte (host memory here); in bytes
    const char* const mask = x.comp ? (const char*)x.cmatte : (const char*)x.mask;
    const int mask_images = x.comp ? x.cm_frames : x.mask_images;
    const size_t fb = x.in_bytes();                                        // input bytes per frame
    const size_t fob = x.out_bytes();                     // output bytes per frame
    char* const outc = (char*)out;
    int sub = x.model == Model::GLOBAL ? host_sub(B, x.KH(), x.KW()) : std::min(host_sub(B, x.KH(), x.KW()), (int)rrv_ctx::MS_GROUP_MAX);
    // The kernels' work follows the working frame, the staging the SOURCE frame: a scaled request's sub-batch also holds at most four times
    // HOST_SUB_PIXELS of source pixels (2 x per axis keeps the unscaled call's sub-batches; at 8 x 8 a sub-batch is one or two frames), so
    // the page-locked and device staging per set stays within four times the unscaled call's.
    if (x.scaled()) sub = (int)std::max(1L, std::min((long)sub, 4 * HOST_SUB_PIXELS / ((long)x.SH * x.SW)));
    // the same rule for the DELIVERED frame, which sizes the output staging
    if (x.staged()) sub = (int)std::max(1L, std::min((long)sub, 4 * HOST_SUB_PIXELS / ((long)x.OH() * x.OW())));
    // a picture request stages and delivers the WHOLE frame
    if (x.pic) sub = (int)std::max(1L, std::min((long)sub, 4 * HOST_SUB_PIXELS / ((long)x.FH * x.FW)));
    const size_t mfb = x.comp ? x.matte_bytes() : x.mask_floats() * sizeof(float);      // of one image's masks / one frame's matte
    auto run = [&](int slot, int k, const void* d_in, int nb, void* d_out, const SeqHook* hk) -> int {      // sub-batch k's kernels
        Xfer part = x;
        part.B = nb;
        if (x.wts) part.wts = x.wts + (size_t)k * sub * x.ns;
        if (mask && !x.comp) { part.mask = h->hstage[k % HOST_SETS].mask; part.mask_images = mask_images == 1 ? 1 : nb; }
        if (x.comp) {      // strengths and a per-frame matte by the frame's position in the whole call
            if (x.cstr) part.cstr = x.cstr + (size_t)k * sub;
            if (mask) { part.cmatte = h->hstage[k % HOST_SETS].mask; part.cm_frames = mask_images == 1 ? 1 : nb; }
        }
        return run_xfer(h, slot, d_in, d_out, part, hk);
    };
    const bool in_pin = is_pinned(frames, (size_t)B * fb), out_pin = is_pinned(out, (size_t)B * fob);
    // the masks are staged like the frames: a sub-batch's part goes through the set's page-locked block (unless the caller's array is
    // page-locked) to its HBM block by a copy on copy_in, in front of the in_done event its kernels wait for; k_done frees both again
    const size_t msub = ((size_t)(mask_images == 1 ? 1 : sub) * mfb + sizeof(float) - 1) / sizeof(float);      // floats of a set's block
    const bool m_pin = mask && is_pinned(mask, (size_t)mask_images * mfb);
    const bool host_in = !in_pin || (mask && !m_pin);      // a page-locked input block of the set is refilled by the host
    RCHK(claim_staging(h));
    const int nchunk = (B + sub - 1) / sub;
    auto slot_of = [&](int k) { return h->profiling ? 0 : (k & 1) % h->n_slots; };      // the compute slot of sub-batch k
    const int nsets = nchunk < HOST_SETS ? nchunk : HOST_SETS;
    const bool zin = h->host_io == 1 || h->host_io == 2, zout = h->host_io == 1 || h->host_io == 3;
    // The tail wait and the piecewise delivery (SeqHook) order the sub-batches of the models that run transfer_device, on two streams with
    // staged copies both ways.  Everything else keeps one launch per layer and sub-batch, unordered: one sub-batch or one stream, the
    // profiled step (slot 0 only), the debug levels, a caller's stream, zero copy.
    // A delivering request too: the piecewise drain hooks into transfer_device's last launch, which is then not the request's last kernel.
    const bool ordered = nchunk > 1 && h->n_slots > 1 && !h->profiling && !h->debug && !x.order(h).sync && h->host_io == 0 &&
                         (x.model == Model::GLOBAL || x.model == Model::BLEND) && !x.indirect();
    const bool tl_on = h->tl.on && nchunk > 1 && nchunk <= rrv_ctx::Timeline::N && h->host_io == 0;
    double tl_setup = 0;
    if (tl_on) { tl_setup = host_ms_since(t_entry); HIPCHK(hipEventRecord(h->tl.entry, h->slots[0].stream)); }
    // a scaled, delivering or guided request: the tables and each compute slot's buffers, before the first launch
    for (int k = 0; k < std::min(nchunk, 2); ++k) RCHK(reserve_stages(h, slot_of(k), sub, x));      // (slot_of has period 2)
    for (int i = 0; i < nsets; ++i) {      // device staging for the copied directions, pinned staging for pageable caller arrays
        RCHK(stage_reserve(h, i, zin ? 0 : (size_t)sub * fb, zout ? 0 : (size_t)sub * fob, false));
        RCHK(stage_reserve(h, i, in_pin ? 0 : (size_t)sub * fb, out_pin ? 0 : (size_t)sub * fob, true));
        if (!mask) continue;
        rrv_ctx::HostStage& st = h->hstage[i];
        RCHK(ensure_dev(h, st.mask, st.mask_cap, msub));
        if (!m_pin && st.mask_pin_cap < msub) {
            if (st.mask_pin) (void)hipHostFree(st.mask_pin);
            st.mask_pin = nullptr; st.mask_pin_cap = 0;
            if (hipHostMalloc((void**)&st.mask_pin, msub * sizeof(float), hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                st.mask_pin = nullptr;
                return fail(h, RRV_E_NOMEM, "staging: out of page-locked host memory");
            }
            st.mask_pin_cap = msub;
        }
    }
    auto count = [&](int k) { return (k + 1) * sub <= B ? sub : B - k * sub; };
    auto drain = [&](int k) -> int {       // sub-batch k delivered (its staging set is free again)
        auto& st = h->hstage[k % HOST_SETS];
        HIPCHK(hipEventSynchronize(st.out_done));
        if (!out_pin) host_copy(outc + (size_t)k * sub * fob, st.pin.out, (size_t)count(k) * fob);
        return RRV_OK;
    };
    int rc = RRV_OK;
    for (int k = 0; k < nchunk && rc == RRV_OK; ++k) {
        auto& st = h->hstage[k % HOST_SETS];
        const bool reuse = k >= HOST_SETS;
        if (reuse && (host_in || !out_pin)) rc = drain(k - HOST_SETS);   // pinned staging of this set is about to be overwritten
        if (rc != RRV_OK) break;
        const int nb = count(k);
        const uint8_t* src = frames + (size_t)k * sub * fb;
        if (!in_pin) { host_copy(st.pin.in, src, (size_t)nb * fb); src = st.pin.in; }
        const char* msrc = nullptr;
        size_t mbytes = 0;
        if (mask) {
            msrc = mask + (mask_images == 1 ? 0 : (size_t)k * sub * mfb);
            mbytes = (size_t)(mask_images == 1 ? 1 : nb) * mfb;
            if (!m_pin) { host_copy(st.mask_pin, msrc, mbytes); msrc = (const char*)st.mask_pin; }
        }
        const int slot = slot_of(k);
        hipStream_t cs = h->slots[slot].stream;
        if (nchunk == 1 && h->host_io == 0) {     // one sub-batch (the reference's one-frame-per-call surface): nothing to overlap, one stream, no events
            HIPCHK(hipMemcpyAsync(st.dev.in, src, (size_t)nb * fb, hipMemcpyHostToDevice, cs));
            if (mask) HIPCHK(hipMemcpyAsync(st.mask, msrc, mbytes, hipMemcpyHostToDevice, cs));
            rc = run(slot, k, st.dev.in, nb, st.dev.out, nullptr);
            if (rc != RRV_OK) break;
            HIPCHK(hipMemcpyAsync(out_pin ? out : st.pin.out, st.dev.out, (size_t)nb * fob, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipStreamSynchronize(cs));
            if (!out_pin) host_copy(out, st.pin.out, (size_t)nb * fob);
            return RRV_OK;
        }
        // zero copy per direction (rrv_set_host_io: 1 both, 2 input only, 3 output only): the first kernel reads the page-locked
        // source over PCIe / the last one writes the destination; the other direction keeps its copy stream
        const uint8_t* k_in = src;
        if (!zin || mask) {
            if (reuse) HIPCHK(hipStreamWaitEvent(h->copy_in, st.k_done, 0));       // the kernels of k-4 have read d_in (and the set's masks)
            if (!zin) {
                HIPCHK(hipMemcpyAsync(st.dev.in, src, (size_t)nb * fb, hipMemcpyHostToDevice, h->copy_in));
                k_in = st.dev.in;
            }
            if (mask) HIPCHK(hipMemcpyAsync(st.mask, msrc, mbytes, hipMemcpyHostToDevice, h->copy_in));
            HIPCHK(hipEventRecord(st.in_done, h->copy_in));
            HIPCHK(hipStreamWaitEvent(cs, st.in_done, 0));
        }
        void* const h_dst = out_pin ? outc + (size_t)k * sub * fob : st.pin.out;
        if (reuse) HIPCHK(hipStreamWaitEvent(cs, st.out_done, 0));             // d_out / pin_out of k-4 has been delivered
        void* const k_out = zout ? h_dst : st.dev.out;
        SeqHook hk;
        if (ordered) {
            if (h->host_phase && k > 0) hk.tail_wait = h->hstage[(k - 1) % HOST_SETS].k_done;      // recorded in this call, behind sub-batch k-1's last kernel
            if (k == nchunk - 1) {
                hk.piece = tail_piece(h, nb, x.KH(), x.KW());
                hk.h_dst = (char*)h_dst; hk.frame_bytes = fob; hk.copy = h->copy_out; hk.ev = st.piece_ev;
            }
        }
        if (tl_on && k == 0) HIPCHK(hipEventRecord(h->tl.first, cs));
        rc = run(slot, k, k_in, nb, k_out, ordered ? &hk : nullptr);
        if (rc != RRV_OK) break;
        if (tl_on) HIPCHK(hipEventRecord(h->tl.k_end[k], cs));
        if (!zin || mask) HIPCHK(hipEventRecord(st.k_done, cs));
        if (zout) { HIPCHK(hipEventRecord(st.out_done, cs)); continue; }
        if (zin && !mask) HIPCHK(hipEventRecord(st.k_done, cs));
        if (hk.piece == 0) {      // (in pieces: transfer_device has queued each range's copy behind its conv_last)
            HIPCHK(hipStreamWaitEvent(h->copy_out, st.k_done, 0));
            HIPCHK(hipMemcpyAsync(h_dst, st.dev.out, (size_t)nb * fob, hipMemcpyDeviceToHost, h->copy_out));
        }
        HIPCHK(hipEventRecord(st.out_done, h->copy_out));
        if (tl_on) HIPCHK(hipEventRecord(h->tl.d_end[k], h->copy_out));
    }
    if (rc != RRV_OK) { (void)sync_all(h); return rc; }
    const int first_open = (host_in || !out_pin) ? (nchunk - HOST_SETS < 0 ? 0 : nchunk - HOST_SETS) : 0;
    if (!host_in && out_pin) {               // nothing to copy on the host: the last D2H of each stream order completes everything
        if (zout) RCHK(sync_all(h));
        else HIPCHK(hipStreamSynchronize(h->copy_out));
    } else {
        for (int k = first_open; k < nchunk; ++k) RCHK(drain(k));
    }
    if (tl_on) RCHK(timeline_print(h, "host_pipeline", B, x.KH(), x.KW(), nchunk, tl_setup, host_ms_since(t_entry)));
    return RRV_OK;
}

int rrv_transfer(rrv_handle h, const uint8_t* frame, int H, int W, float* out) {
    return host_pipeline(h, frame, out, Xfer{Model::GLOBAL, 1, H, W, PLAIN, OUT_F32});
}
int rrv_transfer_u8(rrv_handle h, const uint8_t* frame, int H, int W, uint8_t* out) {
    return host_pipeline(h, frame, out, Xfer{Model::GLOBAL, 1, H, W, PLAIN, OUT_U8});
}

// one frame with one blended state, one frame of the frame mode: a request of one sub-batch (no event, one stream, slot 0 and its state set 0)
int rrv_transfer_blend(rrv_handle h, const uint8_t* frame, int H, int W, const float* wts, int ns, float* out) {
    return host_pipeline(h, frame, out, Xfer{Model::BLEND, 1, H, W, PLAIN, OUT_F32, ns, wts}, true);
}
int rrv_transfer_blend_u8(rrv_handle h, const uint8_t* frame, int H, int W, const float* wts, int ns, uint8_t* out) {
    return host_pipeline(h, frame, out, Xfer{Model::BLEND, 1, H, W, PLAIN, OUT_U8, ns, wts}, true);
}
int rrv_transfer_frame_mode(rrv_handle h, const uint8_t* frame, int H, int W, float* out) {
    return host_pipeline(h, frame, out, Xfer{Model::FRAME, 1, H, W, PLAIN, OUT_F32});
}
int rrv_transfer_frame_mode_u8(rrv_handle h, const uint8_t* frame, int H, int W, uint8_t* out) {
    return host_pipeline(h, frame, out, Xfer{Model::FRAME, 1, H, W, PLAIN, OUT_U8});
}

int rrv_transfer_batch(rrv_handle h, const uint8_t* frames, int B, int H, int W, float* out) {
    return host_pipeline(h, frames, out, Xfer{Model::GLOBAL, B, H, W, PLAIN, OUT_F32});
}
int rrv_transfer_batch_u8(rrv_handle h, const uint8_t* frames, int B, int H, int W, uint8_t* out) {
    return host_pipeline(h, frames, out, Xfer{Model::GLOBAL, B, H, W, PLAIN, OUT_U8});
}

int rrv_transfer_frames(rrv_handle h, const uint8_t* frames, int B, int H, int W, float* out) {
    return host_pipeline(h, frames, out, Xfer{Model::GLOBAL, B, H, W, PADDED, OUT_F32});
}
int rrv_transfer_frames_u8(rrv_handle h, const uint8_t* frames, int B, int H, int W, uint8_t* out) {
    return host_pipeline(h, frames, out, Xfer{Model::GLOBAL, B, H, W, PADDED, OUT_U8});
}

int rrv_transfer_blend_batch(rrv_handle h, const uint8_t* frames, int B, int H, int W, const float* wts, int ns, int pad_crop, float* out) {
    return host_pipeline(h, frames, out, Xfer{Model::BLEND, B, H, W, pad_crop != 0, OUT_F32, ns, wts});
}
int rrv_transfer_blend_batch_u8(rrv_handle h, const uint8_t* frames, int B, int H, int W, const float* wts, int ns, int pad_crop, uint8_t* out) {
    return host_pipeline(h, frames, out, Xfer{Model::BLEND, B, H, W, pad_crop != 0, OUT_U8, ns, wts});
}

int rrv_transfer_mask_batch(rrv_handle h, const uint8_t* frames, int B, int H, int W, const float* mask, int ns, int mask_images, int pad_crop, float* out) {
    return host_pipeline(h, frames, out, Xfer{Model::MASK, B, H, W, pad_crop != 0, OUT_F32, ns, /* wts */ nullptr, mask, mask_images});
}
int rrv_transfer_mask_batch_u8(rrv_handle h, const uint8_t* frames, int B, int H, int W, const float* mask, int ns, int mask_images, int pad_crop, uint8_t* out) {
    return host_pipeline(h, frames, out, Xfer{Model::MASK, B, H, W, pad_crop != 0, OUT_U8, ns, /* wts */ nullptr, mask, mask_images});
}

int rrv_transfer_frame_mode_batch(rrv_handle h, const uint8_t* frames, int B, int H, int W, float* out) {
    return host_pipeline(h, frames, out, Xfer{Model::FRAME, B, H, W, PLAIN, OUT_F32});
}
int rrv_transfer_frame_mode_batch_u8(rrv_handle h, const uint8_t* frames, int B, int H, int W, uint8_t* out) {
    return host_pipeline(h, frames, out, Xfer{Model::FRAME, B, H, W, PLAIN, OUT_U8});
}

int rrv_transfer_frame_mode_frames(rrv_handle h, const uint8_t* frames, int B, int H, int W, float* out) {
    return host_pipeline(h, frames, out, Xfer{Model::FRAME, B, H, W, PADDED, OUT_F32});
}
int rrv_transfer_frame_mode_frames_u8(rrv_handle h, const uint8_t* frames, int B, int H, int W, uint8_t* out) {
    return host_pipeline(h, frames, out, Xfer{Model::FRAME, B, H, W, PADDED, OUT_U8});
}

// YUV 4:2:0 output of the host entries (conv_last_k's YUV form): frame b at b * (OH*OW + 2*CH*CW) samples of `out`, bytes or (layouts 8 / 9) uint16
static int yuv_host(rrv_handle h, const uint8_t* frames, int layout, void* out, Xfer x) {
    if (!h) return RRV_E_ARG;
    if (parse_out_yuv(layout, &x.fmt) != DescErr::OK) return refuse_layout(h, "transfer_yuv: layout");
    return host_pipeline(h, frames, out, x);
}
int rrv_transfer_yuv(rrv_handle h, const uint8_t* frames, int B, int H, int W, int flags, int layout, uint8_t* out) {
    if (!h) return RRV_E_ARG;
    if (flags & ~(RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE)) return fail(h, RRV_E_ARG, "transfer_yuv: unknown flags");
    return yuv_host(h, frames, layout, out, Xfer{flags & RRV_TF_FRAME_MODE ? Model::FRAME : Model::GLOBAL, B, H, W, (flags & RRV_TF_PAD_CROP) != 0});
}
int rrv_transfer_blend_batch_yuv(rrv_handle h, const uint8_t* frames, int B, int H, int W, const float* wts, int ns, int pad_crop, int layout, uint8_t* out) {
    return yuv_host(h, frames, layout, out, Xfer{Model::BLEND, B, H, W, pad_crop != 0, OUT_F32, ns, wts});
}
int rrv_transfer_mask_batch_yuv(rrv_handle h, const uint8_t* frames, int B, int H, int W, const float* mask, int ns, int mask_images, int pad_crop,
                                int layout, uint8_t* out) {
    return yuv_host(h, frames, layout, out, Xfer{Model::MASK, B, H, W, pad_crop != 0, OUT_F32, ns, /* wts */ nullptr, mask, mask_images});
}

// 8-bit YUV 4:2:0 input of the host entries (conv_first_k<IN_YUV_*>): frame b at b * (H*W + 2*CH*CW) bytes of `frames`; `out` as float32 or
// uint8 HWC BGR PIXEL frames or as I420 / NV12.  The staging, the zero-copy path and the copy pool size a frame by Xfer::in_bytes.
// The host entries that name their output by descriptor (_from_yuv, _scaled, _deliver) end alike, once each has parsed its input: the flags
// against those the entry knows, a refusal of the family's own (`refused`: its text, nullptr: none), the output descriptor, flags -> model
// and pad, the pipeline.  family: the entry family's name, the prefix of every refusal.
static int desc_host(rrv_handle h, const char* family, const uint8_t* frames, void* out, rrv_image_desc od, int flags, int known_flags, const char* refused, Xfer x) {
    const std::string who = std::string(family) + ": ";
    if (flags & ~known_flags) return fail(h, RRV_E_ARG, who + "unknown flags");
    if (refused) return fail(h, RRV_E_ARG, who + refused);
    if (parse_out(od, &x.fmt) != DescErr::OK || x.fmt.chw || x.fmt.space != SP_PIXEL)
        return fail(h, RRV_E_ARG, who + "the output is float32 or uint8 HWC BGR in the PIXEL space, uint8 I420 / NV12, or uint16 I420_16 / P016 (4:2:0, or with RRV_LAY_422 / RRV_LAY_444)");
    if (flags & RRV_TF_FRAME_MODE) x.model = Model::FRAME;
    x.pad = (flags & RRV_TF_PAD_CROP) != 0;
    return host_pipeline(h, frames, out, x);
}
static int from_yuv_host(rrv_handle h, const uint8_t* frames, int in_layout, void* out, rrv_image_desc od, int flags, int known_flags, Xfer x) {
    if (!h) return RRV_E_ARG;
    if (parse_in_yuv(in_layout, &x.in) != DescErr::OK) return refuse_layout(h, "transfer_from_yuv: in_layout");
    return desc_host(h, "transfer_from_yuv", frames, out, od, flags, known_flags, x.H < 8 || x.W < 8 ? "frames must be at least 8 x 8 pixels" : nullptr, x);
}
int rrv_transfer_from_yuv(rrv_handle h, const uint8_t* frames, int in_layout, int B, int H, int W, void* out, rrv_image_desc od, int flags) {
    return from_yuv_host(h, frames, in_layout, out, od, flags, RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE, Xfer{Model::GLOBAL, B, H, W});
}
int rrv_transfer_blend_from_yuv(rrv_handle h, const uint8_t* frames, int in_layout, int B, int H, int W, const float* wts, int ns, void* out,
                                rrv_image_desc od, int flags) {
    return from_yuv_host(h, frames, in_layout, out, od, flags, RRV_TF_PAD_CROP, Xfer{Model::BLEND, B, H, W, PLAIN, OUT_F32, ns, wts});
}
int rrv_transfer_mask_from_yuv(rrv_handle h, const uint8_t* frames, int in_layout, int B, int H, int W, const float* mask, int ns, int mask_images,
                               void* out, rrv_image_desc od, int flags) {
    return from_yuv_host(h, frames, in_layout, out, od, flags, RRV_TF_PAD_CROP, Xfer{Model::MASK, B, H, W, PLAIN, OUT_F32, ns, /* wts */ nullptr, mask, mask_images});
}

// ---- the scaled entries: frames of SH x SW resampled to the H x W working frame on the GPU, in front of everything else
// the resampler alone, queued on hip_stream itself (NULL: the null stream): nothing of the handle's own streams takes part
int rrv_resample_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W, float* d_out, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!in) return fail(h, RRV_E_ARG, "resample_view: null view");
    InFmt fmt;
    if (!parse_in_view(in->desc, &fmt)) return fail(h, RRV_E_ARG, "resample_view: in.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (!d_in || !d_out) return fail(h, RRV_E_ARG, "resample_view: null buffer");
    if (B < 1 || B > 64) return fail(h, RRV_E_ARG, "resample_view: batch must be in 1..64");
    RCHK(check_scale(h, "resample_view", SH, SW, H, W));
    std::string why;
    if (!view_check(*in, B, SH, SW, false, &why)) return fail(h, RRV_E_ARG, "resample_view: in." + why);
    HIPCHK(hipSetDevice(h->dev));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    return resample_launch(h, q, d_in, fmt, img_view(*in), B, SH, SW, H, W, d_out);
}
// the transfer behind the resampler and / or in front of the delivery stage (DH = DW = 0: none), views on both sides
static int scaled_view_run(rrv_handle h, const char* who, bool must_scale, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W,
                           int DH, int DW, void* d_out, const rrv_image_view* out, int flags, void* hip_stream) {
    Xfer x{Model::GLOBAL, B, H, W};
    x.SH = SH; x.SW = SW; x.DH = DH; x.DW = DW;
    if (must_scale && h && !x.scaled()) return fail(h, RRV_E_ARG, std::string(who) + ": SH, SW must be at least 1");
    return view_run(h, who, d_in, in, d_out, out, flags, hip_stream, x);
}
int rrv_transfer_scaled_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W, void* d_out,
                                    const rrv_image_view* out, int flags, void* hip_stream) {
    return scaled_view_run(h, "transfer_scaled_view", true, d_in, in, B, SH, SW, H, W, 0, 0, d_out, out, flags, hip_stream);
}
// ---- the delivering entries: the stylized working frame resampled to DH x DW behind the last kernel (run_xfer)
// the delivery stage alone, queued on hip_stream itself (NULL: the null stream): nothing of the handle's own streams takes part
int rrv_deliver_view_device(rrv_handle h, const float* d_in, int B, int H, int W, int DH, int DW, void* d_out, const rrv_image_view* out, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!out) return fail(h, RRV_E_ARG, "deliver_view: null view");
    OutFmt fmt;
    if (!view_desc_ok(out->desc) || parse_out(out->desc, &fmt) != DescErr::OK)
        return fail(h, RRV_E_ARG, "deliver_view: out.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (!d_in || !d_out) return fail(h, RRV_E_ARG, "deliver_view: null buffer");
    if (B < 1 || B > 64) return fail(h, RRV_E_ARG, "deliver_view: batch must be in 1..64");
    RCHK(check_deliver(h, "deliver_view", H, W, DH, DW));
    std::string why;
    if (!view_check(*out, B, DH, DW, true, &why)) return fail(h, RRV_E_ARG, "deliver_view: out." + why);
    HIPCHK(hipSetDevice(h->dev));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    return deliver_launch(h, q, d_in, B, H, W, DH, DW, d_out, fmt, img_view(*out));
}
int rrv_transfer_deliver_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W, int DH, int DW,
                                     void* d_out, const rrv_image_view* out, int flags, void* hip_stream) {
    return scaled_view_run(h, "transfer_deliver_view", false, d_in, in, B, SH, SW, H, W, DH, DW, d_out, out, flags, hip_stream);
}
// ---- the guided entries (include/rerevst_hip.h "Guided delivery")
// the stage alone and the equal-size delivery behind it, queued on hip_stream itself (NULL: the null stream): nothing of the handle's own
// streams takes part.  The coefficient planes and Q live in two buffers of the handle that only this entry uses.
int rrv_deliver_guided_view_device(rrv_handle h, const float* d_P, const float* d_guide_lo, const float* d_guide_hi, int B, int H, int W, int DH, int DW, int r,
                                   float eps, void* d_out, const rrv_image_view* out, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!out) return fail(h, RRV_E_ARG, "deliver_guided_view: null view");
    OutFmt fmt;
    if (!view_desc_ok(out->desc) || parse_out(out->desc, &fmt) != DescErr::OK)
        return fail(h, RRV_E_ARG, "deliver_guided_view: out.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (!d_P || !d_guide_lo || !d_guide_hi || !d_out) return fail(h, RRV_E_ARG, "deliver_guided_view: null buffer");
    if (B < 1 || B > 64) return fail(h, RRV_E_ARG, "deliver_guided_view: batch must be in 1..64");
    RCHK(check_guided(h, "deliver_guided_view", H, W, DH, DW, r, eps));
    std::string why;
    if (!view_check(*out, B, DH, DW, true, &why)) return fail(h, RRV_E_ARG, "deliver_guided_view: out." + why);
    HIPCHK(hipSetDevice(h->dev));
    RCHK(gd_tables(h, H, W, DH, DW));
    RCHK(ensure_dev(h, h->gd_ab, h->gd_ab_cap, (size_t)B * H * W * 6));
    RCHK(ensure_dev(h, h->gd_q, h->gd_q_cap, (size_t)B * DH * DW * 3));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    RCHK(guided_launch(h, q, d_P, d_guide_lo, d_guide_hi, B, H, W, DH, DW, r, eps, h->gd_ab, h->gd_q));
    return deliver_launch(h, q, h->gd_q, B, DH, DW, DH, DW, d_out, fmt, img_view(*out));
}
int rrv_transfer_guided_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W, int DH, int DW, int r,
                                    float eps, void* d_out, const rrv_image_view* out, int flags, void* hip_stream) {
    Xfer x{Model::GLOBAL, B, H, W};
    x.SH = SH; x.SW = SW; x.DH = DH; x.DW = DW;
    x.gr = r ? r : -1; x.geps = eps;      // (r = 0 is refused as a radius, not taken for a plain delivery)
    return view_run(h, "transfer_guided_view", d_in, in, d_out, out, flags, hip_stream, x);
}
// ---- the compositing entries (include/rerevst_hip.h "Compositing")
// the stage alone and the equal-size delivery behind it, queued on hip_stream itself (NULL: the null stream): nothing of the handle's own
// streams takes part.  The mixed frame lives in a buffer of the handle that only this entry uses.
int rrv_composite_view_device(rrv_handle h, const float* d_P, const float* d_src, int B, int DH, int DW, const rrv_composite* c, void* d_out,
                              const rrv_image_view* out, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!out) return fail(h, RRV_E_ARG, "composite_view: null view");
    OutFmt fmt;
    if (!view_desc_ok(out->desc) || parse_out(out->desc, &fmt) != DescErr::OK)
        return fail(h, RRV_E_ARG, "composite_view: out.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (!d_P || !d_src || !d_out) return fail(h, RRV_E_ARG, "composite_view: null buffer");
    if (B < 1 || B > 64) return fail(h, RRV_E_ARG, "composite_view: batch must be in 1..64");
    RCHK(check_deliver(h, "composite_view", DH, DW, DH, DW));
    Xfer x{Model::GLOBAL, B, DH, DW};
    static const rrv_composite plain{nullptr, nullptr, RRV_DT_F32, 0, RRV_KEEP_NONE};
    RCHK(set_composite(h, "composite_view", c ? c : &plain, B, &x));      // (the stage alone runs a request that composites nothing too: out = P)
    std::string why;
    if (!view_check(*out, B, DH, DW, true, &why)) return fail(h, RRV_E_ARG, "composite_view: out." + why);
    HIPCHK(hipSetDevice(h->dev));
    const rrv_ctx::RsTab *ty, *tx;
    RCHK(rs_pair(h, DH, DW, DH, DW, &ty, &tx));
    RCHK(ensure_dev(h, h->cm_buf, h->cm_cap, (size_t)B * DH * DW * 3));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    const rrv_composite& r = c ? *c : plain;
    RCHK(composite_launch(h, q, d_P, d_src, B, DH, DW, r.strength, r.matte, r.matte_dtype, r.matte ? r.matte_frames : 0, r.keep, h->cm_buf));
    return deliver_launch(h, q, h->cm_buf, B, DH, DW, DH, DW, d_out, fmt, img_view(*out));
}
int rrv_transfer_composite_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W, int DH, int DW, int r,
                                       float eps, const rrv_composite* c, void* d_out, const rrv_image_view* out, int flags, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    Xfer x{Model::GLOBAL, B, H, W};
    x.SH = SH; x.SW = SW; x.DH = DH; x.DW = DW;
    if (r) { x.gr = r; x.geps = eps; }
    if (B < 1 || B > 64) return fail(h, RRV_E_ARG, "transfer_composite_view: batch must be in 1..64");      // (c->strength holds B values: judged before they are read)
    RCHK(set_composite(h, "transfer_composite_view", c, B, &x));
    return view_run(h, "transfer_composite_view", d_in, in, d_out, out, flags, hip_stream, x);
}
// ---- JPEG output (include/rerevst_hip.h "JPEG output")
int rrv_jpeg_tables(int quality, uint16_t luma[64], uint16_t chroma[64]) {
    if (!luma || !chroma || quality < 1 || quality > 100) return RRV_E_ARG;
    jpeg_tables(quality, luma, chroma);
    return RRV_OK;
}
int rrv_jpeg_bound(int H, int W, int chroma, int restart, size_t* bytes) {
    JpegP p{};
    if (!bytes || !jpeg_plan(H, W, chroma, restart, &p)) return RRV_E_ARG;
    *bytes = jpeg_bound(p);
    return RRV_OK;
}
int rrv_jpeg_plan(int H, int W, int chroma, int restart, int* mcu_cols, int* mcu_rows, int* interval, int* blocks, int* header_bytes) {
    JpegP p{};
    if (!mcu_cols || !mcu_rows || !interval || !blocks || !header_bytes || !jpeg_plan(H, W, chroma, restart, &p)) return RRV_E_ARG;
    *mcu_cols = p.mcu_cols; *mcu_rows = p.mcu_rows; *interval = p.interval; *blocks = p.blocks; *header_bytes = p.header_len;
    return RRV_OK;
}
// the halves alone and together, queued on hip_stream itself (NULL: the null stream): nothing of the handle's own streams takes part
int rrv_jpeg_blocks_device(rrv_handle h, const float* d_in, int B, int H, int W, const rrv_jpeg* j, int16_t* d_coef, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    JpegP p{};
    RCHK(set_jpeg(h, "jpeg_blocks", j, B, H, W, false, 0, &p));
    if (!d_in || !d_coef) return fail(h, RRV_E_ARG, "jpeg_blocks: null buffer");
    if ((uintptr_t)d_coef & 15) return fail(h, RRV_E_ARG, "jpeg_blocks: d_coef must be 16-byte aligned");
    HIPCHK(hipSetDevice(h->dev));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    p.in = d_in; p.coef = d_coef;
    return jpeg_blocks_launch(h, q, p);
}
int rrv_jpeg_entropy_device(rrv_handle h, const int16_t* d_coef, int B, int H, int W, const rrv_jpeg* j, uint8_t* d_out, size_t cap, int* d_sizes, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    JpegP p{};
    RCHK(set_jpeg(h, "jpeg_entropy", j, B, H, W, true, cap, &p));
    if (!d_coef || !d_out || !d_sizes) return fail(h, RRV_E_ARG, "jpeg_entropy: null buffer");
    if ((uintptr_t)d_coef & 15) return fail(h, RRV_E_ARG, "jpeg_entropy: d_coef must be 16-byte aligned");
    HIPCHK(hipSetDevice(h->dev));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    RCHK(ensure_dev(h, h->jp_idx, h->jp_idx_cap, 2 * (size_t)B * p.n_int));
    p.coef = const_cast<int16_t*>(d_coef); p.out = d_out; p.sizes = d_sizes;
    p.lens = h->jp_idx; p.offs = h->jp_idx + (size_t)B * p.n_int;
    return jpeg_entropy_launch(h, q, p);
}
int rrv_jpeg_encode_device(rrv_handle h, const float* d_in, int B, int H, int W, const rrv_jpeg* j, uint8_t* d_out, size_t cap, int* d_sizes, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    JpegP p{};
    RCHK(set_jpeg(h, "jpeg_encode", j, B, H, W, true, cap, &p));
    if (!d_in || !d_out || !d_sizes) return fail(h, RRV_E_ARG, "jpeg_encode: null buffer");
    HIPCHK(hipSetDevice(h->dev));
    // both scratch buffers before the first launch: out of memory leaves nothing queued
    RCHK(ensure_dev(h, h->jp_coef, h->jp_coef_cap, (size_t)B * p.blocks * 64));
    RCHK(ensure_dev(h, h->jp_idx, h->jp_idx_cap, 2 * (size_t)B * p.n_int));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    p.in = d_in; p.coef = h->jp_coef; p.out = d_out; p.sizes = d_sizes;
    p.lens = h->jp_idx; p.offs = h->jp_idx + (size_t)B * p.n_int;
    RCHK(jpeg_blocks_launch(h, q, p));
    return jpeg_entropy_launch(h, q, p);
}
// ---- JPEG input (include/rerevst_hip.h "JPEG input")
static_assert(sizeof(rrv_jpeg_info) == sizeof(JpegInfo) && offsetof(rrv_jpeg_info, scan_offset) == offsetof(JpegInfo, scan_offset) &&
              offsetof(rrv_jpeg_info, q) == offsetof(JpegInfo, q) && offsetof(rrv_jpeg_info, huff_bits) == offsetof(JpegInfo, huff_bits) &&
              offsetof(rrv_jpeg_info, huff_vals) == offsetof(JpegInfo, huff_vals), "rrv_jpeg_info is jpeg_dec.h's JpegInfo");
static_assert(RRV_JPEG_ST_DATA == JD_DATA && RRV_JPEG_ST_CODE == JD_CODE && RRV_JPEG_ST_RUN == JD_RUN && RRV_JPEG_ST_CATEGORY == JD_CATEGORY &&
              RRV_JPEG_ST_MARKER_MISSING == JD_MARKER_MISSING && RRV_JPEG_ST_MARKER_WRONG == JD_MARKER_WRONG && RRV_JPEG_ST_MARKER_SURPLUS == JD_MARKER_SURPLUS,
              "the status codes of the header are the kernels'");
int rrv_jpeg_parse(const uint8_t* stream, size_t size, rrv_jpeg_info* info, char* why, size_t why_len) {
    if (why && why_len) why[0] = 0;
    if (!info) { jpeg_refuse(why, why_len, "null rrv_jpeg_info"); return RRV_E_ARG; }
    if (!stream) { jpeg_refuse(why, why_len, "null stream"); return RRV_E_ARG; }
    return jpeg_parse(stream, size, reinterpret_cast<JpegInfo*>(info), why, why_len) ? RRV_OK : RRV_E_DATA;
}
const char* rrv_jpeg_status_words(int status) { return jpeg_status_words(status); }
// The infos of a call -> the kernels' parameters and the frame descriptors (host), judged before any GPU work.  scan: the call reads streams.
static int set_jpeg_in(rrv_handle h, const char* who, const rrv_jpeg_info* infos, int B, bool scan, size_t cap, JpegDecP* p, std::vector<JpegDecFrame>* frames) {
    const std::string w = std::string(who) + ": ";
    if (B < 1 || B > JP_B_MAX) return fail(h, RRV_E_ARG, w + "batch must be in 1..64");
    if (!infos) return fail(h, RRV_E_ARG, w + "null rrv_jpeg_info array");
    const JpegInfo* const f = reinterpret_cast<const JpegInfo*>(infos);
    if (!jpeg_dec_fill(f[0], p)) return fail(h, RRV_E_ARG, w + "info 0: H, W must be in 1..65535, chroma 400, 420, 422 or 444, interval 0..65535");
    p->B = B; p->cap = cap; p->n_int_max = 1;
    frames->resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const std::string wb = w + "info " + std::to_string(b) + ": ";
        if (f[b].H != f[0].H || f[b].W != f[0].W || f[b].chroma != f[0].chroma)
            return fail(h, RRV_E_ARG, wb + "a " + std::to_string(f[b].H) + " x " + std::to_string(f[b].W) + " frame, chroma " + std::to_string(f[b].chroma) + ", in a call of " +
                                          std::to_string(f[0].H) + " x " + std::to_string(f[0].W) + ", chroma " + std::to_string(f[0].chroma) +
                                          ": the frames of one call share H, W and the chroma format");
        if (!jpeg_dec_frame(f[b], &(*frames)[(size_t)b]))
            return fail(h, RRV_E_ARG, wb + "its fields do not hold together (interval, MCU counts, blocks, intervals, scan bytes below 2^32, Huffman specifications): pass what rrv_jpeg_parse filled");
        if (scan && (f[b].scan_offset > cap || f[b].scan_bytes > cap - f[b].scan_offset))
            return fail(h, RRV_E_ARG, wb + "cap = " + std::to_string(cap) + " bytes is below the frame's size, " + std::to_string(f[b].scan_offset + f[b].scan_bytes));
        p->n_int_max = std::max(p->n_int_max, f[b].intervals);
    }
    return RRV_OK;
}
// the descriptors into the handle's buffer, ordered on the call's stream.  They go through a page-locked buffer of the handle, so the copy is a
// true asynchronous one whatever the runtime does with pageable memory; an event says when the previous call's copy has left that buffer.
static int jpeg_in_upload(rrv_handle h, const Seq& q, const std::vector<JpegDecFrame>& frames, JpegDecP* p) {
    const size_t bytes = frames.size() * sizeof(JpegDecFrame);
    if (h->jd_ev) HIPCHK(hipEventSynchronize(h->jd_ev));
    else HIPCHK(hipEventCreateWithFlags(&h->jd_ev, hipEventDisableTiming));
    if (h->jd_pin_cap < bytes) {
        if (h->jd_pin) (void)hipHostFree(h->jd_pin);
        h->jd_pin = nullptr; h->jd_pin_cap = 0;
        if (hipHostMalloc(&h->jd_pin, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h->jd_pin = nullptr; return fail(h, RRV_E_NOMEM, "jpeg input: out of page-locked host memory for the frame descriptors"); }
        h->jd_pin_cap = bytes;
    }
    memcpy(h->jd_pin, frames.data(), bytes);
    HIPCHK(hipMemcpyAsync(h->jd_frames, h->jd_pin, bytes, hipMemcpyHostToDevice, q.stream));
    HIPCHK(hipEventRecord(h->jd_ev, q.stream));
    p->frames = h->jd_frames;
    p->ivl = h->jd_ivl;
    return RRV_OK;
}
static int jpeg_scan_launch(rrv_handle h, const Seq& q, const JpegDecP& p) {
    int e = 0;
    // for the profile log: the slots read once by each of the two kernels at most, the blocks cleared and written
    RCHK(launch(h, q, "jpeg_scan", 0.0, (2.0 * p.cap + 2.0 * 128.0 * p.blocks) * p.B, [&] { e = rrv_jpeg_scan_launch(&p, q.stream); }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("jpeg_scan: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}
static int jpeg_planes_launch(rrv_handle h, const Seq& q, const JpegDecP& p) {
    int e = 0;
    // for the profile log: the blocks read, the planes written; one multiply per coefficient and the two 8-point passes at 29 operations each per 8 samples
    RCHK(launch(h, q, "jpeg_planes", (1.0 + 2.0 * 29.0 / 8.0) * 64.0 * p.blocks * p.B, (128.0 * p.blocks + (double)p.frame_bytes) * p.B, [&] { e = rrv_jpeg_planes_launch(&p, q.stream); }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("jpeg_planes: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}
int rrv_jpeg_scan_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, int16_t* d_coef, int* d_status, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    JpegDecP p{};
    std::vector<JpegDecFrame> frames;
    RCHK(set_jpeg_in(h, "jpeg_scan", infos, B, true, cap, &p, &frames));
    if (!d_streams || !d_coef) return fail(h, RRV_E_ARG, "jpeg_scan: null buffer");
    if (!d_status) return fail(h, RRV_E_ARG, "jpeg_scan: null d_status");
    if ((uintptr_t)d_coef & 15) return fail(h, RRV_E_ARG, "jpeg_scan: d_coef must be 16-byte aligned");
    HIPCHK(hipSetDevice(h->dev));
    RCHK(ensure_dev(h, h->jd_frames, h->jd_frames_cap, (size_t)B));
    RCHK(ensure_dev(h, h->jd_ivl, h->jd_ivl_cap, (size_t)B * (p.n_int_max + 1)));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    p.streams = d_streams; p.coef = d_coef; p.status = d_status;
    RCHK(jpeg_in_upload(h, q, frames, &p));
    return jpeg_scan_launch(h, q, p);
}
int rrv_jpeg_planes_device(rrv_handle h, const int16_t* d_coef, const rrv_jpeg_info* infos, int B, uint8_t* d_planes, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    JpegDecP p{};
    std::vector<JpegDecFrame> frames;
    RCHK(set_jpeg_in(h, "jpeg_planes", infos, B, false, 0, &p, &frames));
    if (!d_coef || !d_planes) return fail(h, RRV_E_ARG, "jpeg_planes: null buffer");
    if ((uintptr_t)d_coef & 15) return fail(h, RRV_E_ARG, "jpeg_planes: d_coef must be 16-byte aligned");
    HIPCHK(hipSetDevice(h->dev));
    RCHK(ensure_dev(h, h->jd_frames, h->jd_frames_cap, (size_t)B));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    p.coef = const_cast<int16_t*>(d_coef); p.planes = d_planes;
    RCHK(jpeg_in_upload(h, q, frames, &p));
    return jpeg_planes_launch(h, q, p);
}
int rrv_jpeg_decode_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, uint8_t* d_planes, int* d_status, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    JpegDecP p{};
    std::vector<JpegDecFrame> frames;
    RCHK(set_jpeg_in(h, "jpeg_decode", infos, B, true, cap, &p, &frames));
    if (!d_streams || !d_planes) return fail(h, RRV_E_ARG, "jpeg_decode: null buffer");
    if (!d_status) return fail(h, RRV_E_ARG, "jpeg_decode: null d_status");
    HIPCHK(hipSetDevice(h->dev));
    // every scratch buffer before the first launch: out of memory leaves nothing queued
    RCHK(ensure_dev(h, h->jd_frames, h->jd_frames_cap, (size_t)B));
    RCHK(ensure_dev(h, h->jd_ivl, h->jd_ivl_cap, (size_t)B * (p.n_int_max + 1)));
    RCHK(ensure_dev(h, h->jd_coef, h->jd_coef_cap, (size_t)B * p.blocks * 64));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    p.streams = d_streams; p.coef = h->jd_coef; p.planes = d_planes; p.status = d_status;
    RCHK(jpeg_in_upload(h, q, frames, &p));
    RCHK(jpeg_scan_launch(h, q, p));
    return jpeg_planes_launch(h, q, p);
}
// ---- transfers whose INPUT form is JPEG: the decode stage in front of the compositing view entry (or its JPEG-out twin), which reads the planes
// as the 8-bit I420 / I422 / I444 frames they are.  JFIF's colour space is BT.601 full range whatever matrix the handle holds: the handle's
// matrix is put aside while the entry queues its launches (a launch keeps the matrix it was queued with) and put back on every way out.
struct JfifMatrix {
    rrv_handle h; float keep[12];
    explicit JfifMatrix(rrv_handle h_) : h(h_) { memcpy(keep, h->yuv_in.m8, sizeof keep); (void)rrv_yuv_input_matrix(RRV_YUV_BT601, 1, h->yuv_in.m8); }
    ~JfifMatrix() { memcpy(h->yuv_in.m8, keep, sizeof keep); }
};
// A from-JPEG call in two steps, so that every check of the decode AND of the transfer behind it runs before anything is queued:
// jpeg_in_check judges the decode's arguments and builds the frame descriptors on the host, jpeg_in_queue reserves the scratch and queues the
// decode of the B streams into the handle's planes buffer on `stream`.
struct JpegInCall { JpegDecP p{}; std::vector<JpegDecFrame> frames; rrv_image_view vin{}; };
static int jpeg_in_check(rrv_handle h, const char* who, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, const int* d_status, JpegInCall* k) {
    RCHK(set_jpeg_in(h, who, infos, B, true, cap, &k->p, &k->frames));
    if (!d_streams) return fail(h, RRV_E_ARG, std::string(who) + ": null buffer");
    if (!d_status) return fail(h, RRV_E_ARG, std::string(who) + ": null d_status");
    if (k->p.H < 8 || k->p.W < 8) return fail(h, RRV_E_ARG, std::string(who) + ": frames must be at least 8 x 8 pixels");
    const int lay = k->p.ncomp == 1 || (k->p.hs == 1 && k->p.vs == 1) ? RRV_LAY_I444 : k->p.vs == 2 ? RRV_LAY_I420 : RRV_LAY_I422;
    k->vin = contiguous_of(rrv_image_desc{RRV_DT_U8, lay, RRV_SP_PIXEL}, k->p.H, k->p.W);
    return RRV_OK;
}
static int jpeg_in_queue(rrv_handle h, JpegInCall& k, const uint8_t* d_streams, int* d_status, hipStream_t stream) {
    JpegDecP& p = k.p;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(ensure_dev(h, h->jd_frames, h->jd_frames_cap, (size_t)p.B));
    RCHK(ensure_dev(h, h->jd_ivl, h->jd_ivl_cap, (size_t)p.B * (p.n_int_max + 1)));
    RCHK(ensure_dev(h, h->jd_coef, h->jd_coef_cap, (size_t)p.B * p.blocks * 64));
    RCHK(ensure_dev(h, h->jd_planes, h->jd_planes_cap, (size_t)p.B * p.frame_bytes));
    Seq q = base_seq(h);
    q.stream = stream;
    p.streams = d_streams; p.coef = h->jd_coef; p.planes = h->jd_planes; p.status = d_status;
    RCHK(jpeg_in_upload(h, q, k.frames, &p));
    RCHK(jpeg_scan_launch(h, q, p));
    return jpeg_planes_launch(h, q, p);
}
// the sizes of a from-JPEG request: a working size of 0 x 0 is the source's
static void jpeg_in_sizes(const rrv_jpeg_info* infos, int work_H, int work_W, int* SH, int* SW, int* H, int* W) {
    const bool scaled = work_H != 0 || work_W != 0;
    *SH = scaled ? infos[0].H : 0; *SW = scaled ? infos[0].W : 0;
    *H = scaled ? work_H : infos[0].H; *W = scaled ? work_W : infos[0].W;
}
// The checks the transfer behind the decode will make (those of rrv_transfer_composite_view_device / rrv_transfer_jpeg_view_device through view_run),
// made here on the same request before the decode is queued: nothing has run when one of them refuses.  out: the output view, or null with j
// (JPEG out).  *ox receives the request (its OH(), OW(), out_bytes()).
static int jpeg_in_precheck(rrv_handle h, const char* who, const JpegInCall& k, const rrv_jpeg_info* infos, int B, int work_H, int work_W, int DH, int DW, int r,
                            float eps, const rrv_composite* c, const rrv_image_view* out, const rrv_jpeg* j, size_t out_cap, int flags, bool host, Xfer* ox) {
    const std::string w = std::string(who) + ": ";
    Xfer x{Model::GLOBAL, B, 0, 0};
    jpeg_in_sizes(infos, work_H, work_W, &x.SH, &x.SW, &x.H, &x.W);
    x.DH = DH; x.DW = DW;
    if (r) { x.gr = r; x.geps = eps; }
    RCHK(set_composite(h, who, c, B, &x));
    if (flags & ~(RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE | (host ? 0 : RRV_TF_ON_STREAM))) return fail(h, RRV_E_ARG, w + "unknown flags");
    x.pad = (flags & RRV_TF_PAD_CROP) != 0;
    if (flags & RRV_TF_FRAME_MODE) x.model = Model::FRAME;
    if (!parse_in_view(k.vin.desc, &x.in)) return fail(h, RRV_E_ARG, w + "the decoded layout is not an input form");
    if (out && (!view_desc_ok(out->desc) || parse_out(out->desc, &x.fmt) != DescErr::OK))
        return fail(h, RRV_E_ARG, w + "out.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (j) {
        JpegP jp{};
        RCHK(set_jpeg(h, who, j, 1, x.OH(), x.OW(), true, out_cap, &jp));
    }
    HIPCHK(hipSetDevice(h->dev));
    RCHK(check_xfer(h, x));
    std::string why;
    if (out && !view_check(*out, B, x.OH(), x.OW(), true, &why)) return fail(h, RRV_E_ARG, w + "out." + why);
    *ox = x;
    return RRV_OK;
}
int rrv_transfer_from_jpeg_view_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, int work_H, int work_W, int DH,
                                       int DW, int r, float eps, const rrv_composite* c, void* d_out, const rrv_image_view* out, int* d_status, int flags,
                                       void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!d_out || !out) return fail(h, RRV_E_ARG, "transfer_from_jpeg_view: null output buffer or view");
    JpegInCall k;
    Xfer x{Model::GLOBAL, B, 0, 0};
    RCHK(jpeg_in_check(h, "transfer_from_jpeg_view", d_streams, cap, infos, B, d_status, &k));
    RCHK(jpeg_in_precheck(h, "transfer_from_jpeg_view", k, infos, B, work_H, work_W, DH, DW, r, eps, c, out, nullptr, 0, flags, false, &x));
    RCHK(jpeg_in_queue(h, k, d_streams, d_status, (hipStream_t)hip_stream));
    const JfifMatrix jfif(h);
    return rrv_transfer_composite_view_device(h, h->jd_planes, &k.vin, B, x.SH, x.SW, x.H, x.W, DH, DW, r, eps, c, d_out, out, flags | RRV_TF_ON_STREAM, hip_stream);
}
int rrv_transfer_jpeg_from_jpeg_view_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, int work_H, int work_W,
                                            int DH, int DW, int r, float eps, const rrv_composite* c, const rrv_jpeg* j, uint8_t* d_out, size_t out_cap,
                                            int* d_sizes, int* d_status, int flags, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!d_out || !d_sizes || !j) return fail(h, RRV_E_ARG, "transfer_jpeg_from_jpeg_view: null output buffer, sizes or rrv_jpeg");
    JpegInCall k;
    Xfer x{Model::GLOBAL, B, 0, 0};
    RCHK(jpeg_in_check(h, "transfer_jpeg_from_jpeg_view", d_streams, cap, infos, B, d_status, &k));
    RCHK(jpeg_in_precheck(h, "transfer_jpeg_from_jpeg_view", k, infos, B, work_H, work_W, DH, DW, r, eps, c, nullptr, j, out_cap, flags, false, &x));
    RCHK(jpeg_in_queue(h, k, d_streams, d_status, (hipStream_t)hip_stream));
    const JfifMatrix jfif(h);
    return rrv_transfer_jpeg_view_device(h, h->jd_planes, &k.vin, B, x.SH, x.SW, x.H, x.W, DH, DW, r, eps, c, j, d_out, out_cap, d_sizes, flags | RRV_TF_ON_STREAM,
                                         hip_stream);
}
// The host twins: every stream parsed on the host first (a refusal is RRV_E_DATA naming the frame), then sub-batches of up to sixteen frames on
// the handle's first stream: each frame's own bytes up, the device entry, the statuses and the output back.  One sub-batch at a time: simple, and
// not the pipeline of the other host entries.  A corrupt frame is RRV_E_DATA naming it; the frames before its sub-batch have been written.
constexpr int JPEG_IN_SUB = 16;
// `before` makes the transfer's own checks on the first sub-batch's request once the streams are parsed: nothing has been copied or queued then.
static int jpeg_in_host(rrv_handle h, const char* who, const uint8_t* const* streams, const size_t* sizes, int B, std::vector<JpegInfo>* infos, size_t* cap,
                        const std::function<int(int)>& before, const std::function<int(int, int, hipStream_t)>& run) {
    const std::string w = std::string(who) + ": ";
    if (B < 1) return fail(h, RRV_E_ARG, w + "batch must be at least 1");
    if (!streams || !sizes) return fail(h, RRV_E_ARG, w + "null streams or sizes");
    infos->resize((size_t)B);
    size_t most = 0;
    for (int b = 0; b < B; ++b) {
        char why[200];
        if (!streams[b]) return fail(h, RRV_E_ARG, w + "stream " + std::to_string(b) + " is null");
        if (!jpeg_parse(streams[b], sizes[b], &(*infos)[(size_t)b], why, sizeof why)) return fail(h, RRV_E_DATA, w + "frame " + std::to_string(b) + ": " + why);
        const JpegInfo &f = (*infos)[(size_t)b], &f0 = (*infos)[0];
        if (f.H != f0.H || f.W != f0.W || f.chroma != f0.chroma)
            return fail(h, RRV_E_ARG, w + "frame " + std::to_string(b) + " is " + std::to_string(f.H) + " x " + std::to_string(f.W) + ", chroma " + std::to_string(f.chroma) +
                                          "; frame 0 is " + std::to_string(f0.H) + " x " + std::to_string(f0.W) + ", chroma " + std::to_string(f0.chroma) +
                                          ": the frames of one call share H, W and the chroma format");
        most = std::max(most, sizes[b]);
    }
    *cap = (most + 15) & ~(size_t)15;
    const int sub = std::min(B, JPEG_IN_SUB);
    RCHK(before(sub));
    HIPCHK(hipSetDevice(h->dev));
    const hipStream_t s = h->slots[0].stream;
    RCHK(ensure_dev(h, h->jd_streams, h->jd_streams_cap, (size_t)sub * *cap));
    RCHK(ensure_dev(h, h->jd_status, h->jd_status_cap, (size_t)sub));
    for (int b0 = 0; b0 < B; b0 += sub) {
        const int nb = std::min(sub, B - b0);
        for (int b = 0; b < nb; ++b) HIPCHK(hipMemcpyAsync(h->jd_streams + (size_t)b * *cap, streams[b0 + b], sizes[b0 + b], hipMemcpyHostToDevice, s));
        int rc = run(b0, nb, s);
        int st[JPEG_IN_SUB] = {0};
        if (rc == RRV_OK) {
            HIPCHK(hipMemcpyAsync(st, h->jd_status, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int b = 0; b < nb; ++b)
                if (st[b] != JD_OK) return fail(h, RRV_E_DATA, w + "frame " + std::to_string(b0 + b) + " is corrupt: " + jpeg_status_words(st[b]));
        } else {
            (void)hipStreamSynchronize(s);      // (the caller's streams are not read after the call returns)
            return rc;
        }
    }
    return RRV_OK;
}
// the checks of a host twin's first sub-batch (jpeg_in_check, jpeg_in_precheck) on host pointers that are only tested for null
static int jpeg_in_host_precheck(rrv_handle h, const char* who, const uint8_t* const* streams, size_t cap, const std::vector<JpegInfo>& infos, int nb, int work_H,
                                 int work_W, int DH, int DW, int r, float eps, const rrv_composite* c, const rrv_image_desc* od, const rrv_jpeg* j, size_t out_cap,
                                 int flags, Xfer* x) {
    const rrv_jpeg_info* const in = reinterpret_cast<const rrv_jpeg_info*>(infos.data());
    JpegInCall k;
    int dummy = 0;
    RCHK(jpeg_in_check(h, who, streams[0], cap, in, nb, &dummy, &k));
    rrv_composite part{};
    if (c) { part = *c; if (c->matte && c->matte_frames != 1) part.matte_frames = nb; }
    rrv_image_view vo{};
    if (od) {      // (the view's geometry follows from the request; only the descriptor can be wrong)
        vo.desc = *od;
        OutFmt f;
        if (!view_desc_ok(*od) || parse_out(*od, &f) != DescErr::OK)
            return fail(h, RRV_E_ARG, std::string(who) + ": out is not a dtype, layout and space combination the descriptor entries accept");
    }
    RCHK(jpeg_in_precheck(h, who, k, in, nb, work_H, work_W, DH, DW, r, eps, c ? &part : nullptr, nullptr, j, out_cap, flags, true, x));
    if (od && parse_out(*od, &x->fmt) != DescErr::OK) return fail(h, RRV_E_ARG, std::string(who) + ": out descriptor");
    return RRV_OK;
}
// a host matte of sub-batch [b0, b0 + nb) in HBM, and the request that names it
static int jpeg_in_request(rrv_handle h, const rrv_composite* c, int b0, int nb, size_t frame_px, hipStream_t s, rrv_composite* part) {
    if (!c) return RRV_OK;
    *part = *c;
    if (c->strength) part->strength = c->strength + b0;
    if (c->matte) {
        const size_t mfb = frame_px * (c->matte_dtype == RRV_DT_U8 ? 1 : 4);
        const int frames = c->matte_frames == 1 ? 1 : nb;
        RCHK(ensure_dev(h, h->jd_matte, h->jd_matte_cap, (size_t)frames * mfb));
        HIPCHK(hipMemcpyAsync(h->jd_matte, (const uint8_t*)c->matte + (c->matte_frames == 1 ? 0 : (size_t)b0 * mfb), (size_t)frames * mfb, hipMemcpyHostToDevice, s));
        part->matte = h->jd_matte; part->matte_frames = frames;
    }
    return RRV_OK;
}
int rrv_transfer_from_jpeg(rrv_handle h, const uint8_t* const* streams, const size_t* sizes, int B, int work_H, int work_W, int DH, int DW, int r, float eps,
                           const rrv_composite* c, void* out, rrv_image_desc od, int flags) {
    if (!h) return RRV_E_ARG;
    if (!out) return fail(h, RRV_E_ARG, "transfer_from_jpeg: null buffer");
    if (flags & ~(RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE)) return fail(h, RRV_E_ARG, "transfer_from_jpeg: unknown flags");
    std::vector<JpegInfo> infos;
    size_t cap = 0, ob = 0, opx = 0;
    rrv_image_view vo{};
    return jpeg_in_host(h, "transfer_from_jpeg", streams, sizes, B, &infos, &cap, [&](int sub) -> int {
        Xfer x{Model::GLOBAL, sub, 0, 0};
        RCHK(jpeg_in_host_precheck(h, "transfer_from_jpeg", streams, cap, infos, sub, work_H, work_W, DH, DW, r, eps, c, &od, nullptr, 0, flags, &x));
        vo = contiguous_of(od, x.OH(), x.OW());      // the delivered frame, from the first stream's size
        ob = x.out_bytes(); opx = (size_t)x.OH() * x.OW();
        return ensure_dev(h, h->jd_out, h->jd_out_cap, (size_t)sub * ob);
    }, [&](int b0, int nb, hipStream_t s) -> int {
        const rrv_jpeg_info* const in = reinterpret_cast<const rrv_jpeg_info*>(infos.data()) + b0;
        rrv_composite part{};
        RCHK(jpeg_in_request(h, c, b0, nb, opx, s, &part));
        RCHK(rrv_transfer_from_jpeg_view_device(h, h->jd_streams, cap, in, nb, work_H, work_W, DH, DW, r, eps, c ? &part : nullptr, h->jd_out, &vo, h->jd_status, flags, s));
        HIPCHK(hipMemcpyAsync((uint8_t*)out + (size_t)b0 * ob, h->jd_out, (size_t)nb * ob, hipMemcpyDeviceToHost, s));
        return RRV_OK;
    });
}
int rrv_transfer_jpeg_from_jpeg(rrv_handle h, const uint8_t* const* streams, const size_t* sizes, int B, int work_H, int work_W, int DH, int DW, int r, float eps,
                                const rrv_composite* c, const rrv_jpeg* j, uint8_t* out, size_t out_cap, int* out_sizes, int flags) {
    if (!h) return RRV_E_ARG;
    if (!out || !out_sizes || !j) return fail(h, RRV_E_ARG, "transfer_jpeg_from_jpeg: null buffer, sizes or rrv_jpeg");
    if (flags & ~(RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE)) return fail(h, RRV_E_ARG, "transfer_jpeg_from_jpeg: unknown flags");
    if (c && c->matte) return fail(h, RRV_E_ARG, "transfer_jpeg_from_jpeg: a matte is not taken by this host entry (the device entry takes one)");
    std::vector<JpegInfo> infos;
    size_t cap = 0;
    const size_t sizes_at = ((size_t)JPEG_IN_SUB * out_cap + 15) & ~(size_t)15;
    return jpeg_in_host(h, "transfer_jpeg_from_jpeg", streams, sizes, B, &infos, &cap, [&](int sub) -> int {
        Xfer x{Model::GLOBAL, sub, 0, 0};
        RCHK(jpeg_in_host_precheck(h, "transfer_jpeg_from_jpeg", streams, cap, infos, sub, work_H, work_W, DH, DW, r, eps, c, nullptr, j, out_cap, flags, &x));
        return ensure_dev(h, h->jd_out, h->jd_out_cap, sizes_at + JPEG_IN_SUB * sizeof(int));
    }, [&](int b0, int nb, hipStream_t s) -> int {
        const rrv_jpeg_info* const in = reinterpret_cast<const rrv_jpeg_info*>(infos.data()) + b0;
        rrv_composite part{};
        RCHK(jpeg_in_request(h, c, b0, nb, 0, s, &part));
        int* const d_sizes = reinterpret_cast<int*>(h->jd_out + sizes_at);
        RCHK(rrv_transfer_jpeg_from_jpeg_view_device(h, h->jd_streams, cap, in, nb, work_H, work_W, DH, DW, r, eps, c ? &part : nullptr, j, h->jd_out, out_cap, d_sizes,
                                                     h->jd_status, flags, s));
        HIPCHK(hipMemcpyAsync(out_sizes + b0, d_sizes, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int b = 0; b < nb; ++b)
            if (out_sizes[b0 + b] > 0)
                HIPCHK(hipMemcpyAsync(out + (size_t)(b0 + b) * out_cap, h->jd_out + (size_t)b * out_cap, (size_t)out_sizes[b0 + b], hipMemcpyDeviceToHost, s));
        return RRV_OK;
    });
}
static bool parse_in_host(const rrv_image_desc& d, InFmt* in);
// a transfer whose output form is JPEG: the request of rrv_transfer_composite_view_device with the encoder behind it
static int jpeg_xfer(rrv_handle h, const char* who, int B, int SH, int SW, int H, int W, int DH, int DW, int r, float eps, const rrv_composite* c, int flags,
                     const rrv_jpeg* j, size_t cap, int max_B, Xfer* x, JpegP* p) {
    *x = Xfer{Model::GLOBAL, B, H, W};
    x->SH = SH; x->SW = SW; x->DH = DH; x->DW = DW;
    if (r) { x->gr = r; x->geps = eps; }
    if (B < 1 || (max_B && B > max_B)) return fail(h, RRV_E_ARG, std::string(who) + (max_B ? ": batch must be in 1..64" : ": batch must be at least 1"));
    RCHK(set_composite(h, who, c, B, x));
    if (flags & ~(RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE | RRV_TF_ON_STREAM)) return fail(h, RRV_E_ARG, std::string(who) + ": unknown flags");
    x->pad = (flags & RRV_TF_PAD_CROP) != 0;
    RCHK(set_jpeg(h, who, j, 1, x->OH(), x->OW(), true, cap, p));      // (the delivered frame; the batch is judged above, and per launch group later)
    x->jp = p;
    return RRV_OK;
}
int rrv_transfer_jpeg_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W, int DH, int DW, int r,
                                  float eps, const rrv_composite* c, const rrv_jpeg* j, uint8_t* d_out, size_t cap, int* d_sizes, int flags, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    Xfer x{Model::GLOBAL, B, H, W};
    JpegP p{};
    RCHK(jpeg_xfer(h, "transfer_jpeg_view", B, SH, SW, H, W, DH, DW, r, eps, c, flags, j, cap, 64, &x, &p));
    if (!d_sizes) return fail(h, RRV_E_ARG, "transfer_jpeg_view: null buffer");
    x.jp_sizes = d_sizes;
    // The checks of the view entries run on a stand-in for the output view: the float32 frame the encoder reads, which lives in the slot.
    // d_out is NOT a buffer of that view: it holds B slots of cap bytes, and run_xfer never addresses it through the view (Xfer::jp).  view_run
    // judges an output view by its own geometry only; a check that relates d_out to the view has to skip a request with x.jp set.
    const rrv_image_view vo = contiguous_of(rrv_image_desc{RRV_DT_F32, RRV_LAY_HWC_BGR, RRV_SP_PIXEL}, x.OH(), x.OW());
    return view_run(h, "transfer_jpeg_view", d_in, in, d_out, &vo, flags, hip_stream, x);
}
// The host twin.  Sub-batch k runs on compute slot k & 1 with staging set k & 1: frames up, the request, the sizes to the host.  Once sub-batch
// k + 1 is queued the host waits for k, reads its sizes and copies sizes[b] bytes of every frame that fitted, while the GPU runs k + 1.
int rrv_transfer_jpeg(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W, int DH, int DW, int r, float eps,
                      const rrv_composite* c, const rrv_jpeg* j, uint8_t* out, size_t cap, int* sizes, int flags) {
    if (!h) return RRV_E_ARG;
    Xfer x{Model::GLOBAL, B, H, W};
    JpegP p{};
    RCHK(jpeg_xfer(h, "transfer_jpeg", B, SH, SW, H, W, DH, DW, r, eps, c, flags & ~RRV_TF_ON_STREAM, j, cap, 0, &x, &p));
    if (flags & RRV_TF_ON_STREAM) return fail(h, RRV_E_ARG, "transfer_jpeg: unknown flags");
    if (!frames || !out || !sizes) return fail(h, RRV_E_ARG, "transfer_jpeg: null buffer");
    if (!parse_in_host(in, &x.in)) return fail(h, RRV_E_ARG, "transfer_jpeg: the input is uint8 HWC BGR or a YUV layout with its own sample type, in the PIXEL space");
    if (flags & RRV_TF_FRAME_MODE) x.model = Model::FRAME;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(check_xfer(h, x, true));
    int sub = std::min(host_sub(B, x.KH(), x.KW()), 64);
    if (x.scaled()) sub = (int)std::max(1L, std::min((long)sub, 4 * HOST_SUB_PIXELS / ((long)x.SH * x.SW)));
    sub = (int)std::max(1L, std::min((long)sub, 4 * HOST_SUB_PIXELS / ((long)x.OH() * x.OW())));
    RCHK(claim_staging(h));
    const size_t fb = x.in_bytes(), sizes_at = ((size_t)sub * cap + 15) & ~(size_t)15, mfb = x.matte_bytes();
    const int nchunk = (B + sub - 1) / sub;
    auto slot_of = [&](int k) { return h->profiling ? 0 : (k & 1) % h->n_slots; };
    // everything either slot and either staging set allocates, before the first launch
    for (int k = 0; k < std::min(nchunk, 2); ++k) {
        RCHK(reserve_stages(h, slot_of(k), x.model == Model::GLOBAL ? sub : std::min(sub, (int)rrv_ctx::MS_GROUP_MAX), x));
        RCHK(stage_reserve(h, k, (size_t)sub * fb, sizes_at + (size_t)sub * sizeof(int), false));
        RCHK(stage_reserve(h, k, 0, (size_t)sub * sizeof(int), true));      // the sizes land page-locked: their copy must not hold the host
        if (x.cmatte) RCHK(ensure_dev(h, h->hstage[k].mask, h->hstage[k].mask_cap, ((size_t)(x.cm_frames == 1 ? 1 : sub) * mfb + 3) / 4));
    }
    auto count = [&](int k) { return std::min(sub, B - k * sub); };
    auto finish = [&](int k) -> int {      // sub-batch k's sizes, then its bytes
        rrv_ctx::HostStage& st = h->hstage[k & 1];
        const hipStream_t cs = h->slots[slot_of(k)].stream;
        const int b0 = k * sub, nb = count(k);
        HIPCHK(hipStreamSynchronize(cs));      // (the sizes have arrived with it)
        memcpy(sizes + b0, st.pin.out, (size_t)nb * sizeof(int));
        for (int b = 0; b < nb; ++b)
            if (sizes[b0 + b] > 0)
                HIPCHK(hipMemcpyAsync(out + (size_t)(b0 + b) * cap, (const uint8_t*)st.dev.out + (size_t)b * cap, (size_t)sizes[b0 + b], hipMemcpyDeviceToHost, cs));
        HIPCHK(hipStreamSynchronize(cs));
        return RRV_OK;
    };
    auto pipeline = [&]() -> int {      // (a lambda so that every way out, the HIP checks' included, passes the one exit below)
    for (int k = 0; k < nchunk; ++k) {
        rrv_ctx::HostStage& st = h->hstage[k & 1];      // (free again: finish(k - 2) has run)
        const int slot = slot_of(k), b0 = k * sub, nb = count(k);
        const hipStream_t cs = h->slots[slot].stream;
        HIPCHK(hipMemcpyAsync(st.dev.in, (const uint8_t*)frames + (size_t)b0 * fb, (size_t)nb * fb, hipMemcpyHostToDevice, cs));
        Xfer part = x;
        part.B = nb;
        if (x.cstr) part.cstr = x.cstr + b0;
        if (x.cmatte) {
            const char* const m = (const char*)x.cmatte + (x.cm_frames == 1 ? 0 : (size_t)b0 * mfb);
            HIPCHK(hipMemcpyAsync(st.mask, m, (size_t)(x.cm_frames == 1 ? 1 : nb) * mfb, hipMemcpyHostToDevice, cs));
            part.cmatte = st.mask; part.cm_frames = x.cm_frames == 1 ? 1 : nb;
        }
        int* const d_sizes = (int*)((char*)st.dev.out + sizes_at);
        part.jp_sizes = d_sizes;
        RCHK(run_xfer(h, slot, st.dev.in, st.dev.out, part));
        HIPCHK(hipMemcpyAsync(st.pin.out, d_sizes, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, cs));
        if (k > 0) RCHK(finish(k - 1));
    }
    return finish(nchunk - 1);
    };
    const int rc = pipeline();
    if (rc != RRV_OK) (void)sync_all(h);      // nothing of a failed call is left in flight on the staging sets
    return rc;
}
// a host frame format of the scaled host entries: uint8 HWC BGR, or any YUV layout with its own dtype
static bool parse_in_host(const rrv_image_desc& d, InFmt* in) {
    if (yuv_layout(d.layout)) return parse_in_view(d, in);
    if (d.dtype != RRV_DT_U8 || d.layout != RRV_LAY_HWC_BGR || d.space != RRV_SP_PIXEL) return false;
    *in = IN_BGR8;
    return true;
}
// the scaled host entries: SH x SW frames in the format `in`, through desc_host
static int scaled_host(rrv_handle h, const char* family, bool must_scale, const void* frames, rrv_image_desc in, void* out, rrv_image_desc od, int flags, Xfer x) {
    if (!h) return RRV_E_ARG;
    if (!parse_in_host(in, &x.in))
        return fail(h, RRV_E_ARG, std::string(family) + ": the input is uint8 HWC BGR or a YUV layout with its own sample type, in the PIXEL space");
    return desc_host(h, family, (const uint8_t*)frames, out, od, flags, RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE,
                     must_scale && !x.scaled() ? "SH, SW must be at least 1" : nullptr, x);
}
int rrv_transfer_scaled(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W, void* out, rrv_image_desc od, int flags) {
    Xfer x{Model::GLOBAL, B, H, W};
    x.SH = SH; x.SW = SW;
    return scaled_host(h, "transfer_scaled", true, frames, in, out, od, flags, x);
}
int rrv_transfer_deliver(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W, int DH, int DW, void* out,
                         rrv_image_desc od, int flags) {
    Xfer x{Model::GLOBAL, B, H, W};
    x.SH = SH; x.SW = SW; x.DH = DH; x.DW = DW;
    return scaled_host(h, "transfer_deliver", false, frames, in, out, od, flags, x);
}
int rrv_transfer_guided(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W, int DH, int DW, int r, float eps, void* out,
                        rrv_image_desc od, int flags) {
    Xfer x{Model::GLOBAL, B, H, W};
    x.SH = SH; x.SW = SW; x.DH = DH; x.DW = DW;
    x.gr = r ? r : -1; x.geps = eps;
    return scaled_host(h, "transfer_guided", false, frames, in, out, od, flags, x);
}
int rrv_transfer_composite(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W, int DH, int DW, int r, float eps,
                           const rrv_composite* c, void* out, rrv_image_desc od, int flags) {
    if (!h) return RRV_E_ARG;
    Xfer x{Model::GLOBAL, B, H, W};
    x.SH = SH; x.SW = SW; x.DH = DH; x.DW = DW;
    if (r) { x.gr = r; x.geps = eps; }
    if (B < 1) return fail(h, RRV_E_ARG, "transfer_composite: batch must be at least 1");
    RCHK(set_composite(h, "transfer_composite", c, B, &x));
    return scaled_host(h, "transfer_composite", false, frames, in, out, od, flags, x);
}
// a sampled frame of SH x SW, resampled into slot 0's buffer on the handle's stream and added as the float32 PIXEL frame it then is.
// device: d_frame is in HBM, complete once `stream` has run what it holds now; else host memory in the contiguous form of `fmt`
// host_bytes: what a host frame uploads when `view` is a window of a larger frame (0: the contiguous SH x SW frame)
static int add_scaled(rrv_handle h, const void* frame, bool device, InFmt fmt, const rrv_image_view* view, hipStream_t stream, int SH, int SW, int H, int W,
                      size_t host_bytes = 0) {
    RCHK(check_frame(h, H, W, "add"));
    RCHK(check_scale(h, "add_scaled", SH, SW, H, W));
    std::string why;
    if (view && !view_check(*view, 1, SH, SW, false, &why)) return fail(h, RRV_E_ARG, "add_scaled: in." + why);
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    if ((!h->patches.empty() || h->pend_n) && (H != h->add_H || W != h->add_W))      // add_frame's rule, judged here before any GPU work
        return fail(h, RRV_E_ARG, "add: all sampled frames must have the same size");
    HIPCHK(hipSetDevice(h->dev));
    RCHK(rs_reserve(h, 0, 1, SH, SW, H, W));
    const Seq q = base_seq(h);
    const void* src = frame;
    if (device) {
        RCHK(wait_for_stream(h, stream));
    } else {
        const size_t fb = host_bytes ? host_bytes : in_frame_bytes(fmt.form, SH, SW, fmt.cs);
        RCHK(ensure_dev(h, h->d_u8, h->d_u8_cap, fb));
        HIPCHK(hipMemcpyAsync(h->d_u8, frame, fb, hipMemcpyHostToDevice, q.stream));
        src = h->d_u8;
    }
    const ImgView vi = view ? img_view(*view) : contiguous_view(in_view_layout(fmt.form), SH, SW, fmt.cs);
    const int rc = resample_launch(h, q, src, fmt, vi, 1, SH, SW, H, W, h->slots[0].rs_buf);
    if (rc != RRV_OK) { (void)hipStreamSynchronize(q.stream); return rc; }      // (the caller's frame is not read after the call returns)
    return add_frame(h, h->slots[0].rs_buf, true, InFmt{IN_F32_HWC, SP_PIXEL}, q.stream, H, W);      // (synchronises: the frame has been read and compacted)
}
// a sampled frame that is a JPEG stream: parsed here, decoded on the handle's stream into the planes buffer and added as the float32 PIXEL frame
// the resampler makes of the planes with JFIF's matrix (at the stream's own size when work_H = work_W = 0: every tap weight is then 1)
int rrv_add_from_jpeg(rrv_handle h, const uint8_t* stream, size_t size, int work_H, int work_W) {
    if (!h) return RRV_E_ARG;
    if (!stream) return fail(h, RRV_E_ARG, "add_from_jpeg: null stream");
    JpegInfo info;
    char why[200];
    if (!jpeg_parse(stream, size, &info, why, sizeof why)) return fail(h, RRV_E_DATA, std::string("add_from_jpeg: ") + why);
    HIPCHK(hipSetDevice(h->dev));
    const size_t cap = (size + 15) & ~(size_t)15;
    RCHK(ensure_dev(h, h->jd_streams, h->jd_streams_cap, cap));
    RCHK(ensure_dev(h, h->jd_status, h->jd_status_cap, 1));
    const hipStream_t s = h->slots[0].stream;
    HIPCHK(hipMemcpyAsync(h->jd_streams, stream, size, hipMemcpyHostToDevice, s));
    JpegInCall k;
    int rc = jpeg_in_check(h, "add_from_jpeg", h->jd_streams, cap, reinterpret_cast<const rrv_jpeg_info*>(&info), 1, h->jd_status, &k);
    if (rc == RRV_OK) rc = jpeg_in_queue(h, k, h->jd_streams, h->jd_status, s);
    const rrv_image_view& vin = k.vin;
    int st = 0;
    if (rc == RRV_OK) {
        HIPCHK(hipMemcpyAsync(&st, h->jd_status, sizeof st, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (st != JD_OK) return fail(h, RRV_E_DATA, std::string("add_from_jpeg: the frame is corrupt: ") + jpeg_status_words(st));
    } else {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    InFmt fmt;
    if (!parse_in_view(vin.desc, &fmt)) return fail(h, RRV_E_ARG, "add_from_jpeg: the decoded layout is not an input form");
    const bool scaled = work_H != 0 || work_W != 0;
    const JfifMatrix jfif(h);
    return add_scaled(h, h->jd_planes, true, fmt, &vin, s, info.H, info.W, scaled ? work_H : info.H, scaled ? work_W : info.W);
}
int rrv_add_scaled_view_device(rrv_handle h, const void* d_frame, const rrv_image_view* in, int SH, int SW, int H, int W, void* hip_stream) {
    if (!h || !d_frame || !in) return RRV_E_ARG;
    InFmt fmt;
    if (!parse_in_view(in->desc, &fmt)) return fail(h, RRV_E_ARG, "add_scaled_view: in.desc is not a dtype, layout and space combination the descriptor entries accept");
    return add_scaled(h, d_frame, true, fmt, in, (hipStream_t)hip_stream, SH, SW, H, W);
}
int rrv_add_scaled(rrv_handle h, const void* frame, rrv_image_desc in, int SH, int SW, int H, int W) {
    if (!h || !frame) return RRV_E_ARG;
    InFmt fmt;
    if (!parse_in_host(in, &fmt)) return fail(h, RRV_E_ARG, "add_scaled: the input is uint8 HWC BGR or a YUV layout with its own sample type, in the PIXEL space");
    return add_scaled(h, frame, false, fmt, nullptr, nullptr, SH, SW, H, W);
}

// ---- shots (include/rerevst_hip.h "Shots"): the signature of a frame's thumbnail, what a cut detector compares
static_assert(SG_WORDS == RRV_SHOT_SIG_WORDS, "the header's signature size is the kernel's");
int rrv_shot_plan(int SH, int SW, int* th, int* tw) {
    if (!th || !tw || SH < 1 || SW < 1) return RRV_E_ARG;
    const int64_t m = std::max(SH, SW);
    int f = 8;
    for (int k = 1; k <= 8; ++k)
        if ((m + k - 1) / k <= 512) { f = k; break; }
    *th = (SH + f - 1) / f; *tw = (SW + f - 1) / f;
    return RRV_OK;
}
// B contiguous float32 [H][W][3] BGR PIXEL frames at d_frames -> d_sig [B][16][32], queued on q.stream
static int shot_sig_launch(rrv_handle h, const Seq& q, const float* d_frames, int B, int H, int W, uint32_t* d_sig) {
    ShotsP p{d_frames, d_sig, B, H, W};
    int e = 0;
    // for the profile log: bytes from the shapes; eleven integer operations per pixel
    RCHK(launch(h, q, "shot_sig", 11.0 * B * H * W, (12.0 * H * W + 4.0 * SG_WORDS) * B, [&] { e = rrv_shots_launch(&p, q.stream); }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("shot_sig: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}
int rrv_shot_signature_device(rrv_handle h, const float* d_frames, int B, int H, int W, uint32_t* d_sig, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!d_frames || !d_sig) return fail(h, RRV_E_ARG, "shot_signature: null buffer");
    if (B < 1 || B > SG_B_MAX) return fail(h, RRV_E_ARG, "shot_signature: batch must be in 1..64");
    if (H < SG_MIN || W < SG_MIN) return fail(h, RRV_E_ARG, "shot_signature: frames must be at least 4 x 4 pixels");
    HIPCHK(hipSetDevice(h->dev));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    return shot_sig_launch(h, q, d_frames, B, H, W, d_sig);
}
// The checks of a signature request on SH x SW frames and its thumbnail size.  (SH, SW >= 1 and th, tw >= 4 put SH / th and SW / tw within
// 1 .. 8, the resampler's limits.)
static int shot_check(rrv_handle h, const char* who, int SH, int SW, int* th, int* tw) {
    if (rrv_shot_plan(SH, SW, th, tw) != RRV_OK) return fail(h, RRV_E_ARG, std::string(who) + ": SH, SW must be at least 1");
    if (*th < SG_MIN || *tw < SG_MIN)
        return fail(h, RRV_E_ARG, std::string(who) + ": the thumbnail of a " + std::to_string(SH) + " x " + std::to_string(SW) + " frame is " + std::to_string(*th) + " x " +
                                      std::to_string(*tw) + ", below 4 x 4 (rrv_shot_plan)");
    return check_scale(h, who, SH, SW, *th, *tw);
}
// everything a signature request of `frames` frames allocates, before its first launch: both axes' tables and the thumbnails
static int shot_reserve(rrv_handle h, int frames, int SH, int SW, int th, int tw) {
    const rrv_ctx::RsTab *ty, *tx;
    RCHK(rs_pair(h, SH, SW, th, tw, &ty, &tx));
    return ensure_dev(h, h->sg_thumb, h->sg_thumb_cap, (size_t)frames * th * tw * 3);
}
// B (1..64) frames of SH x SW in the format `fmt` through `v` -> their thumbnails -> d_sig, queued on `stream`; shot_reserve has run
static int shot_queue(rrv_handle h, const void* d_in, InFmt fmt, const rrv_image_view& v, int B, int SH, int SW, int th, int tw, uint32_t* d_sig, hipStream_t stream) {
    Seq q = base_seq(h);
    q.stream = stream;
    RCHK(resample_launch(h, q, d_in, fmt, img_view(v), B, SH, SW, th, tw, h->sg_thumb));
    return shot_sig_launch(h, q, h->sg_thumb, B, th, tw, d_sig);
}
int rrv_shot_signature_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, uint32_t* d_sig, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!in) return fail(h, RRV_E_ARG, "shot_signature_view: null view");
    InFmt fmt;
    if (!parse_in_view(in->desc, &fmt)) return fail(h, RRV_E_ARG, "shot_signature_view: in.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (!d_in || !d_sig) return fail(h, RRV_E_ARG, "shot_signature_view: null buffer");
    if (B < 1 || B > SG_B_MAX) return fail(h, RRV_E_ARG, "shot_signature_view: batch must be in 1..64");
    int th = 0, tw = 0;
    RCHK(shot_check(h, "shot_signature_view", SH, SW, &th, &tw));
    std::string why;
    if (!view_check(*in, B, SH, SW, false, &why)) return fail(h, RRV_E_ARG, "shot_signature_view: in." + why);
    HIPCHK(hipSetDevice(h->dev));
    RCHK(shot_reserve(h, B, SH, SW, th, tw));
    return shot_queue(h, d_in, fmt, *in, B, SH, SW, th, tw, d_sig, (hipStream_t)hip_stream);
}
// The host twins: sub-batches of up to sixteen frames on the handle's first stream, one after the other: frames up, the request, signatures back.
constexpr int SHOT_SUB = 16;
int rrv_shot_signature(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, uint32_t* sig) {
    if (!h) return RRV_E_ARG;
    if (!frames || !sig) return fail(h, RRV_E_ARG, "shot_signature: null buffer");
    if (B < 1) return fail(h, RRV_E_ARG, "shot_signature: batch must be at least 1");
    InFmt fmt;
    if (!parse_in_host(in, &fmt)) return fail(h, RRV_E_ARG, "shot_signature: the input is uint8 HWC BGR or a YUV layout with its own sample type, in the PIXEL space");
    int th = 0, tw = 0;
    RCHK(shot_check(h, "shot_signature", SH, SW, &th, &tw));
    HIPCHK(hipSetDevice(h->dev));
    const int sub = std::min(B, SHOT_SUB);
    const size_t fb = in_frame_bytes(fmt.form, SH, SW, fmt.cs);
    const rrv_image_view v = contiguous_of(in, SH, SW);
    RCHK(shot_reserve(h, sub, SH, SW, th, tw));
    RCHK(ensure_dev(h, h->sg_in, h->sg_in_cap, (size_t)sub * fb));
    RCHK(ensure_dev(h, h->sg_sig, h->sg_sig_cap, (size_t)sub * SG_WORDS));
    const hipStream_t s = h->slots[0].stream;
    for (int b0 = 0; b0 < B; b0 += sub) {
        const int nb = std::min(sub, B - b0);
        HIPCHK(hipMemcpyAsync(h->sg_in, (const uint8_t*)frames + (size_t)b0 * fb, (size_t)nb * fb, hipMemcpyHostToDevice, s));
        const int rc = shot_queue(h, h->sg_in, fmt, v, nb, SH, SW, th, tw, h->sg_sig, s);
        if (rc != RRV_OK) { (void)hipStreamSynchronize(s); return rc; }      // (the caller's frames are not read after the call returns)
        HIPCHK(hipMemcpyAsync(sig + (size_t)b0 * SG_WORDS, h->sg_sig, (size_t)nb * SG_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return RRV_OK;
}
int rrv_shot_signature_from_jpeg(rrv_handle h, const uint8_t* const* streams, const size_t* sizes, int B, uint32_t* sig) {
    if (!h) return RRV_E_ARG;
    if (!sig) return fail(h, RRV_E_ARG, "shot_signature_from_jpeg: null buffer");
    std::vector<JpegInfo> infos;
    size_t cap = 0;
    int th = 0, tw = 0;
    return jpeg_in_host(h, "shot_signature_from_jpeg", streams, sizes, B, &infos, &cap, [&](int sub) -> int {
        JpegInCall k;
        int dummy = 0;
        RCHK(jpeg_in_check(h, "shot_signature_from_jpeg", streams[0], cap, reinterpret_cast<const rrv_jpeg_info*>(infos.data()), sub, &dummy, &k));
        RCHK(shot_check(h, "shot_signature_from_jpeg", k.p.H, k.p.W, &th, &tw));
        HIPCHK(hipSetDevice(h->dev));
        RCHK(shot_reserve(h, sub, k.p.H, k.p.W, th, tw));
        return ensure_dev(h, h->sg_sig, h->sg_sig_cap, (size_t)sub * SG_WORDS);
    }, [&](int b0, int nb, hipStream_t s) -> int {
        JpegInCall k;
        RCHK(jpeg_in_check(h, "shot_signature_from_jpeg", h->jd_streams, cap, reinterpret_cast<const rrv_jpeg_info*>(infos.data()) + b0, nb, h->jd_status, &k));
        RCHK(jpeg_in_queue(h, k, h->jd_streams, h->jd_status, s));
        InFmt fmt;
        if (!parse_in_view(k.vin.desc, &fmt)) return fail(h, RRV_E_ARG, "shot_signature_from_jpeg: the decoded layout is not an input form");
        const JfifMatrix jfif(h);      // JFIF's colour space whatever matrix the handle holds: put aside here, back on every way out
        RCHK(shot_queue(h, h->jd_planes, fmt, k.vin, nb, k.p.H, k.p.W, th, tw, h->sg_sig, s));
        HIPCHK(hipMemcpyAsync(sig + (size_t)b0 * SG_WORDS, h->sg_sig, (size_t)nb * SG_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        return RRV_OK;
    });
}

// ---- picture area (include/rerevst_hip.h "Picture area"): the line profile a bar detector reads, and the window of a frame as part of a call
static_assert(RRV_PICTURE_THRESHOLD >= 0 && RRV_PICTURE_THRESHOLD <= PC_T_MAX, "the header's default threshold is one the kernel takes");
// the window rules; nullptr: a window of an SH x SW frame, else the offending field and what is wrong with it
static const char* picture_why(int SH, int SW, const rrv_picture* p) {
    if (!p) return "picture is null";
    if (SH < 1 || SW < 1) return "SH, SW must be at least 1";
    if (p->y0 < 0 || (p->y0 & 1)) return "picture.y0 must be even and at least 0";
    if (p->x0 < 0 || (p->x0 & 1)) return "picture.x0 must be even and at least 0";
    if (p->h < 8) return "picture.h must be at least 8";
    if (p->w < 8) return "picture.w must be at least 8";
    if ((int64_t)p->y0 + p->h > SH) return "picture.h reaches below the frame (y0 + h > SH)";
    if ((int64_t)p->x0 + p->w > SW) return "picture.w reaches beyond the frame (x0 + w > SW)";
    if ((p->h & 1) && p->y0 + p->h != SH) return "picture.h must be even unless the window reaches the frame's bottom edge";
    if ((p->w & 1) && p->x0 + p->w != SW) return "picture.w must be even unless the window reaches the frame's right edge";
    return nullptr;
}
int rrv_picture_check(int SH, int SW, const rrv_picture* p) { return picture_why(SH, SW, p) ? RRV_E_ARG : RRV_OK; }
static bool picture_whole(int SH, int SW, const rrv_picture& p) { return p.y0 == 0 && p.x0 == 0 && p.h == SH && p.w == SW; }
// the view of the window of a frame addressed through `full` (a known descriptor, a checked window): offsets move, pitches and the frame stride stay
static rrv_image_view window_of(const rrv_image_view& full, const rrv_picture& p) {
    rrv_image_view w = full;
    const int64_t y0 = p.y0, x0 = p.x0;
    const int cs = view_chroma(full.desc), cy = (int)(y0 >> chroma_sy(cs)), cx = (int)(x0 >> chroma_sx(cs));
    switch (view_layout(full.desc)) {
    case VL_HWC: w.plane_offset[0] += y0 * full.pitch[0] + 3 * x0; break;
    case VL_CHW: for (int k = 0; k < 3; ++k) w.plane_offset[k] += y0 * full.pitch[k] + x0; break;
    case VL_I420:
        w.plane_offset[0] += y0 * full.pitch[0] + x0;
        for (int k = 1; k < 3; ++k) w.plane_offset[k] += (int64_t)cy * full.pitch[k] + cx;
        break;
    default:
        w.plane_offset[0] += y0 * full.pitch[0] + x0;
        w.plane_offset[1] += (int64_t)cy * full.pitch[1] + 2 * (int64_t)cx;
        break;
    }
    return w;
}
int rrv_picture_view(const rrv_image_view* full, int SH, int SW, const rrv_picture* p, rrv_image_view* win) {
    if (!full || !win || !view_desc_ok(full->desc) || picture_why(SH, SW, p)) return RRV_E_ARG;
    *win = window_of(*full, *p);
    return RRV_OK;
}
// B contiguous float32 [H][W][3] BGR PIXEL frames at d_frames -> d_prof [B][H + W] through the scratch `part`, queued on q.stream
static int picture_launch(rrv_handle h, const Seq& q, const float* d_frames, int B, int H, int W, int threshold, uint32_t* part, uint32_t* d_prof) {
    PictureP p{d_frames, d_prof, part, B, H, W, threshold};
    int e = 0;
    // for the profile log: bytes from the shapes (the frames read, the scratch written and read, the profile written); fourteen integer operations per pixel
    RCHK(launch(h, q, "picture_profile", 14.0 * B * H * W, (12.0 * H * W + 8.0 * pc_strips(H) * W + 4.0 * (H + W)) * B, [&] { e = rrv_picture_launch(&p, q.stream); }));
    if (e != 0) return fail(h, RRV_E_HIP, std::string("picture_profile: launch failed: ") + hipGetErrorString((hipError_t)e));
    return RRV_OK;
}
static int picture_profile_check(rrv_handle h, const char* who, int B, int H, int W, int threshold) {
    if (B < 1 || B > PC_B_MAX) return fail(h, RRV_E_ARG, std::string(who) + ": batch must be in 1..64");
    if (H < PC_MIN || W < PC_MIN) return fail(h, RRV_E_ARG, std::string(who) + ": frames must be at least 8 x 8 pixels");
    if (threshold < 0 || threshold > PC_T_MAX) return fail(h, RRV_E_ARG, std::string(who) + ": threshold must be in 0..254");
    return RRV_OK;
}
int rrv_picture_profile_device(rrv_handle h, const float* d_frames, int B, int H, int W, int threshold, uint32_t* d_prof, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!d_frames || !d_prof) return fail(h, RRV_E_ARG, "picture_profile: null buffer");
    RCHK(picture_profile_check(h, "picture_profile", B, H, W, threshold));
    HIPCHK(hipSetDevice(h->dev));
    RCHK(ensure_dev(h, h->pc_part, h->pc_part_cap, pc_part_words(B, H, W)));
    Seq q = base_seq(h);
    q.stream = (hipStream_t)hip_stream;
    return picture_launch(h, q, d_frames, B, H, W, threshold, h->pc_part, d_prof);
}
// everything a profile request of `frames` frames of SH x SW allocates, before its first launch: the equal-size tables, the float frames, the scratch
static int picture_reserve(rrv_handle h, int frames, int SH, int SW) {
    const rrv_ctx::RsTab *ty, *tx;
    RCHK(rs_pair(h, SH, SW, SH, SW, &ty, &tx));
    RCHK(ensure_dev(h, h->pc_frames, h->pc_frames_cap, (size_t)frames * SH * SW * 3));
    return ensure_dev(h, h->pc_part, h->pc_part_cap, pc_part_words(frames, SH, SW));
}
// B (1..64) frames of SH x SW in the format `fmt` through `v` -> their float32 frames -> d_prof, queued on `stream`; picture_reserve has run
static int picture_queue(rrv_handle h, const void* d_in, InFmt fmt, const rrv_image_view& v, int B, int SH, int SW, int threshold, uint32_t* d_prof, hipStream_t stream) {
    Seq q = base_seq(h);
    q.stream = stream;
    RCHK(resample_launch(h, q, d_in, fmt, img_view(v), B, SH, SW, SH, SW, h->pc_frames));
    return picture_launch(h, q, h->pc_frames, B, SH, SW, threshold, h->pc_part, d_prof);
}
int rrv_picture_profile_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int threshold, uint32_t* d_prof, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    if (!in) return fail(h, RRV_E_ARG, "picture_profile_view: null view");
    InFmt fmt;
    if (!parse_in_view(in->desc, &fmt)) return fail(h, RRV_E_ARG, "picture_profile_view: in.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (!d_in || !d_prof) return fail(h, RRV_E_ARG, "picture_profile_view: null buffer");
    RCHK(picture_profile_check(h, "picture_profile_view", B, SH, SW, threshold));
    std::string why;
    if (!view_check(*in, B, SH, SW, false, &why)) return fail(h, RRV_E_ARG, "picture_profile_view: in." + why);
    HIPCHK(hipSetDevice(h->dev));
    RCHK(picture_reserve(h, B, SH, SW));
    return picture_queue(h, d_in, fmt, *in, B, SH, SW, threshold, d_prof, (hipStream_t)hip_stream);
}
// The host twin of the whole detection pass: every sub-batch is uploaded once and gives its signatures and / or its profiles, one after the
// other on the handle's first stream.  A sub-batch holds at most sixteen frames and at most 4 x HOST_SUB_PIXELS source pixels (the scaled
// host twins' budget), so that the float frames of a 4K sub-batch stay what a scaled call stages.
int rrv_scan_frames(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int threshold, uint32_t* sig, uint32_t* prof) {
    if (!h) return RRV_E_ARG;
    if (!frames) return fail(h, RRV_E_ARG, "scan_frames: null buffer");
    if (!sig && !prof) return fail(h, RRV_E_ARG, "scan_frames: sig and prof are both null: nothing to compute");
    if (B < 1) return fail(h, RRV_E_ARG, "scan_frames: batch must be at least 1");
    InFmt fmt;
    if (!parse_in_host(in, &fmt)) return fail(h, RRV_E_ARG, "scan_frames: the input is uint8 HWC BGR or a YUV layout with its own sample type, in the PIXEL space");
    if (SH < 1 || SW < 1) return fail(h, RRV_E_ARG, "scan_frames: SH, SW must be at least 1");
    int th = 0, tw = 0;
    if (sig) RCHK(shot_check(h, "scan_frames", SH, SW, &th, &tw));
    if (prof) RCHK(picture_profile_check(h, "scan_frames", 1, SH, SW, threshold));
    HIPCHK(hipSetDevice(h->dev));
    const int sub = (int)std::max(1L, std::min((long)std::min(B, SHOT_SUB), 4 * HOST_SUB_PIXELS / ((long)SH * SW)));
    const size_t fb = in_frame_bytes(fmt.form, SH, SW, fmt.cs), pw = (size_t)SH + SW;
    const rrv_image_view v = contiguous_of(in, SH, SW);
    if (sig) {
        RCHK(shot_reserve(h, sub, SH, SW, th, tw));
        RCHK(ensure_dev(h, h->sg_sig, h->sg_sig_cap, (size_t)sub * SG_WORDS));
    }
    if (prof) {
        RCHK(picture_reserve(h, sub, SH, SW));
        RCHK(ensure_dev(h, h->pc_prof, h->pc_prof_cap, (size_t)sub * pw));
    }
    RCHK(ensure_dev(h, h->pc_in, h->pc_in_cap, (size_t)sub * fb));
    const hipStream_t s = h->slots[0].stream;
    for (int b0 = 0; b0 < B; b0 += sub) {
        const int nb = std::min(sub, B - b0);
        HIPCHK(hipMemcpyAsync(h->pc_in, (const uint8_t*)frames + (size_t)b0 * fb, (size_t)nb * fb, hipMemcpyHostToDevice, s));
        int rc = RRV_OK;
        if (sig) rc = shot_queue(h, h->pc_in, fmt, v, nb, SH, SW, th, tw, h->sg_sig, s);
        if (rc == RRV_OK && prof) rc = picture_queue(h, h->pc_in, fmt, v, nb, SH, SW, threshold, h->pc_prof, s);
        if (rc != RRV_OK) { (void)hipStreamSynchronize(s); return rc; }      // (the caller's frames are not read after the call returns)
        if (sig) HIPCHK(hipMemcpyAsync(sig + (size_t)b0 * SG_WORDS, h->sg_sig, (size_t)nb * SG_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (prof) HIPCHK(hipMemcpyAsync(prof + (size_t)b0 * pw, h->pc_prof, (size_t)nb * pw * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return RRV_OK;
}
// The add entries: rrv_add_scaled_view_device on the window's view, SH := p->h, SW := p->w; H = W = 0: the window's own size
int rrv_add_picture_view_device(rrv_handle h, const void* d_frame, const rrv_image_view* in, int SH, int SW, const rrv_picture* p, int H, int W, void* hip_stream) {
    if (!h || !d_frame || !in) return RRV_E_ARG;
    InFmt fmt;
    if (!parse_in_view(in->desc, &fmt)) return fail(h, RRV_E_ARG, "add_picture_view: in.desc is not a dtype, layout and space combination the descriptor entries accept");
    if (const char* why = picture_why(SH, SW, p)) return fail(h, RRV_E_ARG, std::string("add_picture_view: ") + why);
    std::string vwhy;
    if (!view_check(*in, 1, SH, SW, false, &vwhy)) return fail(h, RRV_E_ARG, "add_picture_view: in." + vwhy);
    const rrv_image_view win = window_of(*in, *p);
    return add_scaled(h, d_frame, true, fmt, &win, (hipStream_t)hip_stream, p->h, p->w, H || W ? H : p->h, H || W ? W : p->w);
}
int rrv_add_picture(rrv_handle h, const void* frame, rrv_image_desc in, int SH, int SW, const rrv_picture* p, int H, int W) {
    if (!h || !frame) return RRV_E_ARG;
    InFmt fmt;
    if (!parse_in_host(in, &fmt)) return fail(h, RRV_E_ARG, "add_picture: the input is uint8 HWC BGR or a YUV layout with its own sample type, in the PIXEL space");
    if (const char* why = picture_why(SH, SW, p)) return fail(h, RRV_E_ARG, std::string("add_picture: ") + why);
    const rrv_image_view win = window_of(contiguous_of(in, SH, SW), *p);
    return add_scaled(h, frame, false, fmt, &win, nullptr, p->h, p->w, H || W ? H : p->h, H || W ? W : p->w, in_frame_bytes(fmt.form, SH, SW, fmt.cs));
}
// The transfer entries: the request on the window as a compositing request (SH := h, SW := w, the working size, DH := h, DW := w) with
// Xfer::pic set; run_xfer places its float32 result in the canvas of the whole source and delivers that.  `x` arrives with B and the window
// fields unset; who: the entry's name in the refusals.  Returns 1 where the window is the whole frame (the caller runs the composite entry).
static int set_picture(rrv_handle h, const char* who, int B, int SH, int SW, const rrv_picture* p, int H, int W, int r, float eps, const rrv_composite* c, int flags,
                       bool host, Xfer* x) {
    const std::string w = std::string(who) + ": ";
    if (const char* why = picture_why(SH, SW, p)) return fail(h, RRV_E_ARG, w + why);
    if (flags & ~(RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE | RRV_TF_ON_STREAM)) return fail(h, RRV_E_ARG, w + "the flags are RRV_TF_FRAME_MODE and RRV_TF_ON_STREAM (RRV_TF_PAD_CROP is forced); blended and masked models are not offered with a window");
    if (B < 1 || (!host && B > 64)) return fail(h, RRV_E_ARG, w + (host ? "batch must be at least 1" : "batch must be in 1..64"));
    if ((H != 0 || W != 0) && (H < 1 || W < 1)) return fail(h, RRV_E_ARG, w + "H, W must be at least 1, or both 0 for the window's own size");
    const bool work = (H != 0 || W != 0) && (H != p->h || W != p->w);      // a working size of its own: the window is resampled to it
    *x = Xfer{Model::GLOBAL, B, work ? H : p->h, work ? W : p->w};
    if (work) { x->SH = p->h; x->SW = p->w; }
    x->DH = p->h; x->DW = p->w;
    if (r) { x->gr = r; x->geps = eps; }
    RCHK(set_composite(h, who, c, B, x));
    if (picture_whole(SH, SW, *p)) return 1;
    x->pic = true; x->py0 = p->y0; x->px0 = p->x0; x->FH = SH; x->FW = SW;
    return RRV_OK;
}
int rrv_transfer_picture_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, const rrv_picture* p, int H, int W, int r,
                                     float eps, const rrv_composite* c, void* d_out, const rrv_image_view* out, int flags, void* hip_stream) {
    if (!h) return RRV_E_ARG;
    const char* const who = "transfer_picture_view";
    if (!in || !out) return fail(h, RRV_E_ARG, std::string(who) + ": null view");
    Xfer x{Model::GLOBAL, B, H, W};
    const int rc = set_picture(h, who, B, SH, SW, p, H, W, r, eps, c, flags, false, &x);
    if (rc < 0) return rc;
    flags |= RRV_TF_PAD_CROP;
    if (rc == 1) return view_run(h, who, d_in, in, d_out, out, flags, hip_stream, x);      // the whole frame: the composite entry, no kernel added
    if (!view_desc_ok(in->desc)) return fail(h, RRV_E_ARG, std::string(who) + ": in.desc is not a dtype, layout and space combination the descriptor entries accept");
    std::string why;
    if (!view_check(*in, B, SH, SW, false, &why)) return fail(h, RRV_E_ARG, std::string(who) + ": in." + why);
    if (view_desc_ok(out->desc) && !view_check(*out, B, SH, SW, true, &why)) return fail(h, RRV_E_ARG, std::string(who) + ": out." + why);      // (an unknown out.desc: view_run's words)
    const rrv_image_view win = window_of(*in, *p);
    x.vfull = in;
    return view_run(h, who, d_in, &win, d_out, out, flags, hip_stream, x);
}
int rrv_transfer_picture(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, const rrv_picture* p, int H, int W, int r, float eps,
                         const rrv_composite* c, void* out, rrv_image_desc od, int flags) {
    if (!h) return RRV_E_ARG;
    const char* const who = "transfer_picture";
    Xfer x{Model::GLOBAL, B, H, W};
    if (flags & RRV_TF_ON_STREAM) return fail(h, RRV_E_ARG, std::string(who) + ": unknown flags");
    const int rc = set_picture(h, who, B, SH, SW, p, H, W, r, eps, c, flags, true, &x);
    if (rc < 0) return rc;
    flags |= RRV_TF_PAD_CROP;
    if (rc == 1) return scaled_host(h, who, false, frames, in, out, od, flags, x);
    InFmt fmt;
    if (!parse_in_host(in, &fmt)) return fail(h, RRV_E_ARG, std::string(who) + ": the input is uint8 HWC BGR or a YUV layout with its own sample type, in the PIXEL space");
    OutFmt ofmt;
    if (parse_out(od, &ofmt) != DescErr::OK || ofmt.chw || ofmt.space != SP_PIXEL)
        return fail(h, RRV_E_ARG, std::string(who) + ": the output is float32 or uint8 HWC BGR in the PIXEL space, uint8 I420 / NV12, or uint16 I420_16 / P016 (4:2:0, or with RRV_LAY_422 / RRV_LAY_444)");
    // the views of the whole contiguous frames on both sides and of the window; they live until the pipeline has returned (it is synchronous)
    const rrv_image_view full = contiguous_of(in, SH, SW), win = window_of(full, *p), vout = contiguous_of(od, SH, SW);
    x.vfull = &full; x.vin = &win; x.vout = &vout;
    return scaled_host(h, who, false, frames, in, out, od, flags, x);
}

// The matrix of the YUV input forms, the inverse of rrv_yuv_matrix's transform: Y' = (Y - 16) 255/219, C' = (C - 128) 255/224 (full range: Y' = Y,
// C' = C - 128), R = Y' + 2(1-Kr) Cr', B = Y' + 2(1-Kb) Cb', G = Y' - (2 Kb (1-Kb) / Kg) Cb' - (2 Kr (1-Kr) / Kg) Cr'; the offsets folded into
// column 3.  Coefficients in double, each rounded once to float32.
// d-bit codes (bits = 8, 10, 12, 16; s = 2^(d-8)): limited range Y' = (Y / s - 16) 255/219, C' = (C / s - 128) 255/224, i.e. the 8-bit coefficients
// divided by s (exact) and the 8-bit offsets; full range Y' = 255/(2^d - 1) Y, C' = 255/(2^d - 1) (C - 2^(d-1)).
static bool yuv_depth_ok(int bits) { return bits == 8 || bits == 10 || bits == 12 || bits == 16; }
int rrv_yuv_input_matrix_depth(int standard, int full_range, int bits, float n[12]) {
    if (!n || (standard != RRV_YUV_BT601 && standard != RRV_YUV_BT709) || !yuv_depth_ok(bits)) return RRV_E_ARG;
    const double kr = standard == RRV_YUV_BT601 ? 0.299 : 0.2126, kb = standard == RRV_YUV_BT601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double s = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double ys = full_range ? 255.0 / top : 255.0 / 219.0 / s, cs = full_range ? 255.0 / top : 255.0 / 224.0 / s;
    const double y0 = full_range ? 0.0 : 16.0 * s, c0 = 128.0 * s;
    const double cb[3] = {0.0, -(2.0 * kb * (1.0 - kb) / kg), 2.0 * (1.0 - kb)}, cr[3] = {2.0 * (1.0 - kr), -(2.0 * kr * (1.0 - kr) / kg), 0.0};
    for (int k = 0; k < 3; ++k) {
        n[4 * k] = (float)ys;
        n[4 * k + 1] = (float)(cs * cb[k]);
        n[4 * k + 2] = (float)(cs * cr[k]);
        n[4 * k + 3] = (float)(-(ys * y0) - c0 * (cs * cb[k]) - c0 * (cs * cr[k]));
    }
    return RRV_OK;
}
int rrv_yuv_input_matrix(int standard, int full_range, float n[12]) { return rrv_yuv_input_matrix_depth(standard, full_range, 8, n); }

// The conversion matrix of the YUV forms: Y = Kr R + Kg G + Kb B, Cb = 128 + (B - Y) / (2 (1 - Kb)), Cr = 128 + (R - Y) / (2 (1 - Kr)); limited
// range scales Y by 219/255 (+16) and the chroma differences by 224/255.  Coefficients in double, each rounded once to float32.
// d-bit codes (s = 2^(d-8)): limited range Y' = (16 + 219/255 Y) s, chroma (128 + 224/255 C) s — the 8-bit matrix times s, exactly; full range
// Y' = (2^d - 1)/255 Y, chroma 2^(d-1) + (2^d - 1)/255 C.
int rrv_yuv_matrix_depth(int standard, int full_range, int bits, float m[12]) {
    if (!m || (standard != RRV_YUV_BT601 && standard != RRV_YUV_BT709) || !yuv_depth_ok(bits)) return RRV_E_ARG;
    const double kr = standard == RRV_YUV_BT601 ? 0.299 : 0.2126, kb = standard == RRV_YUV_BT601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double s = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double ys = full_range ? top / 255.0 : 219.0 / 255.0 * s, cs = full_range ? top / 255.0 : 224.0 / 255.0 * s;
    const double y[3] = {kr, kg, kb};
    for (int c = 0; c < 3; ++c) {
        m[c] = (float)(ys * y[c]);
        m[4 + c] = (float)(cs * ((c == 2 ? 1.0 : 0.0) - y[c]) / (2.0 * (1.0 - kb)));
        m[8 + c] = (float)(cs * ((c == 0 ? 1.0 : 0.0) - y[c]) / (2.0 * (1.0 - kr)));
    }
    m[3] = full_range ? 0.f : (float)(16.0 * s);
    m[7] = m[11] = (float)(128.0 * s);
    return RRV_OK;
}
int rrv_yuv_matrix(int standard, int full_range, float m[12]) { return rrv_yuv_matrix_depth(standard, full_range, 8, m); }

// The uint16 forms' state: the code depth of each side, and matrices independent of the 8-bit ones and of each other.  NULL: BT.601 limited
// range at the depth in force when a call launches (run_encoder / run_last work it out then).
int rrv_set_yuv_depth(rrv_handle h, int in_bits, int out_bits) {
    if (!h) return RRV_E_ARG;
    auto ok = [](int b) { return b == 0 || b == 10 || b == 12 || b == 16; };
    if (!ok(in_bits) || !ok(out_bits)) return fail(h, RRV_E_ARG, "set_yuv_depth: a depth is 10, 12 or 16 bits (0 leaves it as it is)");
    if (in_bits) h->yuv_in.bits = in_bits;
    if (out_bits) h->yuv_out.bits = out_bits;
    return RRV_OK;
}
// The four matrix setters: the input and the output side are independent of each other, and so are a side's 8-bit and uint16 matrices.
// NULL puts back BT.601 limited range (the uint16 forms: at the depth in force when a call launches).
static int set_yuv_matrix(rrv_handle h, bool input, bool wide, const float* src, const char* name) {
    if (!h) return RRV_E_ARG;
    YuvSide& s = input ? h->yuv_in : h->yuv_out;
    if (src) {
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(src[i])) return fail(h, RRV_E_ARG, std::string(name) + ": the twelve coefficients must be finite");
        memcpy(wide ? s.m16 : s.m8, src, sizeof s.m8);
    } else if (!wide) return (input ? rrv_yuv_input_matrix : rrv_yuv_matrix)(RRV_YUV_BT601, 0, s.m8);
    if (wide) s.set16 = src != nullptr;
    return RRV_OK;
}
int rrv_set_yuv_matrix(rrv_handle h, const float m[12]) { return set_yuv_matrix(h, false, false, m, "set_yuv_matrix"); }
int rrv_set_yuv_input_matrix(rrv_handle h, const float n[12]) { return set_yuv_matrix(h, true, false, n, "set_yuv_input_matrix"); }
int rrv_set_yuv16_matrix(rrv_handle h, const float m[12]) { return set_yuv_matrix(h, false, true, m, "set_yuv16_matrix"); }
int rrv_set_yuv16_input_matrix(rrv_handle h, const float n[12]) { return set_yuv_matrix(h, true, true, n, "set_yuv16_input_matrix"); }

// ---- look-ahead form of Stylization.transfer for a one-frame-per-call driver loop (generate_real_video.py:152-171) ----
// rrv_transfer_async queues H2D copy -> kernels -> D2H copy of ONE frame on the copy / compute streams and returns a
// ticket at once; rrv_transfer_wait blocks until that frame's output is in `out`.  With the next frame submitted before
// the previous one is awaited, frame i+1's copy-in and kernels overlap frame i's kernel tails and copy-out (two
// compute streams, four staging sets: up to four tickets may be open; a fifth submission retires the oldest first).
// A pageable `frame` is copied into pinned staging before the call returns (the caller may reuse it at once); a
// pageable `out` is filled by rrv_transfer_wait.  Same arithmetic as rrv_transfer: the results are bit-identical.
static int retire_ticket(rrv_handle h, int set) {
    auto& tk = h->tickets[set];
    if (!tk.open) return RRV_OK;
    HIPCHK(hipEventSynchronize(h->hstage[set].out_done));
    if (tk.out) host_copy(tk.out, h->hstage[set].pin.out, tk.out_bytes);
    tk.open = false;
    return RRV_OK;
}

static int transfer_async(rrv_handle h, const uint8_t* frame, int H, int W, void* out, OutFmt fmt, long* ticket) {
    if (!h || !frame || !out || !ticket) return RRV_E_ARG;
    RCHK(check_frame(h, H, W, "transfer"));
    HIPCHK(hipSetDevice(h->dev));
    const size_t fb = (size_t)H * W * 3, fo = (size_t)(H / 8 * 8) * (W / 8 * 8) * 3 * out_elem(fmt);     // input / output bytes
    const long id = h->next_ticket;
    const int set = (int)(id % HOST_SETS);
    auto& st = h->hstage[set];
    RCHK(retire_ticket(h, set));                                   // the set's previous ticket (four submissions ago)
    const bool in_pin = is_pinned(frame, fb), out_pin = is_pinned(out, fo);
    // this set's staging (nothing of it is in flight any more); the last kernel writes the output to page-locked memory itself
    RCHK(stage_reserve(h, set, in_pin ? 0 : fb, out_pin ? 0 : fo, true));
    RCHK(stage_reserve(h, set, fb, 0, false));
    const uint8_t* src = frame;
    if (!in_pin) { host_copy(st.pin.in, frame, fb); src = st.pin.in; }
    // Four tickets may be open: each runs on its own (stream, workspace) with a quarter of the CUs per persistent grid, so
    // the frames run side by side instead of queueing behind each other's last partial round of work items (one frame
    // fills 1.56 - 12.5 rounds of 256 workgroups per layer; measured device-resident at 512 x 512, one frame per launch:
    // 508 frames/s on one stream, 569 on two, 603 on four with a quarter of the CUs each — profiles/r03_b1_streams.txt)
    const int slot = h->profiling ? 0 : (int)(id % RRV_MAX_SLOTS);      // the ticket's own pair, whatever rrv_set_pipeline says
    h->next_slot = 0;
    Seq q = slot_seq(h, slot);
    q.f43 = true;                                    // the per-frame path
    hipStream_t cs = q.stream;
    if (!h->profiling && h->grid_share == 1) {       // this ticket's share: as many shares as frames in flight once it is queued (1 .. 4); else the handle's
        int open = 1;
        for (auto& tk : h->tickets)
            if (tk.open && tk.id != id - HOST_SETS && hipEventQuery(h->hstage[tk.id % HOST_SETS].out_done) == hipErrorNotReady) ++open;
        (void)hipGetLastError();
        q.share = open > RRV_MAX_SLOTS ? RRV_MAX_SLOTS : open;
    }
    // No copy streams, whatever rrv_set_host_io says: the frame is copied in on the ticket's OWN stream (1.2 MB; a
    // kernel reading it from host memory byte by byte costs more, bench `zero_copy_input_only`) and the last kernel writes
    // the destination in page-locked host memory in 192-byte bursts.  (Separate copy streams would add two streams to the
    // four compute streams — more than hardware queues, and a D2H copy then waits behind another frame's kernels:
    // measured 230-260 frames/s against 551.)
    RCHK(ensure_active(h));
    HIPCHK(hipMemcpyAsync(st.dev.in, src, fb, hipMemcpyHostToDevice, cs));
    HIPCHK(hipEventRecord(st.in_done, cs));      // the frame has left the caller's buffer (waited for below when the copy reads it directly)
    const int rc0 = transfer_device(h, q, st.dev.in, 1, H, W, out_pin ? out : st.pin.out, FrameIO{IN_BGR8, fmt, nullptr, nullptr, nullptr, CallerOrder{h->caller_stream, h->caller_sync}});
    // Contract (include/rerevst_hip.h): `frame` may be reused as soon as the call returns.  A pageable frame was copied to
    // staging above; a page-locked one is the DIRECT source of the asynchronous H2D copy, so wait for that copy (queued
    // first on an idle stream: finished long before the launches above were) — also on the error path.
    if (in_pin) HIPCHK(hipEventSynchronize(st.in_done));
    if (rc0 != RRV_OK) return rc0;
    HIPCHK(hipEventRecord(st.out_done, cs));
    auto& tk0 = h->tickets[set];
    tk0.id = id; tk0.out = out_pin ? nullptr : out; tk0.out_bytes = fo; tk0.open = true;
    h->next_ticket = id + 1;
    *ticket = id;
    return RRV_OK;
}
int rrv_transfer_async(rrv_handle h, const uint8_t* frame, int H, int W, float* out, long* ticket) {
    return transfer_async(h, frame, H, W, out, OUT_F32, ticket);
}
int rrv_transfer_async_u8(rrv_handle h, const uint8_t* frame, int H, int W, uint8_t* out, long* ticket) {
    return transfer_async(h, frame, H, W, out, OUT_U8, ticket);
}

int rrv_transfer_wait(rrv_handle h, long ticket) {
    if (!h) return RRV_E_ARG;
    if (ticket < 0 || ticket >= h->next_ticket) return fail(h, RRV_E_ARG, "transfer_wait: no such ticket");
    HIPCHK(hipSetDevice(h->dev));
    const int set = (int)(ticket % HOST_SETS);
    if (h->tickets[set].id != ticket) {
        if (h->tickets[set].id > ticket) return RRV_OK;            // retired by a later submission: its output is already delivered
        return fail(h, RRV_E_ARG, "transfer_wait: unknown ticket");
    }
    return retire_ticket(h, set);
}

// ---- multi-style feature API ("Multi-style Interpolation/stylization.py":66-100): the reference caches the
// encoder output of every frame on disk (test.py:87-101) and feeds it back; here the cache lives in HBM.
static size_t feature_floats(int H, int W) {      // ring-layout [1, H/8, W/8, 512] image + the same slack as talloc (tile-overrun reads stay inside)
    const int fh = H / 8, fw = W / 8;
    return (size_t)(fh + 2) * (fw + 2) * 512 + (size_t)20 * (fw + 2 + 20) * 512;
}

int rrv_generate_content_features(rrv_handle h, const uint8_t* frame, int H, int W, int* feature_id) {
    if (!h || !frame || !feature_id) return RRV_E_ARG;
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    RCHK(check_frame(h, H, W, "generate_content_features"));
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    rrv_ctx::Feature ft{nullptr, H, W, nullptr, true};
    const size_t need = feature_floats(H, W) * sizeof(float);
    if (h->feat_bytes + need > h->feat_cap) {        // over the cap: keep the pixels, encode on use
        RCHK(dmalloc(h, (void**)&ft.u8, (size_t)H * W * 3));
        HIPCHK(hipMemcpy(ft.u8, frame, (size_t)H * W * 3, hipMemcpyHostToDevice));
        h->features.push_back(ft);
        *feature_id = (int)h->features.size() - 1;
        return RRV_OK;
    }
    RCHK(ensure_dev(h, h->d_u8, h->d_u8_cap, (size_t)H * W * 3));
    const Seq q = base_seq(h);
    HIPCHK(hipMemcpyAsync(h->d_u8, frame, (size_t)H * W * 3, hipMemcpyHostToDevice, q.stream));
    RCHK(enc_plan(h, q, h->enc_add, 1, H, W));
    RCHK(run_encoder(h, q, h->enc_add, h->d_u8, IN_BGR8, 0, nullptr, nullptr, 1));
    const Tens& f = h->enc_add.c41;
    RCHK(dalloc(h, q, &ft.p, feature_floats(H, W), true));
    HIPCHK(hipMemcpyAsync(ft.p, f.p, f.img_floats() * sizeof(float), hipMemcpyDeviceToDevice, q.stream));
    HIPCHK(hipStreamSynchronize(q.stream));
    h->feat_bytes += need;
    h->features.push_back(ft);
    *feature_id = (int)h->features.size() - 1;
    return RRV_OK;
}

// The caching pass of a whole run of frames ("Multi-style Interpolation/test.py":87-101 encodes every frame once, one at a
// time, and writes cache/%d.pt): B equally sized frames in ONE call.  Sub-batches (as in host_pipeline: ~6.6 Mpixel) alternate
// over the two compute streams while the copy-in stream brings the next ones; the encoder runs several frames per launch
// with the per-frame path's kernel choice (use_f43), and its last layer stores straight into the cache — one arena per call,
// features back to back in ring layout, zeroed once — so there is no allocation, device copy or host wait per frame.
// Frames beyond the cache cap are kept as pixels (one block), as rrv_generate_content_features does.
int rrv_generate_content_features_batch(rrv_handle h, const uint8_t* frames, int B, int H, int W, int* feature_ids) {
    if (!h || !frames || !feature_ids || B < 1) return RRV_E_ARG;
    if (!h->finalized) return fail(h, RRV_E_WEIGHTS, "weights not finalized");
    RCHK(check_frame(h, H, W, "generate_content_features"));
    HIPCHK(hipSetDevice(h->dev));
    RCHK(claim_staging(h));
    const size_t fb = (size_t)H * W * 3;
    Tens one; one.B = 1; one.H = H / 8; one.W = W / 8; one.C = 512;
    const size_t img = one.img_floats(), slack = feature_floats(H, W) - img;
    // how many fit the cache (the arena of n features holds n images + one slack)
    int n_res = 0;
    while (n_res < B && h->feat_bytes + ((size_t)(n_res + 1) * img + slack) * sizeof(float) <= h->feat_cap) ++n_res;
    const int id0 = (int)h->features.size();
    const size_t bytes0 = h->feat_bytes, blocks0 = h->feat_blocks.size();
    float* arena = nullptr;
    // Everything from here on either completes or is undone: a failed allocation / launch must not leave
    // valid-looking feature ids over a zero-filled or half-encoded arena for a later add_patch / transfer_features to use.
    auto work = [&]() -> int {
    if (n_res) {
        RCHK(dmalloc(h, (void**)&arena, ((size_t)n_res * img + slack) * sizeof(float)));
        h->feat_blocks.push_back(arena);
        HIPCHK(hipMemsetAsync(arena, 0, ((size_t)n_res * img + slack) * sizeof(float), h->slots[0].stream));      // the zero ring of every feature
        HIPCHK(hipStreamSynchronize(h->slots[0].stream));
        h->feat_bytes += ((size_t)n_res * img + slack) * sizeof(float);
        for (int i = 0; i < n_res; ++i) h->features.push_back(rrv_ctx::Feature{arena + (size_t)i * img, H, W, nullptr, false});
    }
    if (n_res < B) {       // over the cap: pixels only
        uint8_t* blk = nullptr;
        RCHK(dmalloc(h, (void**)&blk, (size_t)(B - n_res) * fb));
        h->feat_blocks.push_back(blk);
        HIPCHK(hipMemcpy(blk, frames + (size_t)n_res * fb, (size_t)(B - n_res) * fb, hipMemcpyHostToDevice));
        for (int i = n_res; i < B; ++i) h->features.push_back(rrv_ctx::Feature{nullptr, H, W, blk + (size_t)(i - n_res) * fb, false});
    }
    for (int i = 0; i < B; ++i) feature_ids[i] = id0 + i;
    if (!n_res) return RRV_OK;
    const int sub = host_sub(n_res, H, W);
    const int nchunk = (n_res + sub - 1) / sub;
    const int nsets = nchunk < HOST_SETS ? nchunk : HOST_SETS;
    const bool in_pin = is_pinned(frames, (size_t)n_res * fb);
    for (int i = 0; i < nsets; ++i) {      // input staging only: the encoder writes into the arena
        RCHK(stage_reserve(h, i, (size_t)sub * fb, 0, false));
        RCHK(stage_reserve(h, i, in_pin ? 0 : (size_t)sub * fb, 0, true));
    }
    const int nstreams = (h->profiling || h->n_slots < 2) ? 1 : 2;
    int rc = RRV_OK;
    for (int k = 0; k < nchunk && rc == RRV_OK; ++k) {
        auto& st = h->hstage[k % HOST_SETS];
        const int nb = (k + 1) * sub <= n_res ? sub : n_res - k * sub;
        const uint8_t* src = frames + (size_t)k * sub * fb;
        if (k >= HOST_SETS) HIPCHK(hipEventSynchronize(st.k_done));            // the encoder of k-4 has read this set's input (also frees pin_in)
        if (!in_pin) { host_copy(st.pin.in, src, (size_t)nb * fb); src = st.pin.in; }
        const int slot = k % nstreams;
        HIPCHK(hipMemcpyAsync(st.dev.in, src, (size_t)nb * fb, hipMemcpyHostToDevice, h->copy_in));
        HIPCHK(hipEventRecord(st.in_done, h->copy_in));
        HIPCHK(hipStreamWaitEvent(h->slots[slot].stream, st.in_done, 0));
        Seq q = slot_seq(h, slot);
        q.f43 = true;                        // the same kernel choice as the per-frame path's encoder (rrv_set_f43)
        EncPlan& e = pick_plan(h, h->slots[slot].enc, nb, H, W);
        rc = enc_plan(h, q, e, nb, H, W, true);
        if (rc != RRV_OK) break;
        e.gen = ++h->launch_gen;
        Tens out41 = one; out41.B = nb; out41.p = arena + (size_t)k * sub * img;
        rc = run_encoder(h, q, e, st.dev.in, IN_BGR8, 0, nullptr, nullptr, nb, &out41);
        if (rc != RRV_OK) break;
        HIPCHK(hipEventRecord(st.k_done, h->slots[slot].stream));
    }
    const int rs = sync_all(h);
    if (rc == RRV_OK) rc = rs;
    if (rc == RRV_OK && h->debug) rc = debug_verify(h, "generate_content_features_batch");
    return rc;
    };
    const int rc = work();
    if (rc != RRV_OK) {
        const std::string why = h->err;
        (void)sync_all(h);
        (void)hipGetLastError();
        h->features.resize((size_t)id0);
        while (h->feat_blocks.size() > blocks0) { (void)hipFree(h->feat_blocks.back()); h->feat_blocks.pop_back(); }
        h->feat_bytes = bytes0;
        for (int i = 0; i < B; ++i) feature_ids[i] = -1;
        h->err = why;
    }
    return rc;
}

int rrv_set_feature_cache_cap(rrv_handle h, size_t bytes) {
    if (!h) return RRV_E_ARG;
    h->feat_cap = bytes;
    return RRV_OK;
}
int rrv_feature_cache_info(rrv_handle h, int* resident, int* spilled, size_t* bytes) {
    if (!h) return RRV_E_ARG;
    int r = 0, sp = 0;
    for (auto& f : h->features) { r += f.p ? 1 : 0; sp += f.u8 ? 1 : 0; }
    if (resident) *resident = r;
    if (spilled) *spilled = sp;
    if (bytes) *bytes = h->feat_bytes;
    return RRV_OK;
}

int rrv_add_patch(rrv_handle h, int feature_id) {
    if (!h || feature_id < 0 || feature_id >= (int)h->features.size() || !(h->features[feature_id].p || h->features[feature_id].u8)) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    RCHK(flush_pending(h));      // keeps the order of add() and add_patch() calls
    const rrv_ctx::Feature& ft = h->features[feature_id];
    if (!h->patches.empty() && (ft.H != h->add_H || ft.W != h->add_W))
        return fail(h, RRV_E_ARG, "add_patch: all sampled features must have the same size");
    Tens f; f.B = 1; f.H = ft.H / 2 / 2 / 2; f.W = ft.W / 2 / 2 / 2; f.C = 512;
    const Seq q = base_seq(h);
    float* keep = nullptr;
    RCHK(dalloc(h, q, &keep, f.img_floats(), false));
    const float* src = ft.p;
    if (!src) {                  // spilled feature: encode its pixels now
        int rc = enc_plan(h, q, h->enc_add, 1, ft.H, ft.W);
        if (rc == RRV_OK) rc = run_encoder(h, q, h->enc_add, ft.u8, IN_BGR8, 0, nullptr, nullptr, 1);
        if (rc == RRV_OK && hipStreamSynchronize(q.stream) != hipSuccess) rc = fail(h, RRV_E_HIP, "add_patch: encoder failed");
        if (rc != RRV_OK) { (void)hipFree(keep); return rc; }
        src = h->enc_add.c41.p;
    }
    HIPCHK(hipMemcpy(keep, src, f.img_floats() * sizeof(float), hipMemcpyDeviceToDevice));
    h->patches.push_back(keep);
    h->patch_h = f.H; h->patch_w = f.W; h->add_H = ft.H; h->add_W = ft.W;
    return RRV_OK;
}

// n cached features, one weight vector each ([n][ns]), in ONE call.  Frames run in GROUPS of up to sixteen per launch
// sequence — every image of a launch carries its own blended state set (per-image parameters and folded KernelFilter
// weights, ConvP::par_bstride / w_bstride), so the small relu4_1-level layers see G x the pixel tiles of one frame —
// and consecutive groups alternate over two (stream, workspace, sixteen state sets): group k+1's blends, folds and
// decoder overlap group k's D2H copy.  A group is one BLEND request of run_xfer over its cached features; rrv_transfer_features is n = 1.  With a fixed kernel mode a frame's arithmetic does not depend on its group
// (bit-identical to one frame per call); the default mode chooses the kernels by the group's frames.  Features beyond the cache cap (kept as pixels) run alone through the encoder + decoder entry.
static int transfer_features_batch(rrv_handle h, const int* ids, const float* wts, int n, int ns, void* out, OutFmt fmt) {
    if (!h || !ids || !wts || !out || n < 1 || ns < 1 || ns > RRV_MAX_STYLES) return RRV_E_ARG;
    const auto t_entry = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(h->dev));
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= (int)h->features.size() || !(h->features[ids[i]].p || h->features[ids[i]].u8)) return fail(h, RRV_E_ARG, "transfer: unknown feature id");
    for (int s = 0; s < ns; ++s)
        if (!h->styles[s].computed) return fail(h, RRV_E_STATE, "blend: state not computed for every style");
    const int H = h->features[ids[0]].H, W = h->features[ids[0]].W;
    for (int i = 1; i < n; ++i)
        if (h->features[ids[i]].H != H || h->features[ids[i]].W != W) return fail(h, RRV_E_ARG, "transfer: features of one call must share their size");
    RCHK(claim_staging(h));
    const size_t npx = (size_t)(H / 8 * 8) * (W / 8 * 8) * 3 * out_elem(fmt);      // output bytes per frame
    char* const outc = (char*)out;
    const bool out_pin = is_pinned(out, (size_t)n * npx);
    // Frames per launch sequence (rrv_set_multistyle_group; default: the host entries' ~6.6 Mpixel per launch — 4 at 1152 x 1152,
    // 16 at 640 x 640 and below).  Measured with four styles (conv_f43_k with per-image parameters, round 5): 1152 x 1152
    // 371 / 382 / 381 frames/s for 1 / 2 / 4; 640 x 640 941 / 1070 / 1167; 384 x 384 1750 / 2163 / 2590.
    int G = h->ms_group;
    if (G == 0) {
        const long s = HOST_SUB_PIXELS / ((long)H * W);
        G = s < 1 ? 1 : s > rrv_ctx::MS_GROUP_MAX ? rrv_ctx::MS_GROUP_MAX : (int)s;
    }
    if (G > n) G = n;
    struct Group { int first, count; };
    std::vector<Group> groups;
    for (int i = 0; i < n;) {           // a spilled feature (pixels, no cached tensor) makes a group of its own
        if (!h->features[ids[i]].p) { groups.push_back({i, 1}); ++i; continue; }
        int c = 0;
        while (c < G && i + c < n && h->features[ids[i + c]].p) ++c;
        groups.push_back({i, c});
        i += c;
    }
    const int ngroups = (int)groups.size();
    const int nslots = (h->profiling || h->n_slots < 2 || ngroups < 2) ? 1 : 2;
    for (int i = 0; i < nslots; ++i) {      // output staging only: the features are on the device
        RCHK(stage_reserve(h, i, 0, (size_t)G * npx, false));
        RCHK(stage_reserve(h, i, 0, out_pin ? 0 : (size_t)G * npx, true));
    }
    const bool tl_on = h->tl.on && ngroups > 1 && ngroups <= rrv_ctx::Timeline::N;
    double tl_setup = 0;
    if (tl_on) { tl_setup = host_ms_since(t_entry); HIPCHK(hipEventRecord(h->tl.entry, h->slots[0].stream)); }
    auto drain = [&](int k) -> int {
        auto& st = h->hstage[k % nslots];
        HIPCHK(hipEventSynchronize(st.out_done));
        if (!out_pin) host_copy(outc + (size_t)groups[k].first * npx, st.pin.out, (size_t)groups[k].count * npx);
        return RRV_OK;
    };
    for (int k = 0; k < ngroups; ++k) {
        const int slot = k % nslots, first = groups[k].first, cnt = groups[k].count;
        auto& st = h->hstage[slot];
        if (k >= nslots) {
            if (!out_pin) RCHK(drain(k - nslots));
            HIPCHK(hipStreamWaitEvent(h->slots[slot].stream, st.out_done, 0));      // this slot's device output has left
        }
        const float* fp[rrv_ctx::MS_GROUP_MAX] = {};
        for (int g = 0; g < cnt; ++g) fp[g] = h->features[ids[first + g]].p;
        void* const h_dst = out_pin ? (void*)(outc + (size_t)first * npx) : st.pin.out;
        if (tl_on && k == 0) HIPCHK(hipEventRecord(h->tl.first, h->slots[slot].stream));      // (a diagnostic: in front of the first group's blend, which is part of its request)
        Xfer part{Model::BLEND, cnt, H, W, PLAIN, fmt, ns, wts + (size_t)first * ns};
        if (fp[0]) part.feats = fp;
        RCHK(run_xfer(h, slot, fp[0] ? nullptr : h->features[ids[first]].u8, st.dev.out, part));      // a spilled feature is re-encoded from its uint8 BGR pixels
        if (tl_on) HIPCHK(hipEventRecord(h->tl.k_end[k], h->slots[slot].stream));
        HIPCHK(hipEventRecord(st.k_done, h->slots[slot].stream));
        HIPCHK(hipStreamWaitEvent(h->copy_out, st.k_done, 0));
        HIPCHK(hipMemcpyAsync(h_dst, st.dev.out, (size_t)cnt * npx, hipMemcpyDeviceToHost, h->copy_out));
        HIPCHK(hipEventRecord(st.out_done, h->copy_out));
        if (tl_on) HIPCHK(hipEventRecord(h->tl.d_end[k], h->copy_out));
    }
    if (out_pin) HIPCHK(hipStreamSynchronize(h->copy_out));
    else for (int k = (ngroups - nslots < 0 ? 0 : ngroups - nslots); k < ngroups; ++k) RCHK(drain(k));
    if (tl_on) RCHK(timeline_print(h, "transfer_features_batch", n, H, W, ngroups, tl_setup, host_ms_since(t_entry)));
    return RRV_OK;
}
int rrv_transfer_features(rrv_handle h, int feature_id, const float* wts, int ns, float* out) {
    return transfer_features_batch(h, &feature_id, wts, 1, ns, out, OUT_F32);
}
int rrv_transfer_features_u8(rrv_handle h, int feature_id, const float* wts, int ns, uint8_t* out) {
    return transfer_features_batch(h, &feature_id, wts, 1, ns, out, OUT_U8);
}
int rrv_transfer_features_batch(rrv_handle h, const int* ids, const float* wts, int n, int ns, float* out) {
    return transfer_features_batch(h, ids, wts, n, ns, out, OUT_F32);
}
int rrv_transfer_features_batch_u8(rrv_handle h, const int* ids, const float* wts, int n, int ns, uint8_t* out) {
    return transfer_features_batch(h, ids, wts, n, ns, out, OUT_U8);
}

int rrv_release_features(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    for (auto& f : h->features) if (f.owned) { if (f.p) (void)hipFree(f.p); if (f.u8) (void)hipFree(f.u8); }
    for (void* b : h->feat_blocks) (void)hipFree(b);
    h->feat_blocks.clear();
    h->features.clear();
    h->feat_bytes = 0;
    return RRV_OK;
}

int rrv_get_preclamp_image(rrv_handle h, float* out, int H, int W, int b) {
    if (!h || !out) return RRV_E_ARG;
    if (!h->last_pre || h->last_pre_H != H || h->last_pre_W != W) return fail(h, RRV_E_STATE, "get_preclamp: no transfer of that size yet");
    if (b < 0 || b >= h->last_pre_B) return fail(h, RRV_E_ARG, "get_preclamp: the last launch had fewer images");
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    HIPCHK(hipMemcpy(out, h->last_pre + (size_t)b * H * W * 3, (size_t)H * W * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return RRV_OK;
}

int rrv_get_preclamp(rrv_handle h, float* out, int H, int W) { return rrv_get_preclamp_image(h, out, H, W, 0); }

int rrv_sync(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    return sync_all(h);
}

int rrv_set_pipeline(rrv_handle h, int n_slots) {
    if (!h || n_slots < 1 || n_slots > RRV_MAX_SLOTS) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    h->n_slots = n_slots;
    h->next_slot = 0;
    return RRV_OK;
}

int rrv_set_grid_share(rrv_handle h, int share) {
    if (!h || share < 1 || share > 4) return RRV_E_ARG;
    h->grid_share = share;
    return RRV_OK;
}

int rrv_set_f43(rrv_handle h, int mode) {
    if (!h || mode < 0 || mode > 2) return RRV_E_ARG;
    RCHK(sync_all(h));
    h->f43_mode = mode;
    return RRV_OK;
}

int rrv_set_multistyle_group(rrv_handle h, int frames) {
    if (!h || frames < 0 || frames > rrv_ctx::MS_GROUP_MAX) return RRV_E_ARG;
    h->ms_group = frames;
    return RRV_OK;
}

int rrv_set_host_io(rrv_handle h, int mode) {
    if (!h || mode < 0 || mode > 3) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    for (int i = 0; i < 4; ++i) RCHK(retire_ticket(h, i));
    RCHK(sync_all(h));
    h->host_io = mode;
    return RRV_OK;
}

// Debug tap `index` -> its row in ENC_T (enc) or DEC_T: 0..8 encoder, 9..22 decoder, 23..29 encoder twins, 30..32 decoder twins,
// 33..36 the level masks lm[0..3] (the TS_MASK rows, behind the three TS_FRAME rows, which have no tap)
static int tap_row(int index, bool& enc) {
    enc = index < 9 || (index >= 23 && index < 30);
    return index < 9 ? index : index < 23 ? index - 9 : index < 30 ? index - 14 : index < 33 ? index - 16 : index - 13;
}

// Debugging aid (race hunting, tools/device_stream_stress.py): copy activation tensor `index` of workspace slot `slot`
// (0..8 encoder c11 p1 c21 p2 c31 c32 c33 p3 c41, 9..22 decoder d f1 f2 f3 xs4 a4 o4 xs3 a3 o3 xs2 a2 o2 dpart) of the plan
// for (H, W) to the host, ring layout, first image.  *floats = its size; nothing is copied when cap is too small.
int rrv_debug_copy_tensor(rrv_handle h, int slot, int index, int H, int W, float* host, size_t cap, size_t* floats) {
    if (!h || slot < 0 || slot >= RRV_MAX_SLOTS || index < 0 || index > 22 || !floats) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    bool enc;
    const int row = tap_row(index, enc);
    const Tens* t = nullptr;
    for (int k = 0; k < 2 && !t; ++k) {
        EncPlan& e = h->slots[slot].enc[k]; DecPlan& d = h->slots[slot].dec[k];
        if (enc ? (e.H == H && e.W == W && e.B > 0) : (d.H == H / 8 * 8 && d.W == W / 8 * 8 && d.B > 0)) t = enc ? &ENC_T[row].of(e) : &DEC_T[row].of(d);
    }
    if (!t || !t->p) return fail(h, RRV_E_STATE, "debug_copy_tensor: no such tensor in this slot");
    *floats = t->img_floats();
    if (host && cap >= *floats) HIPCHK(hipMemcpy(host, t->p, *floats * sizeof(float), hipMemcpyDeviceToHost));
    return RRV_OK;
}

// Layer-parity tap: tensor `index` (0..22 as above, 23..32 the channel-chunk-major twins q11 q1 q21 q2 q31 q32 q33 qa4 qa3
// qa2, 33..36 the level masks of a masked multi-style launch at stride 1, 2, 4, 8: mask_kernels.h LevelMask) of image `image`,
// as stored.  *layout = 0: ring-layout NHWC [H+2][W+2][C]; 1: P8 [C/8][H+2][W+8][8] (conv_f43.h LAY).
// Refused (RRV_E_STATE) unless the most recent launch on that plan wrote the tensor for that image (a level mask: a masked
// launch, and image 0 only when it had one mask for every image).
int rrv_debug_copy_tensor_ex(rrv_handle h, int slot, int index, int image, int H, int W, float* host, size_t cap, size_t* floats,
                             int* layout, int* channels) {
    if (!h || slot < 0 || slot >= RRV_MAX_SLOTS || index < 0 || index > 36 || image < 0 || !floats) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    bool enc;
    const int row = tap_row(index, enc);
    const int flags = enc ? ENC_T[row].flags : DEC_T[row].flags;
    const Tens* t = nullptr;
    unsigned pgen = 0;
    for (int k = 0; k < 2; ++k) {
        EncPlan& e = h->slots[slot].enc[k]; DecPlan& d = h->slots[slot].dec[k];
        const bool match = enc ? (e.H == H && e.W == W && e.B > 0) : (d.H == H / 8 * 8 && d.W == W / 8 * 8 && d.B > 0);
        const unsigned g = enc ? e.gen : d.gen;
        if (match && (!t || g > pgen)) { t = enc ? &ENC_T[row].of(e) : &DEC_T[row].of(d); pgen = g; }
    }
    if (!t || !t->p) return fail(h, RRV_E_STATE, "debug_copy_tensor_ex: no such tensor in this slot");
    if (t->gen != pgen || pgen == 0) return fail(h, RRV_E_STATE, "debug_copy_tensor_ex: the plan's last launch did not write this tensor");
    if (image >= t->gen_B) return fail(h, RRV_E_STATE, "debug_copy_tensor_ex: the plan's last launch did not write this image");
    const bool p8 = flags & TS_P8;
    const int C = p8 ? (enc ? ENC_T[row].C : DEC_T[row].C) : t->C;
    const size_t n = p8 ? (size_t)(C / 8) * t->img_floats() : t->img_floats();
    if ((size_t)(image + 1) * n > (p8 ? (size_t)t->B / (C / 8) : (size_t)t->B) * n) return fail(h, RRV_E_STATE, "debug_copy_tensor_ex: image beyond the tensor");
    *floats = n;
    if (layout) *layout = p8 ? 1 : 0;
    if (channels) *channels = C;
    if (host && cap >= n) HIPCHK(hipMemcpy(host, t->p + (size_t)image * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return RRV_OK;
}

// Layer-parity read-back (tests/test_gpu_frame_mode_layers.py): the state set image `image` of the last launch on `slot` ran
// with (frame mode: its statistics and predicted filters; grouped multi-style: its blended state), or the style half of the
// filter predictions of prepared style `image`.
int rrv_debug_copy_state(rrv_handle h, int what, int slot, int image, float* out, int n) {
    if (!h || !out || image < 0) return RRV_E_ARG;
    if (what == RRV_DBG_STYLE_PRED) {
        if (slot != 0 || image >= RRV_MAX_STYLES || n != 6 * 32) return RRV_E_ARG;
        const StyleState& S = h->styles[image];
        if (!S.prepared || !S.smean) return fail(h, RRV_E_STATE, "debug_copy_state: prepare_style has not been called for this style");
        HIPCHK(hipSetDevice(h->dev));
        RCHK(sync_all(h));
        HIPCHK(hipMemcpy(out, S.smean, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        return RRV_OK;
    }
    if (what == RRV_DBG_STYLE_BLOB) {      // as it stands: a pass ended by rrv_debug_prep_stop leaves the later entries unwritten
        if (slot != 0 || image >= RRV_MAX_STYLES || n != RRV_STATE_FLOATS) return RRV_E_ARG;
        const StyleState& S = h->styles[image];
        if (!S.prepared || !S.blob) return fail(h, RRV_E_STATE, "debug_copy_state: prepare_style has not been called for this style");
        HIPCHK(hipSetDevice(h->dev));
        RCHK(sync_all(h));
        HIPCHK(hipMemcpy(out, S.blob, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        return RRV_OK;
    }
    if (what != RRV_DBG_STATE_SET || slot < 0 || slot > 1 || image >= rrv_ctx::MS_GROUP_MAX || n != RRV_STATE_FLOATS) return RRV_E_ARG;
    if (!h->slots[slot].set_images) return fail(h, RRV_E_STATE, "debug_copy_state: the slot's last launch kept no per-image state");
    if (image >= h->slots[slot].set_images) return fail(h, RRV_E_STATE, "debug_copy_state: the slot's last launch did not write this image");
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    HIPCHK(hipMemcpy(out, h->slot_sets(slot)[image].active, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return RRV_OK;
}

int rrv_debug_prep_stop(rrv_handle h, int stage) {
    if (!h || stage < -1 || stage >= ST_COUNT) return RRV_E_ARG;
    if (stage < 0 && h->prep_stop >= 0) {
        HIPCHK(hipSetDevice(h->dev));
        RCHK(sync_all(h));
        prep_free(h);
    }
    h->prep_stop = stage;
    return RRV_OK;
}

// Layer-parity tap of the preparation pass (tests/test_gpu_prep_layers.py): one image of a tensor the last rrv_compute under
// rrv_debug_prep_stop kept (index 0..19: the rows of PREP_T), of a sampled frame's stored feature, of the style encoder's plan
// or of a style's map.  Ring layout.
int rrv_debug_copy_prep_tensor(rrv_handle h, int index, int image, float* host, size_t cap, size_t* floats, int* H, int* W, int* C) {
    constexpr int NT = (int)(sizeof(PREP_T) / sizeof(PREP_T[0]));
    static_assert(NT == RRV_DBG_PREP_PATCH, "rerevst_hip.h numbers the rows of PREP_T");
    if (!h || index < 0 || index > RRV_DBG_PREP_MAP || image < 0 || !floats) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    Tens t;
    int first = 0;      // the image t.p holds (a stored feature and a style's map are allocations of their own)
    if (index < NT) {
        t = PREP_T[index].of(h->prep);
    } else if (index == RRV_DBG_PREP_PATCH) {
        t.B = (int)h->patches.size(); t.H = h->patch_h; t.W = h->patch_w; t.C = 512;
        if (image < t.B) { t.p = h->patches[(size_t)image]; first = image; }
        else if (t.B) t.p = h->patches[0];
    } else if (index < RRV_DBG_PREP_MAP) {
        static const size_t enc_row[4] = {0, 2, 4, 8};
        t = ENC_T[enc_row[index - RRV_DBG_PREP_STYLE_C11]].of(h->enc_style);
        t.B = 1;
    } else if (image < RRV_MAX_STYLES && h->styles[image].prepared) {
        t = h->styles[image].map; t.B = image + 1; first = image;
    }
    if (!t.p) return fail(h, RRV_E_STATE, "debug_copy_prep_tensor: the last pass did not allocate this tensor");
    if (image >= t.B) return fail(h, RRV_E_STATE, "debug_copy_prep_tensor: image beyond the batch");
    const size_t n = t.img_floats();
    *floats = n;
    if (H) *H = t.H;
    if (W) *W = t.W;
    if (C) *C = t.C;
    if (host && cap >= n) HIPCHK(hipMemcpy(host, t.p + (size_t)(image - first) * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return RRV_OK;
}

// ---- weight read-back (tests/test_gpu_packs.py) ----------------------------------------------------------------------------------------
// One row per buffer, in the order the header promises.  p: the buffer (a folded KernelFilter's: state set 0's); fold: 0 a checkpoint
// weight, 1 + f / 4 + f the folded down / up weights of KernelFilter f (one buffer per state set).
namespace {
struct WRef { std::string key; int form; const float* p; size_t floats; int Cout, Cin, taps, BN, fold; };
std::vector<WRef> weight_list(rrv_handle h) {
    std::vector<WRef> v;
    auto add = [&](const std::string& key, int form, const float* p, size_t floats, const ConvW& w, int fold = 0) {
        if (p) v.push_back({key, form, p, floats, w.Cout, w.Cin, w.taps, form == RRV_DBG_W_PK ? w.BN : 0, fold});
    };
    for (const auto& kv : h->conv) {
        const ConvW& w = kv.second;
        const size_t n = (size_t)w.Cout * w.Cin;
        add(kv.first, RRV_DBG_W_RAW, w.raw, n * w.taps, w);
        add(kv.first, RRV_DBG_W_PK, w.pk, n * w.taps, w);
        add(kv.first, RRV_DBG_W_PK_WINO, w.pk_wino, n * 16, w);
        add(kv.first, RRV_DBG_W_PK_UPS, w.pk_ups, n * 9, w);
        add(kv.first, RRV_DBG_W_PK_UPS_SC, w.pk_ups_sc, n * Ups5Geo::NUB, w);
        add(kv.first, RRV_DBG_W_PK_F43, w.pk_f43, n * 36, w);
        add(kv.first, RRV_DBG_W_BIAS, w.bias, (size_t)w.Cout, w);
    }
    ConvW first; first.Cout = 64; first.Cin = 3; first.taps = 9;
    for (int which = 0; which < 2; ++which) {
        add(enc_key(which, 0), RRV_DBG_W_FIRST, h->first_w[which], 27 * 64, first);
        if (which == 0) add(enc_key(0, 0), RRV_DBG_W_FIRST_GREY, h->first_wg, 1216, first);
        add(enc_key(which, 0), RRV_DBG_W_BIAS, h->first_b[which], 64, first);
    }
    ConvW last; last.Cout = 3; last.Cin = 64; last.taps = 9;
    add("Decoder.slice1", RRV_DBG_W_LAST, h->last_w, 2 * 4 * 64 * 4, last);
    add("Decoder.slice1", RRV_DBG_W_BIAS, h->last_b, 4, last);
    for (int f = 0; f < 3; ++f) {
        char pre[64];
        snprintf(pre, sizeof pre, "Decoder.Filter%d.fold_", f + 1);
        const ConvW &fd = h->sets[0].fold_down[f], &fu = h->sets[0].fold_up[f];
        add(std::string(pre) + "down", RRV_DBG_W_RAW, fd.raw, (size_t)32 * 512 * 9, fd, 1 + f);
        add(std::string(pre) + "down", RRV_DBG_W_BIAS, fd.bias, 256, fd, 1 + f);
        add(std::string(pre) + "down", RRV_DBG_W_PK_WINO, fd.pk_wino, (size_t)32 * 512 * 16, fd, 1 + f);
        add(std::string(pre) + "up", RRV_DBG_W_RAW, fu.raw, (size_t)512 * 32 * 9, fu, 4 + f);
        add(std::string(pre) + "up", RRV_DBG_W_PK_WINO, fu.pk_wino, (size_t)512 * 32 * 16, fu, 4 + f);
    }
    return v;
}
}  // namespace

int rrv_debug_weight_count(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    if (!h->finalized) return fail(h, RRV_E_STATE, "debug_weight_count: the weights are not finalized");
    return (int)weight_list(h).size();
}

int rrv_debug_weight_info(rrv_handle h, int index, char* key, size_t keycap, int* form, int* Cout, int* Cin, int* taps, int* BN, int* sets,
                          size_t* floats) {
    if (!h) return RRV_E_ARG;
    if (!h->finalized) return fail(h, RRV_E_STATE, "debug_weight_info: the weights are not finalized");
    const std::vector<WRef> v = weight_list(h);
    if (index < 0 || index >= (int)v.size()) return fail(h, RRV_E_ARG, "debug_weight_info: no weight buffer " + std::to_string(index));
    const WRef& r = v[(size_t)index];
    if (key) {
        if (r.key.size() + 1 > keycap) return fail(h, RRV_E_ARG, "debug_weight_info: the key needs " + std::to_string(r.key.size() + 1) + " bytes");
        memcpy(key, r.key.c_str(), r.key.size() + 1);
    }
    if (form) *form = r.form;
    if (Cout) *Cout = r.Cout;
    if (Cin) *Cin = r.Cin;
    if (taps) *taps = r.taps;
    if (BN) *BN = r.BN;
    if (sets) *sets = r.fold ? rrv_ctx::N_SETS : 1;
    if (floats) *floats = r.floats;
    return RRV_OK;
}

int rrv_debug_copy_weights(rrv_handle h, int index, int set, float* host, size_t cap, size_t* floats) {
    if (!h || !floats) return RRV_E_ARG;
    if (!h->finalized) return fail(h, RRV_E_STATE, "debug_copy_weights: the weights are not finalized");
    const std::vector<WRef> v = weight_list(h);
    if (index < 0 || index >= (int)v.size()) return fail(h, RRV_E_ARG, "debug_copy_weights: no weight buffer " + std::to_string(index));
    const WRef& r = v[(size_t)index];
    if (set < 0 || set >= (r.fold ? rrv_ctx::N_SETS : 1)) return fail(h, RRV_E_ARG, "debug_copy_weights: " + r.key + " has no state set " + std::to_string(set));
    const float* p = r.p;
    if (r.fold) {
        const int f = (r.fold - 1) % 3;
        if (!(h->sets[set].folded >> f & 1u))
            return fail(h, RRV_E_STATE, "debug_copy_weights: nothing has folded " + r.key + " of state set " + std::to_string(set));
        const ConvW& w = r.fold <= 3 ? h->sets[set].fold_down[f] : h->sets[set].fold_up[f];
        p = r.form == RRV_DBG_W_RAW ? w.raw : r.form == RRV_DBG_W_BIAS ? w.bias : w.pk_wino;
    }
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    *floats = r.floats;
    if (host && cap >= r.floats) HIPCHK(hipMemcpy(host, p, r.floats * sizeof(float), hipMemcpyDeviceToHost));
    return RRV_OK;
}

int rrv_set_workspace_cap(rrv_handle h, size_t bytes) {
    if (!h || !bytes) return RRV_E_ARG;
    h->ws_cap = bytes;
    return RRV_OK;
}
int rrv_last_compute_info(rrv_handle h, int* groups, int* group_size, size_t* workspace_bytes) {
    if (!h) return RRV_E_ARG;
    if (groups) *groups = h->last_groups;
    if (group_size) *group_size = h->last_group_size;
    if (workspace_bytes) *workspace_bytes = h->last_ws_bytes;
    return RRV_OK;
}

int rrv_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return RRV_E_ARG;
    *out = nullptr;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) return RRV_E_NOMEM;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pin_ranges[(const char*)*out] = bytes;
    return RRV_OK;
}
int rrv_host_free(void* p) {
    if (!p) return RRV_E_ARG;
    { std::lock_guard<std::mutex> lk(g_pin_mu); g_pin_ranges.erase((const char*)p); }
    return hipHostFree(p) == hipSuccess ? RRV_OK : RRV_E_ARG;
}
int rrv_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return RRV_E_ARG;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? RRV_OK : RRV_E_HIP;
}
int rrv_host_unregister(void* p) { return (p && hipHostUnregister(p) == hipSuccess) ? RRV_OK : RRV_E_ARG; }

int rrv_set_caller_stream(rrv_handle h, void* stream, int enable) {
    if (!h) return RRV_E_ARG;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    h->caller_stream = (hipStream_t)stream;
    h->caller_sync = enable != 0;
    return RRV_OK;
}

int rrv_profile_begin(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    for (ProfEntry& e : h->prof) { (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); }
    h->prof.clear();
    (void)sync_all(h);          // profiled launches run un-pipelined on slot 0 so event intervals do not overlap
    h->profiling = true;
    return RRV_OK;
}

int rrv_profile_end(rrv_handle h) {
    if (!h) return RRV_E_ARG;
    h->profiling = false;
    HIPCHK(hipSetDevice(h->dev));
    RCHK(sync_all(h));
    for (ProfEntry& e : h->prof) HIPCHK(hipEventElapsedTime(&e.ms, e.e0, e.e1));
    return RRV_OK;
}

int rrv_profile_count(rrv_handle h) { return h ? (int)h->prof.size() : RRV_E_ARG; }

int rrv_profile_entry(rrv_handle h, int i, const char** name, float* ms, double* flops, double* bytes, double* flops_executed) {
    if (!h || i < 0 || i >= (int)h->prof.size()) return RRV_E_ARG;
    const ProfEntry& e = h->prof[i];
    if (name) *name = e.name.c_str();
    if (ms) *ms = e.ms;
    if (flops) *flops = e.flops;
    if (bytes) *bytes = e.bytes;
    if (flops_executed) *flops_executed = e.flops_exec;
    return RRV_OK;
}

int rrv_profile_entry_grid(rrv_handle h, int i, unsigned* grid, int* xcd_slabs) {
    if (!h || i < 0 || i >= (int)h->prof.size()) return RRV_E_ARG;
    if (grid) *grid = h->prof[i].grid;
    if (xcd_slabs) *xcd_slabs = h->prof[i].xcd_slabs;
    return RRV_OK;
}

}  // extern "C"

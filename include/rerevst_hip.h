/*
 * rerevst_hip.h — C ABI of librerevst_hip.so, the MI355X (gfx950) per-frame stylization
 * path of ReReVST.
 *
 * Every entry point replaces one method of the reference's Python drop-in boundary,
 * class `Stylization` in test/framework.py:56-118 (multi-style twin:
 * "Multi-style Interpolation/stylization.py":42-100).  Plain pointers and sizes only; all
 * image buffers are caller-owned.  A handle owns its device weights, workspace, saved
 * state and one HIP stream; it is NOT thread-safe (the reference model is stateful and
 * non-reentrant as well).  Multi-GPU = one handle per process per GPU.
 *
 * Return value: 0 on success, negative RRV_E_* otherwise; rrv_last_error() gives the text.
 */
#ifndef REREVST_HIP_H
#define REREVST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rrv_ctx* rrv_handle;

enum {
    RRV_OK = 0,
    RRV_E_ARG = -1,        /* bad argument / shape */
    RRV_E_HIP = -2,        /* HIP runtime error */
    RRV_E_WEIGHTS = -3,    /* unknown key, wrong shape, or weights incomplete */
    RRV_E_STATE = -4,      /* transfer before compute()/set_state, compute with no frames, ... */
    RRV_E_NOMEM = -5,      /* out of device (or page-locked host) memory */
    RRV_E_DEBUG = -6,      /* bounds-checked debug mode found a store outside a tensor's valid region */
    RRV_E_COMM = -7,       /* RCCL: library not found, or a communicator / collective call failed */
    RRV_E_DATA = -8        /* JPEG input: a stream the parser refuses, or a frame whose entropy-coded data is corrupt */
};

/* Floats in the per-style shared-state blob: 11 norm layers x {mean,rstd,lo,hi}[C]
 * (2368 channels), 6 dynamic filters [32][32], style (mean,std) for relu1_1..relu4_1
 * (test/style_network_global.py:37-40,148,171,330).  Layout documented in DESIGN.md. */
#define RRV_STATE_FLOATS 17536
#define RRV_MAX_STYLES 8
#define RRV_MAX_SLOTS 4

/* Stylization.__init__ (test/framework.py:57-78): picks the device and builds the model.
 * `device` is the HIP device ordinal. */
int rrv_create(int device, rrv_handle* out);
int rrv_destroy(rrv_handle h);
const char* rrv_last_error(rrv_handle h);

/* model.load_state_dict(torch.load(checkpoint)) (test/framework.py:75): one call per
 * state_dict key used by the inference path (Encoder.*, EncoderStyle.*, Decoder.*; the
 * reference deletes Vgg19.* itself, style_network_global.py:467-469).  `data` is host
 * fp32, OIHW for convolutions / [out,in] for FC, exactly as stored in the checkpoint;
 * repacking to the kernel-native layout happens inside.  rrv_finalize_weights() checks
 * the full key set is present (strict load) and uploads. */
int rrv_load_weight(rrv_handle h, const char* key, const float* data, const int64_t* shape, int ndim);
int rrv_finalize_weights(rrv_handle h);

/* Stylization.prepare_style (test/framework.py:99-104; multi-style stylization.py:71-79).
 * style: uint8 BGR HWC [Hs][Ws][3].  style_id in [0, RRV_MAX_STYLES). */
int rrv_prepare_style(rrv_handle h, const uint8_t* style_bgr, int Hs, int Ws, int style_id);

/* Stylization.clean (test/framework.py:93-95). */
int rrv_clean(rrv_handle h);

/* Stylization.add (test/framework.py:82-86): encode one sampled frame (uint8 BGR HWC,
 * UNPADDED as the driver passes it, generate_real_video.py:139-143) and keep its
 * relu4_1 feature.  All frames added between clean() and compute() must share H, W. */
int rrv_add(rrv_handle h, const uint8_t* frame_bgr, int H, int W);

/* Stylization.compute (test/framework.py:88-91): batched decoder pass over the added
 * frames that records the saved statistics / dynamic filters for every prepared style. */
int rrv_compute(rrv_handle h);

/* Memory policy of rrv_compute.  Decoder.compute as written keeps every sampled frame's decoder activations resident
 * (O(B * 64 * H * W) floats at the last level; the reference authors' own long-sequence sketch streams them through a
 * disk cache, test/style_network.py:597-624).  When that workspace would exceed `bytes` (default 64 GiB) rrv_compute
 * STREAMS instead: one sync point (normalisation layer / filter prediction) at a time, groups of G frames re-run the
 * decoder prefix from their relu4_1 features and contribute partial statistics (sum, centred square sum, min, max;
 * pairwise merge in fp64) — workspace = one group, independent of B; the state blob equals the resident one to
 * rounding.  rrv_last_compute_info reports what the last rrv_compute did. */
int rrv_set_workspace_cap(rrv_handle h, size_t bytes);
int rrv_last_compute_info(rrv_handle h, int* groups, int* group_size, size_t* workspace_bytes);

/* The saved state of one style as a flat blob (what an RCCL broadcast ships to the other
 * ranks, and what the golden fixtures compare).  n must be RRV_STATE_FLOATS. */
int rrv_get_state(rrv_handle h, float* out, int n, int style_id);
int rrv_set_state(rrv_handle h, const float* in, int n, int style_id);

/* Multi-GPU (one process and one handle per GPU; the reference has no distributed code — SURVEY 8(e)): frames are
 * independent once the saved state exists, so the only collective is ONE ncclBroadcast of the blob per style and video,
 * from the rank that ran prepare_style / add / compute.  rrv_broadcast_state issues it on the handle's stream over an
 * ordinary ncclComm_t (pass the application's own, e.g. MPI- or torch-built, as void*); on the other ranks the style
 * then is exactly as after rrv_set_state.  librccl.so is opened on first use (RRV_RCCL_PATH overrides the search).
 * The three rrv_comm_* helpers build a communicator for callers without RCCL bindings (ctypes, cgo, JNI): rank 0 calls
 * rrv_comm_unique_id, ships the 128 bytes to the others by any means, every rank calls rrv_comm_init_rank. */
int rrv_comm_unique_id(char id[128]);
int rrv_comm_init_rank(rrv_handle h, const char id[128], int nranks, int rank, void** comm);
int rrv_comm_destroy(void* comm);
int rrv_broadcast_state(rrv_handle h, void* comm, int root, int my_rank, int style_id);

/* Stylization.transfer (test/framework.py:106-118): uint8 BGR HWC [H][W][3] in host
 * memory -> float32 BGR HWC [H][W][3] in 0..255 in host memory (includes the H2D / D2H crossings of
 * framework.py:109 `.to(device)` and :40 `.cpu()`).  Any H, W >= 8: as in the reference the three max pools floor the
 * size, so out_bgr is [Ho][Wo][3] with Ho = 8*(H/8), Wo = 8*(W/8) (= [H][W][3] for the multiples of 64 the reference
 * driver produces); (H+2)*(W+2)*64 < 2^31 (about 33 Mpixel per frame; RRV_E_ARG beyond).  The same holds for every
 * other transfer entry (batch, device, blend, features, frame mode).  Page-locked caller buffers (rrv_host_alloc / rrv_host_register)
 * are DMA'd directly; pageable ones are staged through the library's own pinned buffers. */
int rrv_transfer(rrv_handle h, const uint8_t* frame_bgr, int H, int W, float* out_bgr);

/* Look-ahead form of rrv_transfer for a one-frame-per-call driver loop (test/generate_real_video.py:152-171 calls
 * framework.transfer once per frame): rrv_transfer_async queues the frame and returns a ticket at once;
 * rrv_transfer_wait(ticket) blocks until `out_bgr` of that call is filled.  Up to FOUR tickets may be open (a fifth
 * submission first completes the oldest): each runs on its own stream and workspace with a quarter of the CUs per
 * launch, so four frames run side by side instead of queueing behind each other's partially filled last round of
 * workgroups.  The frame is copied to the device on the ticket's own stream (one H2D copy; no separate copy streams)
 * and the last kernel writes the result to page-locked host memory directly (the caller's buffer if it is page-locked,
 * the library's staging otherwise).  Keeping three frames submitted ahead of the one collected gives 551 frames/s at
 * 512x512 and 1418 at 256x256 against 431 / 868 for rrv_transfer.
 * `frame_bgr` may be reused as soon as the call returns (a pageable frame has been copied to staging by then; for a
 * page-locked one the call waits for its H2D copy); `out_bgr` must stay valid until its ticket is waited for.
 * Bit-identical to rrv_transfer. */
int rrv_transfer_async(rrv_handle h, const uint8_t* frame_bgr, int H, int W, float* out_bgr, long* ticket);
int rrv_transfer_wait(rrv_handle h, long ticket);

/* Same computation on device-resident buffers (HBM in, HBM out), asynchronous on the
 * handle's own (non-blocking) streams; rrv_sync() waits.
 * ORDERING: the library's streams are NOT ordered against any stream of the caller.  Either (a) make sure the input
 * is complete before the call (e.g. torch.cuda.synchronize()) and call rrv_sync() before reading the output, or
 * (b) register the producing / consuming stream once with rrv_set_caller_stream(): every *_device entry then waits
 * for the work queued on that stream so far and makes that stream wait for its own output (event based, no host
 * sync), i.e. the call behaves as if it had been enqueued on the caller's stream. */
int rrv_transfer_device(rrv_handle h, const void* d_frame_bgr_u8, int H, int W, void* d_out_bgr_f32);

/* B frames per launch ([B][H][W][3] in, [B][H][W][3] out, both in HBM): frames are independent
 * once the state exists (test/style_network_global.py:499-501), so batching only widens every
 * kernel's grid -- it removes the workgroup-quantisation loss of the small layers.
 * rrv_transfer_device(h, in, H, W, out) == rrv_transfer_batch_device(h, in, 1, H, W, out). */
int rrv_transfer_batch_device(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_f32);

/* Multi-style transfer (stylization.py:94-100 + style_network.py:432-460): every saved
 * quantity is replaced by sum_s weight[s]*q_s before the same forward.  Device buffers. */
int rrv_transfer_blend_device(rrv_handle h, const void* d_frame_bgr_u8, int H, int W,
                              const float* style_weight, int n_styles, void* d_out_bgr_f32);

/* Host-buffer forms of the two entries above (H2D copy, same device path, D2H copy). */
int rrv_transfer_batch(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, float* out_bgr);
int rrv_transfer_blend(rrv_handle h, const uint8_t* frame_bgr, int H, int W, const float* style_weight, int n_styles,
                       float* out_bgr);

/* The reference driver's ReshapeTool + crop on the device (test/generate_real_video.py:61-83 process: reflect-pad
 * 64 px on every side and up to a multiple of 64, cv2.BORDER_REFLECT; :167 crop [64:64+H, 64:64+W]): UNPADDED
 * [B][H][W][3] uint8 frames in, [B][H][W][3] float32 stylized frames out.  The padded frame never exists: the first
 * kernel reads the source through the reflection, the last one writes only the crop window.  Bit-identical to
 * pad -> rrv_transfer_batch -> crop for a fixed kernel choice (rrv_set_f43 mode 0 / 2; in the default mode 1 the choice
 * follows the launch geometry, and the crop window is one).  _device: HBM buffers, asynchronous; the host form pipelines sub-batches. */
int rrv_transfer_frames_device(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_f32);
int rrv_transfer_frames(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, float* out_bgr);

/* Multi-style feature API ("Multi-style Interpolation/stylization.py"): generate_content_features :87-92
 * (encode a frame once; the reference caches the tensor on disk, test.py:87-101 — here it stays in HBM and
 * an integer id is returned), add_patch :66-67 (sample a cached feature for the statistics pass; then
 * rrv_compute == compute_norm :81-83), transfer(feature, style_weight) :94-100 (decoder only, blended state).
 * rrv_release_features frees the cache. */
int rrv_generate_content_features(rrv_handle h, const uint8_t* frame_bgr, int H, int W, int* feature_id);
/* The caching pass of a run of frames (test.py:87-101 encodes every frame of the video once) in ONE call: frames_bgr[B][H][W][3],
 * feature_ids[B] out.  Sub-batches are pipelined inside (copy-in stream + two compute streams, several frames per encoder
 * launch, the per-frame path's kernel choice — rrv_set_f43), and the encoder's last layer stores straight into the cache
 * (one arena per call): no allocation, device copy or host wait per frame.  Frames beyond the cache cap are kept as pixels. */
int rrv_generate_content_features_batch(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, int* feature_ids);
int rrv_add_patch(rrv_handle h, int feature_id);
int rrv_transfer_features(rrv_handle h, int feature_id, const float* style_weight, int n_styles, float* out_bgr);
/* n cached features with one weight vector each (style_weight[n][n_styles], out_bgr[n][H][W][3]) in one call — what the
 * reference driver's loop does frame by frame (test.py:127-131) — pipelined inside: consecutive frames alternate over
 * two (stream, workspace, blended-state) sets and the D2H copy of one frame overlaps the next frame's kernels. */
int rrv_transfer_features_batch(rrv_handle h, const int* feature_ids, const float* style_weight, int n, int n_styles, float* out_bgr);
int rrv_release_features(rrv_handle h);
/* Frames per launch sequence of rrv_transfer_features_batch: 1..16, or 0 (default) = by the frame size, ~6.6 Mpixel per
 * launch as in the single-style host entries (4 at 1152 x 1152, 16 at 640 x 640 and below).  With more than one, every
 * image of a launch carries its own blended state set (per-image normalisation parameters and folded KernelFilter
 * weights), which widens every layer's grid and lets the kernel choice (rrv_set_f43) count the group's frames; with a
 * fixed kernel mode the results are bit-identical for every setting.  Measured with four styles in the default mode
 * (round 5, conv_f43_k with per-image parameters), frames/s for 1 / 2 / 4 per launch: 1152 x 1152 371 / 382 / 381,
 * 640 x 640 941 / 1070 / 1167, 384 x 384 1750 / 2163 / 2590. */
int rrv_set_multistyle_group(rrv_handle h, int frames);

/* Kernel choice for the same-resolution 3x3 layers of the per-frame path that have a Winograd F(4x4,3x3) pack (conv_f43_k):
 * encoder conv1_2 .. conv3_4 (test/style_network_global.py:271-281) and the three ResidualBlock.conv2 (:104,119-122).
 * mode 0 = always F(2x2,3x3); 1 (default, also RRV_F43=) = F(4x4,3x3) where the launch geometry lets it win: a rule on the
 * layer, the frames per launch, the frame size and the CUs the launch may use (the device's CU count under HSA_CU_MASK /
 * RRV_CUS, divided by the grid share of the look-ahead tickets) — from four 640 x 640 frames per launch on every packed layer,
 * from two 1152 x 1152 frames, from one where the items are long; 1.25-1.38x per layer, +16 % frames/s at 512 x 512;
 * 2 = always F(4x4,3x3).  The preparation pass (prepare_style / add / compute) and the frame mode always run F(2x2,3x3).
 * RRV_F43_LAYERS (bit 0..6 = encoder conv1_2 .. conv3_4, bit 7..9 = slice4 / slice3 / slice2 .conv2; default all ten) narrows
 * the set.  In mode 1 a state whose dynamic filters are far from the O(1) scale (Frobenius norm above 4 sqrt 32: ill-conditioned
 * in float32 whoever evaluates it) keeps the seven encoder layers on F(2x2,3x3).  F(4x4,3x3) makes 1.4x the rounding error of
 * F(2x2,3x3): worst pre-clamp error over 32 inputs x 4 weight sets <= 0.73 of the stated bound in the default mode
 * (profiles/r05_parity_margin.txt).  In mode 1 a frame's low-order bits therefore depend on how it was submitted; with a fixed
 * mode every single-style entry delivers the same bits for the same frame, and every mode is run-to-run deterministic.  The
 * one-frame feature cache entry (rrv_generate_content_features) always runs F(2x2,3x3); rrv_generate_content_features_batch
 * and the grouped per-image-state launches (rrv_set_multistyle_group > 1) follow the mode. */
int rrv_set_f43(rrv_handle h, int mode);
/* Capacity policy of the feature cache (default 64 GiB).  The reference spills every frame's feature to disk
 * (test.py:87-101, cache/%d.pt), so its video length is unbounded; here a cached feature costs 42 MB of HBM per
 * 1152x1152 frame.  Once the cache would exceed `bytes`, rrv_generate_content_features keeps the frame's uint8 pixels
 * instead (a tenth of the size) and every use of that feature re-runs the encoder first (rrv_transfer_features[_batch]
 * = encoder + blended decoder, rrv_add_patch encodes on the spot) — slower, never an out-of-memory error.
 * rrv_feature_cache_info: cached features, spilled ones, bytes held by the cached ones. */
int rrv_set_feature_cache_cap(rrv_handle h, size_t bytes);
int rrv_feature_cache_info(rrv_handle h, int* resident, int* spilled, size_t* bytes);

/* Stylization(checkpoint, cuda, use_Global=False).transfer (test/framework.py:69-72,106-118 with
 * test/style_network_frame.py): per-frame InstanceNorm statistics (:39-43) and per-frame filter
 * prediction (:53-62,97-105); needs only rrv_prepare_style (style 0), whose saved state is not touched.  Host buffers. */
int rrv_transfer_frame_mode(rrv_handle h, const uint8_t* frame_bgr, int H, int W, float* out_bgr);

/* The same model for B frames per call, with the shapes of the global entries: _batch as rrv_transfer_batch (any
 * H, W >= 8, [B][8*(H/8)][8*(W/8)][3] out), _frames as rrv_transfer_frames (UNPADDED frames, reflect pad and crop on
 * the device, [B][H][W][3] out).  Each frame gets its own statistics and predicted filters in its own state set, in
 * launch sequences of up to 16 frames; frame b's output is bit-identical to rrv_transfer_frame_mode on that frame
 * alone (of its padded form for _frames), in every rrv_set_f43 mode: frame mode runs F(2x2,3x3) throughout.
 * _device: HBM buffers, B in 1..64, asynchronous, alternating over workspace slots 0 and 1, ordered by
 * rrv_set_caller_stream.  Host forms: sub-batches of at most 16 frames through the staging pipeline
 * (rrv_set_host_io applies).  Need rrv_prepare_style (style 0), else RRV_E_STATE; style 0's saved state is not
 * touched.  Scratch per workspace slot and frame size: 3 x 64 x 8*(H/8) doubles per frame plus 20 rows of slack. */
int rrv_transfer_frame_mode_batch_device(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_f32);
int rrv_transfer_frame_mode_batch(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, float* out_bgr);
int rrv_transfer_frame_mode_frames_device(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_f32);
int rrv_transfer_frame_mode_frames(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, float* out_bgr);

/* uint8 output: every entry that writes a stylized frame has a _u8 twin with the same arguments, except that the output
 * is uint8 BGR HWC, the same [.][Ho][Wo][3] elements, one byte each (a quarter of the float32 bytes over PCIe, in
 * staging and in HBM).  The last kernel computes the float32 value exactly as the float twin does, rounds it half to
 * even (rintf, as numpy's np.rint) and stores the byte; the value is already clamped to 0..255.  So each twin's output is
 * identical to to_uint8(float twin's output) = np.clip(np.rint(x), 0, 255).astype(np.uint8) (cv2.imwrite's conversion),
 * bit for bit, on the same inputs with the same frames per call.  Errors, staging, page-locked buffers, rrv_set_host_io,
 * tickets and rrv_get_preclamp_image behave as for the float twin; rrv_transfer_wait collects rrv_transfer_async_u8 tickets. */
int rrv_transfer_u8(rrv_handle h, const uint8_t* frame_bgr, int H, int W, uint8_t* out_bgr);       /* == to_uint8(rrv_transfer) */
int rrv_transfer_async_u8(rrv_handle h, const uint8_t* frame_bgr, int H, int W, uint8_t* out_bgr, long* ticket);   /* == to_uint8(rrv_transfer_async) */
int rrv_transfer_batch_u8(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, uint8_t* out_bgr);   /* == to_uint8(rrv_transfer_batch) */
int rrv_transfer_frames_u8(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, uint8_t* out_bgr);  /* == to_uint8(rrv_transfer_frames) */
int rrv_transfer_device_u8(rrv_handle h, const void* d_frame_bgr_u8, int H, int W, void* d_out_bgr_u8);      /* == to_uint8(rrv_transfer_device) */
int rrv_transfer_batch_device_u8(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_u8);   /* == to_uint8(rrv_transfer_batch_device) */
int rrv_transfer_frames_device_u8(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_u8);  /* == to_uint8(rrv_transfer_frames_device) */
int rrv_transfer_blend_u8(rrv_handle h, const uint8_t* frame_bgr, int H, int W, const float* style_weight, int n_styles,
                          uint8_t* out_bgr);                                                                   /* == to_uint8(rrv_transfer_blend) */
int rrv_transfer_blend_device_u8(rrv_handle h, const void* d_frame_bgr_u8, int H, int W,
                                 const float* style_weight, int n_styles, void* d_out_bgr_u8);                /* == to_uint8(rrv_transfer_blend_device) */
int rrv_transfer_features_u8(rrv_handle h, int feature_id, const float* style_weight, int n_styles, uint8_t* out_bgr);   /* == to_uint8(rrv_transfer_features) */
int rrv_transfer_features_batch_u8(rrv_handle h, const int* feature_ids, const float* style_weight, int n, int n_styles,
                                   uint8_t* out_bgr);                                                          /* == to_uint8(rrv_transfer_features_batch) */
int rrv_transfer_frame_mode_u8(rrv_handle h, const uint8_t* frame_bgr, int H, int W, uint8_t* out_bgr);     /* == to_uint8(rrv_transfer_frame_mode) */
int rrv_transfer_frame_mode_batch_u8(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, uint8_t* out_bgr);   /* == to_uint8(rrv_transfer_frame_mode_batch) */
int rrv_transfer_frame_mode_batch_device_u8(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_u8);   /* == to_uint8(rrv_transfer_frame_mode_batch_device) */
int rrv_transfer_frame_mode_frames_u8(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, uint8_t* out_bgr);  /* == to_uint8(rrv_transfer_frame_mode_frames) */
int rrv_transfer_frame_mode_frames_device_u8(rrv_handle h, const void* d_frames_bgr_u8, int B, int H, int W, void* d_out_bgr_u8);  /* == to_uint8(rrv_transfer_frame_mode_frames_device) */

/* Torch-pipeline forms of the device entries: one descriptor-based entry for the image layouts and value spaces a torch
 * pipeline holds.  An image is described by its element type, layout and value space:
 *   dtype  RRV_DT_U8 (uint8) | RRV_DT_F32 (float32)
 *   layout RRV_LAY_HWC_BGR ([B][H][W][3] BGR, cv2's) | RRV_LAY_CHW_RGB ([B][3][H][W] RGB, torch's NCHW), contiguous
 *   space  RRV_SP_PIXEL (0..255) | RRV_SP_UNIT (0..1) | RRV_SP_NORM (test/framework.py transform_image: (x/255 - mean)/std)
 * uint8 is PIXEL only.  The output's spaces: PIXEL float32 = rrv_transfer_batch_device's values; PIXEL uint8 = the _u8
 * twin's; UNIT = the clamped value the PIXEL form multiplies by 255 (UNIT * 255.0f == PIXEL, bit for bit); NORM = the
 * pre-clamp network output (rrv_get_preclamp_image), i.e. the output of the reference's `self.model(frame)` for a NORM input.
 * Bit-identity of the input forms: every form is converted to the normalised value the uint8 path computes from px, so
 * a frame derived from uint8 px the reference's way gives the uint8 path's output bit for bit: float32 PIXEL (float)px;
 * UNIT (float)px / 255.0f (correctly rounded, as numpy's float32 division); NORM ((float)px / 255.0f - mean) / std in
 * float32 with mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225); any uint8 layout.  An output layout changes
 * only where the values go.
 * flags: RRV_TF_PAD_CROP = the geometry of rrv_transfer_frames_device (UNPADDED [B][H][W] frames in, reflect pad and crop
 * on the device, [B][H][W] out); else that of rrv_transfer_batch_device ([B][8*(H/8)][8*(W/8)] out).  RRV_TF_FRAME_MODE =
 * the frame-mode model of rrv_transfer_frame_mode_{batch,frames}_device (needs rrv_prepare_style).  Shape limits, slots and
 * errors are those entries': B in 1..64, (H+2)*(W+2)*64 < 2^31 for the padded geometry.  An invalid descriptor (uint8 with
 * UNIT or NORM, an unknown value) or flag is RRV_E_ARG, and the handle stays usable.
 * hip_stream != NULL: the call behaves as if it were enqueued on that stream (the events of rrv_set_caller_stream, for this
 * call only: no host sync); NULL: the ordering of the other *_device entries, unless flags has RRV_TF_ON_STREAM, which
 * orders the call on hip_stream whatever its value, NULL being the null stream (torch's default stream). */
typedef struct { int dtype; int layout; int space; } rrv_image_desc;
#define RRV_DT_U8 0
#define RRV_DT_F32 1
#define RRV_LAY_HWC_BGR 0
#define RRV_LAY_CHW_RGB 1
#define RRV_SP_PIXEL 0
#define RRV_SP_UNIT 1
#define RRV_SP_NORM 2
#define RRV_TF_PAD_CROP 1      /* unpadded frames in, crop window out (ReshapeTool + crop on the device) */
#define RRV_TF_FRAME_MODE 2    /* use_Global=False model (per-frame statistics); needs rrv_prepare_style */
#define RRV_TF_ON_STREAM 4     /* order on hip_stream also when it is NULL (the null stream) */
int rrv_transfer_image_device(rrv_handle h, const void* d_in, rrv_image_desc in, int B, int H, int W,
                              void* d_out, rrv_image_desc out, int flags, void* hip_stream);

/* Multi-style interpolation from FRAMES, batched ("Multi-style Interpolation/stylization.py":94-100 transfer(feature, style_weight)
 * with style_network.py:35-53,135-139,348-360 — every saved statistic, dynamic filter and style (mean, std) replaced by
 * sum_s weight[s] * q_s — and :432-460, the forward pass; the reference blends one cached feature per call, test.py:127-131).
 * rrv_transfer_image_device with one weight vector per image: style_weight is [B][n_styles] float32, n_styles in
 * 1..RRV_MAX_STYLES, every style 0..n_styles-1 computed (else RRV_E_STATE).  The frames run in launch sequences of up to sixteen,
 * each image with its own blended state set (as rrv_transfer_features_batch), encoder and decoder from the frames; consecutive
 * calls alternate over workspace slots 0 and 1.  For a fixed kernel mode (rrv_set_f43 0 / 2) image b's output is bit-identical
 * to rrv_transfer_blend on that frame alone with style_weight[b] (of its padded form with RRV_TF_PAD_CROP).
 * flags: RRV_TF_PAD_CROP, RRV_TF_ON_STREAM as above; RRV_TF_FRAME_MODE is RRV_E_ARG (the reference's frame-mode model has no
 * blended state).  RRV_TF_WEIGHTS_DEVICE: style_weight points to device memory, produced on hip_stream (or complete before the
 * call): a blend kernel reads it there, in stream order, and the host never sees the values — weights computed on the GPU need
 * no synchronisation and no copy.  Without it style_weight is host memory, read before the call returns (the weights travel in
 * the blend kernel's argument, a launch sequence's rows at a time: no copy, no host synchronisation and no workspace); the same
 * float32 values give the same bits either way. */
#define RRV_TF_WEIGHTS_DEVICE (1 << 3)   /* = 8, next to RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE | RRV_TF_ON_STREAM */
int rrv_transfer_image_blend_device(rrv_handle h, const void* d_in, rrv_image_desc in, int B, int H, int W,
                                    const float* style_weight, int n_styles,
                                    void* d_out, rrv_image_desc out, int flags, void* hip_stream);
/* The same model on host buffers (stylization.py:94-100, style_network.py:35-53,135-139,348-360,432-460), pipelined as
 * rrv_transfer_batch (pad_crop == 0: [B][8*(H/8)][8*(W/8)][3] out) / rrv_transfer_frames (pad_crop != 0: UNPADDED frames, reflect
 * pad and crop on the device, [B][H][W][3] out): uint8 BGR HWC frames in, float32 BGR out — the _u8 twin: uint8, == to_uint8 of
 * the float form — any B >= 1 in sub-batches of at most sixteen frames through the same staging sets and copy streams;
 * style_weight[B][n_styles] in host memory. */
int rrv_transfer_blend_batch(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W,
                             const float* style_weight, int n_styles, int pad_crop, float* out_bgr),
    rrv_transfer_blend_batch_u8(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W,
                                const float* style_weight, int n_styles, int pad_crop, uint8_t* out_bgr);

/* Multi-style interpolation with weights that vary PER PIXEL ("Multi-style Interpolation/stylization.py":94-100 transfer(feature,
 * style_weight) with style_network.py:35-53 mean / rstd / min / max, :135-139 the dynamic filters, :348-360 the style moments, and the
 * forward pass :432-460 — the reference blends each saved quantity q as sum_s w_s q_s once per frame; here w is a mask).
 * d_mask: float32 [mask_images][n_styles][H][W] in device memory, planar and contiguous, at the resolution of the frames as passed
 * (with RRV_TF_PAD_CROP the UNPADDED frame: the mask is reflect-padded on the device exactly as the frame is); mask_images = B (one
 * mask per frame) or 1 (one mask for every frame); n_styles in 1..RRV_MAX_STYLES, every style 0..n_styles-1 computed (else
 * RRV_E_STATE).  Nothing normalises the mask.  For a decoder tensor at stride r = 1, 2, 4, 8 of the network's input frame m_s(p) is
 * the float32 mean of M[s] over the r x r input pixels that tensor pixel p covers (successive 2 x 2 means, a fixed order), and the
 * decoder forward uses q(p) = sum_s m_s(p) q_s wherever style_network.py:432-460 uses q: clamp((x - mean(p)) rstd(p), lo(p), hi(p)),
 * the AdaIN affine * std(p) + mean(p), and apply_filter with F1(p) on down_sample's output before the LeakyReLU and F2(p) on the result
 * before the upsample convolution.  The encoder does not see the mask.  A mask constant over the frame (M[s] == w_s) is
 * rrv_transfer_image_blend_device with style_weight = w in real arithmetic; in float32 the two differ by rounding, since this entry
 * runs the decoder unfused (the frame mode's kernels, F(2x2,3x3) in every rrv_set_f43 mode) in launch sequences of up to sixteen
 * frames: image b's output does not depend on the batch it rides in, bit for bit.  The saved states are only read.
 * The mask is read in stream order (hip_stream / RRV_TF_ON_STREAM as for rrv_transfer_image_device): a mask computed on the GPU needs
 * no synchronisation.  flags: RRV_TF_PAD_CROP, RRV_TF_ON_STREAM; RRV_TF_FRAME_MODE is RRV_E_ARG, as are mask_images not in {1, B},
 * n_styles out of range and a null mask; the handle stays usable.  All image descriptors of rrv_transfer_image_device, in and out.
 * Consecutive calls alternate over workspace slots 0 and 1.  Workspace per slot and frame size: 8 x 85/64 floats per pixel and frame. */
int rrv_transfer_image_mask_device(rrv_handle h, const void* d_in, rrv_image_desc in, int B, int H, int W,
                                   const float* d_mask, int n_styles, int mask_images,
                                   void* d_out, rrv_image_desc out, int flags, void* hip_stream);
/* The same model on host buffers (stylization.py:94-100, style_network.py:35-53,135-139,348-360,432-460), pipelined as
 * rrv_transfer_blend_batch (pad_crop == 0: [B][8*(H/8)][8*(W/8)][3] out; != 0: UNPADDED frames, reflect pad and crop on the device,
 * [B][H][W][3] out): uint8 BGR HWC frames in, float32 BGR out — the _u8 twin: uint8, == to_uint8 of the float form — any B >= 1 in
 * sub-batches of at most sixteen frames; mask[mask_images][n_styles][H][W] in host memory, each sub-batch's part copied to HBM in
 * front of its kernels. */
int rrv_transfer_mask_batch(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W,
                            const float* mask, int n_styles, int mask_images, int pad_crop, float* out_bgr),
    rrv_transfer_mask_batch_u8(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W,
                               const float* mask, int n_styles, int mask_images, int pad_crop, uint8_t* out_bgr);

/* 8-bit YUV 4:2:0 output for video encoders (ffmpeg over a pipe, VCN / AMF, libx264, libaom): the colour transform and the 2 x 2
 * chroma subsampling run in the last kernel's store, 1.5 bytes per pixel leave the GPU and the host touches no pixel.
 * Arithmetic.  R, G, B are the float32 PIXEL values of the stylized pixel (what the float32 entry delivers, before any rounding) and
 * m[3][4] a conversion matrix: rows Y, Cb, Cr; columns the coefficients of R, G, B and an offset.
 *   c_k = ((m[k][0]*R + m[k][1]*G) + m[k][2]*B) + m[k][3]      every product and sum rounded to float32, in this order, no fused multiply-add
 *   Y byte  = rint(min(max(c_0, 0), 255)), half to even as the _u8 forms round; one per output pixel
 *   chroma  planes of CH = (OH+1)/2 rows and CW = (OW+1)/2 columns for the OH x OW frame the entry delivers.  Sample (i, j) covers output
 *           pixels (2i..2i+1, 2j..2j+1): ((tl + tr) + (bl + br)) * 0.25f of the unrounded, unclamped c_1 (then c_2) in float32 in that
 *           order, then rint(min(max(., 0), 255)).  A pixel of the block outside the frame (the last row / column of an odd OH / OW,
 *           so only in the pad / crop geometry) takes the value of its nearest pixel of the block inside; the padding is never
 *           read.  The mean sites the chroma at the block centre: Y4M's C420jpeg.
 * So a YUV entry's bytes are this arithmetic applied to its float32 twin's output for the same frames and frames per call, bit for bit.
 * Frame layout, all uint8, frame_bytes = OH*OW + 2*CH*CW, frame b of a call at b * frame_bytes with nothing in between:
 *   RRV_LAY_I420  [Y: OH*OW][Cb: CH*CW][Cr: CH*CW]                RRV_LAY_NV12  [Y: OH*OW][CbCr interleaved: CH*CW*2]
 * rrv_yuv_matrix fills m for a standard (Kr, Kb = 0.299, 0.114 for BT.601; 0.2126, 0.0722 for BT.709; Kg = 1 - Kr - Kb) and range — full:
 * Y = Kr R + Kg G + Kb B, Cb = 128 + (B - Y) / (2 (1 - Kb)), Cr = 128 + (R - Y) / (2 (1 - Kr)); limited: Y' = 16 + (219/255) Y and the
 * chroma differences times 224/255 — each coefficient evaluated in double and rounded once to float32; it needs no handle and no GPU.
 * rrv_set_yuv_matrix installs any twelve finite floats (else RRV_E_ARG); NULL restores the default, BT.601 limited range, which is what
 * players assume for untagged yuv420p.  The matrix is handle state read when a call launches its last kernel; workspaces and saved state
 * do not see it.
 * Host entries, pipelined as their float twins (staging, page-locked buffers and rrv_set_host_io apply), any B >= 1, layout = RRV_LAY_I420
 * or RRV_LAY_NV12 (anything else is RRV_E_ARG, the handle stays usable):
 *   rrv_transfer_yuv              flags within RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE (else RRV_E_ARG): rrv_transfer_batch / _frames and
 *                                 rrv_transfer_frame_mode_batch / _frames
 *   rrv_transfer_blend_batch_yuv  rrv_transfer_blend_batch            rrv_transfer_mask_batch_yuv  rrv_transfer_mask_batch
 * Device entries: rrv_transfer_image_device, _blend_device and _mask_device take out.layout = RRV_LAY_I420 / RRV_LAY_NV12 with
 * out.dtype == RRV_DT_U8 and out.space == RRV_SP_PIXEL (anything else, and either layout for the input, is RRV_E_ARG); all flags and
 * input forms as before.  rrv_get_preclamp_image works as after the float twin.
 * Not offered: tickets (rrv_transfer_async), the cached-feature entries (rrv_transfer_features[_batch]) and the one-frame
 * rrv_transfer_blend[_device] and rrv_transfer_frame_mode.  The rrv_image_desc entries still refuse RRV_LAY_I420 / RRV_LAY_NV12 as an INPUT
 * layout (RRV_E_ARG): 8-bit YUV frames enter through the rrv_*_from_yuv entries below (or through an rrv_image_view, which names any layout). */
enum {                         /* output-only values of rrv_image_desc.layout (and the in_layout of the _from_yuv entries), after RRV_LAY_HWC_BGR = 0 and RRV_LAY_CHW_RGB = 1 */
    RRV_LAY_I420 = 2,          /* planar Y, Cb, Cr (ffmpeg's yuv420p) */
    RRV_LAY_NV12 = 3           /* planar Y, then interleaved Cb Cr */
};
enum { RRV_YUV_BT601 = 0, RRV_YUV_BT709 = 1 };      /* rrv_yuv_matrix's standards */
int rrv_yuv_matrix(int standard, int full_range, float m[12]);
int rrv_set_yuv_matrix(rrv_handle h, const float m[12]);
int rrv_transfer_yuv(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W, int flags, int layout, uint8_t* out_yuv);
int rrv_transfer_blend_batch_yuv(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W,
                                 const float* style_weight, int n_styles, int pad_crop, int layout, uint8_t* out_yuv);
int rrv_transfer_mask_batch_yuv(rrv_handle h, const uint8_t* frames_bgr, int B, int H, int W,
                                const float* mask, int n_styles, int mask_images, int pad_crop, int layout, uint8_t* out_yuv);

/* 8-bit YUV 4:2:0 INPUT (a hardware decoder's NV12, ffmpeg's yuv420p, a .y4m file): the first kernel reads Y, Cb and Cr, 1.5 bytes per pixel
 * cross PCIe instead of 3, and the host converts nothing.  With a YUV output the decoder -> stylize -> encoder loop touches no pixel on the host.
 * Input frame, all uint8, for an H x W frame as passed: CH = (H+1)/2, CW = (W+1)/2, frame_bytes = H*W + 2*CH*CW, frame b at b * frame_bytes;
 * RRV_LAY_I420 [Y: H*W][Cb: CH*CW][Cr: CH*CW], RRV_LAY_NV12 [Y: H*W][CbCr interleaved: CH*CW*2] — exactly the layouts the output entries write.
 * Arithmetic.  Pixel (y, x) takes Y[y][x] and the chroma sample (y >> 1, x >> 1): chroma is replicated over its 2 x 2 block, the adjoint of the
 * output's box mean for C420jpeg siting.  (The content encoder folds a frame to one grey value per pixel — RGB2Gray, test/style_network_global.py
 * :487-497 — so a better chroma interpolation would not be visible in the result.)  n[3][4] is a conversion matrix: rows R, G, B; columns the
 * coefficients of Y, Cb, Cr and an offset.
 *   v_k  = ((n[k][0]*Y + n[k][1]*Cb) + n[k][2]*Cr) + n[k][3]     every product and sum rounded to float32, in this order, no fused multiply-add
 *   px_k = min(max(v_k, 0), 255)                                   not rounded to an integer
 * and from there on px is a float32 PIXEL input (RRV_DT_F32, RRV_LAY_HWC_BGR, RRV_SP_PIXEL).  So a YUV call's result equals, bit for bit, the
 * result of its float32 PIXEL BGR twin fed with the frame this arithmetic produces: over the device entries in every rrv_set_f43 mode, between
 * the host entries and the device twin in the fixed modes 0 and 2.  With RRV_TF_PAD_CROP the reflection acts on the pixel coordinates first and
 * the chroma lookup follows, which equals reflect-padding the converted frame, also for odd H / W.
 * rrv_yuv_input_matrix fills n with the inverse of rrv_yuv_matrix's transform for a standard and range — limited: Y' = (Y - 16) 255/219,
 * C' = (C - 128) 255/224; full: Y' = Y, C' = C - 128; R = Y' + 2(1-Kr) Cr', B = Y' + 2(1-Kb) Cb', G = Y' - (2 Kb (1-Kb) / Kg) Cb' -
 * (2 Kr (1-Kr) / Kg) Cr', the offsets folded into column 3 — each coefficient evaluated in double and rounded once to float32; it needs no handle
 * and no GPU.  rrv_set_yuv_input_matrix installs any twelve finite floats (else RRV_E_ARG); NULL restores the default, BT.601 limited range.  It
 * is handle state, independent of the output matrix, read when a call launches its first kernel (for rrv_add_from_yuv: when the deferred
 * encoding runs, in rrv_compute at the latest).
 * Device entries: rrv_transfer_from_yuv_device, _blend_from_yuv_device and _mask_from_yuv_device are rrv_transfer_image_device, _image_blend_device
 * and _image_mask_device with in_layout = RRV_LAY_I420 / RRV_LAY_NV12 in place of the input descriptor: the same flags, stream ordering, slots,
 * limits and errors; H, W >= 8; `out` any output descriptor, RRV_LAY_I420 / RRV_LAY_NV12 included (NV12 in -> NV12 out is decoder to encoder).
 * Host entries: rrv_transfer_from_yuv (flags within RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE), rrv_transfer_blend_from_yuv and
 * rrv_transfer_mask_from_yuv (flags within RRV_TF_PAD_CROP), pipelined as rrv_transfer_yuv (sub-batches of at most sixteen frames, staging,
 * page-locked buffers, every rrv_set_host_io mode), any B >= 1; `out` is float32 or uint8 RRV_LAY_HWC_BGR in RRV_SP_PIXEL, or uint8 I420 / NV12.
 * rrv_add_from_yuv[_device]: rrv_add / rrv_add_image_device for a sampled frame in one of the two layouts (deferred encoding, as they do).
 * Anything else — another in_layout, a null buffer, H or W < 8, an unknown flag — is RRV_E_ARG and the handle stays usable.  Not offered:
 * rrv_prepare_style from YUV (styles are image files), tickets and the cached-feature entries. */
int rrv_yuv_input_matrix(int standard, int full_range, float n[12]);
int rrv_set_yuv_input_matrix(rrv_handle h, const float n[12]);
int rrv_transfer_from_yuv_device(rrv_handle h, const void* d_in, int in_layout, int B, int H, int W,
                                 void* d_out, rrv_image_desc out, int flags, void* hip_stream);
int rrv_transfer_blend_from_yuv_device(rrv_handle h, const void* d_in, int in_layout, int B, int H, int W,
                                       const float* style_weight, int n_styles,
                                       void* d_out, rrv_image_desc out, int flags, void* hip_stream);
int rrv_transfer_mask_from_yuv_device(rrv_handle h, const void* d_in, int in_layout, int B, int H, int W,
                                      const float* d_mask, int n_styles, int mask_images,
                                      void* d_out, rrv_image_desc out, int flags, void* hip_stream);
int rrv_transfer_from_yuv(rrv_handle h, const uint8_t* frames_yuv, int in_layout, int B, int H, int W,
                          void* out, rrv_image_desc out_desc, int flags);
int rrv_transfer_blend_from_yuv(rrv_handle h, const uint8_t* frames_yuv, int in_layout, int B, int H, int W,
                                const float* style_weight, int n_styles,
                                void* out, rrv_image_desc out_desc, int flags);
int rrv_transfer_mask_from_yuv(rrv_handle h, const uint8_t* frames_yuv, int in_layout, int B, int H, int W,
                               const float* mask, int n_styles, int mask_images,
                               void* out, rrv_image_desc out_desc, int flags);
int rrv_add_from_yuv(rrv_handle h, const uint8_t* frame_yuv, int in_layout, int H, int W);
int rrv_add_from_yuv_device(rrv_handle h, const void* d_frame_yuv, int in_layout, int H, int W, void* hip_stream);

/* 10 / 12 / 16-bit YUV 4:2:0, in and out (HEVC Main10, AV1, VP9 profile 2: a hardware decoder's P010, ffmpeg's yuv420p10le, a C420p10
 * .y4m file): every entry above that takes RRV_LAY_I420 / RRV_LAY_NV12 also takes the two uint16 layouts below; there are no new transfer entries.
 * Frame layout.  Samples are uint16 in host byte order; CH = (H+1)/2, CW = (W+1)/2, frame_samples = H*W + 2*CH*CW; frame b starts at sample
 * b * frame_samples with nothing in between (frame_samples can be odd: a frame is only 2-byte aligned).
 *   RRV_LAY_I420_16  planar [Y][Cb][Cr], the d-bit code in the LOW bits   (ffmpeg yuv420p10le / 12le / 16le, Y4M C420p10 / p12 / p16)
 *   RRV_LAY_P016     [Y][CbCr interleaved], the code in the HIGH bits, low bits 0   (ffmpeg p010le / p012le / p016le; hardware decoders / encoders)
 * rrv_set_yuv_depth sets d for the input and the output side: each 10 (the default), 12 or 16; 0 leaves that side as it is; anything else is
 * RRV_E_ARG.  It is handle state read when a call launches (for rrv_add_from_yuv: when the deferred encoding runs).
 * Matrices map between RGB in the 0..255 PIXEL scale and d-bit codes, each coefficient evaluated in double and rounded once to float32.
 * rrv_yuv_matrix_depth: limited range Y' = (16 + 219/255 Y) 2^(d-8), chroma (128 + 224/255 C) 2^(d-8) — the 8-bit matrix times 2^(d-8), exactly;
 * full range Y' = (2^d - 1)/255 Y, chroma 2^(d-1) + (2^d - 1)/255 C.  rrv_yuv_input_matrix_depth is the inverse of these formulas, written out
 * from them as rrv_yuv_input_matrix is.  bits is 8 (== rrv_yuv_matrix / rrv_yuv_input_matrix), 10, 12 or 16, else RRV_E_ARG; no handle, no GPU.
 * rrv_set_yuv16_matrix / rrv_set_yuv16_input_matrix install twelve finite floats (else RRV_E_ARG) for the uint16 layouts only: they are
 * independent of the 8-bit matrices and of each other.  NULL restores the default: BT.601 limited range at the depth in force when the call
 * launches.  The 8-bit layouts never see the depth or these matrices.
 * Output arithmetic: c_k as for 8 bits with the 16-bit matrix; Y code = rint(min(max(c_0, 0), 2^d - 1)), half to even; a chroma code the same clamp
 * and rint of ((tl + tr) + (bl + br)) * 0.25f of the unclamped c_1 / c_2, odd last rows and columns as for 8 bits; stored sample = code
 * (RRV_LAY_I420_16) or code << (16 - d) (RRV_LAY_P016).  So a 16-bit entry's samples are this arithmetic applied to its float32 twin's output,
 * bit for bit, for the same frames and frames per call.
 * Input arithmetic: code = sample (RRV_LAY_I420_16: used as it is, a well-formed stream sets no bit above d) or sample >> (16 - d) (RRV_LAY_P016:
 * the low bits are ignored); v_k and px_k = min(max(v_k, 0), 255) as for 8 bits with the 16-bit input matrix, px NOT rounded, so a 10-bit source keeps
 * its fractional pixel values; from there px is a float32 PIXEL BGR input, with the bit-identity statements of the 8-bit input entries.
 * Where: rrv_transfer_yuv, rrv_transfer_blend_batch_yuv and rrv_transfer_mask_batch_yuv take layout 8 / 9 (out_yuv then holds 2 * frame_samples bytes
 * per frame); the three rrv_transfer_image*_device entries and the `out` / `out_desc` of the six rrv_*_from_yuv* entries take
 * {RRV_DT_U16, 8 | 9, RRV_SP_PIXEL}; the six rrv_*_from_yuv* entries and rrv_add_from_yuv[_device] take in_layout 8 / 9.  Any mix of input and output
 * depth and layout is allowed (8-bit in -> 10-bit out, P010 -> P010).  RRV_E_ARG, the handle staying usable: RRV_DT_U16 with any other layout or
 * space, layouts 8 / 9 with another dtype, layouts 8 / 9 as an rrv_image_desc INPUT; layout values 4..7 stay refused.  Flags, stream ordering,
 * slots, sub-batching, rrv_set_host_io modes, page-locked buffers and rrv_get_preclamp_image behave as for the 8-bit forms.  A sample stream is
 * 3 bytes per pixel each way, what a uint8 BGR input already is and a quarter of the float32 output.  HDR transfer functions are the caller's:
 * the network is trained on display-referred 0..1 values, a PQ / HLG source needs tone mapping first. */
enum { RRV_DT_U16 = 2 };        /* rrv_image_desc.dtype after RRV_DT_U8 = 0 and RRV_DT_F32 = 1: uint16 samples, only with the two layouts below */
enum { RRV_LAY_I420_16 = 8,     /* planar [Y][Cb][Cr], uint16, code in the LOW bits */
       RRV_LAY_P016    = 9 };   /* [Y][CbCr interleaved], uint16, code in the HIGH bits, low bits 0 */
int rrv_set_yuv_depth(rrv_handle h, int in_bits, int out_bits);
int rrv_yuv_matrix_depth(int standard, int full_range, int bits, float m[12]);
int rrv_yuv_input_matrix_depth(int standard, int full_range, int bits, float n[12]);
int rrv_set_yuv16_matrix(rrv_handle h, const float m[12]);
int rrv_set_yuv16_input_matrix(rrv_handle h, const float n[12]);

/* YUV 4:2:2 and 4:4:4, 8 to 16 bits, in and out (ProRes 422 / 4444 and DNxHR, which are never 4:2:0; broadcast 4:2:2 10-bit contribution
 * feeds; an SDI capture card's NV16 / P210; 4:4:4 screen content; a C422p10 .y4m file).  The chroma format is a flag OR-ed onto one of the four
 * YUV layouts above; there are no new entry points, kernels or instantiations: the subsampling is a launch parameter of the YUV kernels.
 *   RRV_LAY_422 = 0x10   chroma planes of CW = (W+1)/2 columns and CH = H rows: a chroma sample per horizontal pixel pair
 *   RRV_LAY_444 = 0x20   chroma planes of CW = W columns and CH = H rows: a chroma sample per pixel
 *   (no flag)            4:2:0 as above: CW = (W+1)/2, CH = (H+1)/2
 *   layout            value  flag form                 samples  ffmpeg -pix_fmt
 *   RRV_LAY_I422        18   RRV_LAY_I420    | 0x10    uint8    yuv422p
 *   RRV_LAY_NV16        19   RRV_LAY_NV12    | 0x10    uint8    nv16
 *   RRV_LAY_I422_16     24   RRV_LAY_I420_16 | 0x10    uint16   yuv422p10le / 12le / 16le   (Y4M C422p10 / p12 / p16)
 *   RRV_LAY_P216        25   RRV_LAY_P016    | 0x10    uint16   p210le / p212le / p216le
 *   RRV_LAY_I444        34   RRV_LAY_I420    | 0x20    uint8    yuv444p
 *   RRV_LAY_NV24        35   RRV_LAY_NV12    | 0x20    uint8    nv24
 *   RRV_LAY_I444_16     40   RRV_LAY_I420_16 | 0x20    uint16   yuv444p10le / 12le / 16le   (Y4M C444p10 / p12 / p16)
 *   RRV_LAY_P416        41   RRV_LAY_P016    | 0x20    uint16   p410le / p412le / p416le
 * Both flags together, or a flag on a base that is not one of the four YUV layouts (values 16, 17, 32, 33, 48 and above), is RRV_E_ARG, as
 * 4..7, 10 and -1 stay.
 * Frame layout: frame_samples = H*W + 2*CH*CW with the CH, CW of the chroma format, the planes in the base layout's order ([Y][Cb][Cr], or
 * [Y][CbCr interleaved: CH rows of CW pairs]), frame b at sample b * frame_samples, nothing in between.  Views: Y is W x H; a planar Cb or Cr
 * plane CW x CH; the semi-planar CbCr plane 2 CW x CH (4:4:4: rows of 2W elements).
 * Where: every place that takes one of the four 4:2:0 layouts takes these eight under the same rules — rrv_transfer_yuv,
 * rrv_transfer_blend_batch_yuv, rrv_transfer_mask_batch_yuv; the `out` descriptor of the three rrv_transfer_image*_device entries; in_layout
 * and `out` of the six rrv_*_from_yuv* entries; rrv_add_from_yuv[_device]; either side of the four rrv_*_view_device entries;
 * rrv_image_view_contiguous and rrv_image_view_check.  The dtype, space, depth (rrv_set_yuv_depth), matrix, flag, sub-batch, host-I/O and
 * stream rules are those of the base layout, and any mix of chroma format, depth and layout between input and output is allowed (NV12 in ->
 * P210 out).  As the base layouts, the new ones stay refused as an rrv_image_desc INPUT.  The largest new frame, 4:4:4 in uint16, is 6 bytes
 * per pixel, half of the float32 BGR frame the staging of the host entries is sized for anyway.
 * Output arithmetic: c_k, the clamp, rint half to even and the << (16 - d) of the P forms are exactly those of the base layout.
 *   4:2:2  chroma sample (i, j) = (l + r) * 0.5f of the unrounded, unclamped c_1 (then c_2) of pixels (i, 2j) and (i, 2j+1), evaluated in
 *          float32 in that order with no contraction; for a last odd column r takes l's value.
 *   4:4:4  the sample is c_k of its pixel.
 *   4:2:0  ((tl + tr) + (bl + br)) * 0.25f, unchanged bit for bit.
 * The pair mean sites chroma at the centre of its pixel pair (4:2:0: of its block), the C420jpeg / MPEG-1 siting the 4:2:0 forms chose; it
 * is one consistent choice for every subsampled format, not the left-sited chroma of MPEG-2 / H.264 4:2:2.
 * Input arithmetic: pixel (y, x) takes chroma sample (y >> sy, x >> sx), (sx, sy) = (1, 1) for 4:2:0, (1, 0) for 4:2:2 and (0, 0) for 4:4:4 —
 * under RRV_TF_PAD_CROP after the reflection — and everything else is as for the base layout.
 * The bit-identity statements of the 4:2:0 forms hold word for word: a YUV-output call equals this arithmetic applied to its float32 twin's
 * output for the same frames and frames per call; a YUV-input call equals its float32 PIXEL BGR twin fed with the converted frame; a view call
 * equals the contiguous call.
 * Out of scope: packed forms (YUY2, UYVY, v210, Y210), 4:4:4 with alpha, mono, chroma sitings other than the box mean, 4:1:1 and 4:4:0. */
enum { RRV_LAY_422 = 0x10,      /* on a YUV layout: 4:2:2, CW = (W+1)/2, CH = H */
       RRV_LAY_444 = 0x20 };    /* on a YUV layout: 4:4:4, CW = W, CH = H */
enum { RRV_LAY_I422    = RRV_LAY_I420    | RRV_LAY_422,     /* 18 */
       RRV_LAY_NV16    = RRV_LAY_NV12    | RRV_LAY_422,     /* 19 */
       RRV_LAY_I422_16 = RRV_LAY_I420_16 | RRV_LAY_422,     /* 24 */
       RRV_LAY_P216    = RRV_LAY_P016    | RRV_LAY_422,     /* 25 */
       RRV_LAY_I444    = RRV_LAY_I420    | RRV_LAY_444,     /* 34 */
       RRV_LAY_NV24    = RRV_LAY_NV12    | RRV_LAY_444,     /* 35 */
       RRV_LAY_I444_16 = RRV_LAY_I420_16 | RRV_LAY_444,     /* 40 */
       RRV_LAY_P416    = RRV_LAY_P016    | RRV_LAY_444 };   /* 41 */

/* rrv_prepare_style (test/framework.py:99-104; stylization.py:71-79) and rrv_add (test/framework.py:82-86) for images a torch
 * pipeline already holds in HBM: the rrv_image_desc rules of rrv_transfer_image_device (uint8 only in PIXEL space; any layout;
 * float32 in PIXEL / UNIT / NORM), one image [Hs][Ws] / [H][W] per call.  The style is read in colour, a sampled frame through
 * the grey fold, by the same first kernel as the content frames; an image derived from uint8 pixels the reference's way gives the
 * uint8 entry's state bit for bit.  The image is read in the order of hip_stream (NULL: the null stream): what that stream holds
 * when the call is made precedes the read, and the read is complete when the call returns (both calls synchronise, as their host
 * twins do; they run once per video).  rrv_add_image_device defers encoding as rrv_add does and keeps the frame in the form it
 * arrived in; a frame in another form than the pending ones encodes those first. */
int rrv_prepare_style_image_device(rrv_handle h, const void* d_style, rrv_image_desc in, int Hs, int Ws, int style_id, void* hip_stream);
int rrv_add_image_device(rrv_handle h, const void* d_frame, rrv_image_desc in, int H, int W, void* hip_stream);

/* Strided image views: pitched and windowed device frames, in and out (a hardware decoder's NV12 / P010 surface with a row pitch above the
 * width, an aligned height and the chroma plane at its own offset; a crop x[:, :, y0:y1, x0:x1] of a torch tensor; a window of a larger canvas
 * as the output; a grey tensor expanded to three channels; YV12 = I420 with the Cb and Cr offsets swapped).  A view is an image descriptor plus
 * where the rows of its planes lie.  All strides and offsets are in ELEMENTS of desc.dtype, as torch's are (a float or uint16 row can never be
 * misaligned); the base pointer is aligned to the element size.  Frame b starts b * frame_stride elements after the base pointer, row r of
 * plane k plane_offset[k] + r * pitch[k] elements after the frame's start.  Planes per layout (row length in elements x rows), with
 * CH = (H+1)/2 and CW = (W+1)/2 as everywhere (with RRV_LAY_422 on the layout CH = H; with RRV_LAY_444 CH = H and CW = W):
 *   RRV_LAY_HWC_BGR                   one: 3W x H
 *   RRV_LAY_CHW_RGB                   R, G, B: W x H each
 *   RRV_LAY_I420, RRV_LAY_I420_16     Y: W x H; Cb, Cr: CW x CH each            (and their 4:2:2 / 4:4:4 forms RRV_LAY_I422[_16], RRV_LAY_I444[_16])
 *   RRV_LAY_NV12, RRV_LAY_P016        Y: W x H; CbCr interleaved: 2 CW x CH     (and RRV_LAY_NV16, RRV_LAY_P216, RRV_LAY_NV24, RRV_LAY_P416)
 * Array entries of planes a layout does not have are ignored.  desc may name every layout on either side: a view entry reads the YUV layouts
 * as well (the rrv_*_from_yuv_device entries are the view entries on contiguous views).  A view has no semantics of its own: a view call
 * equals, bit for bit, the contiguous call on the same pixels, in every kernel mode.  Both ends of the hot path address every frame through a
 * view (conv_first_k / conv_last_k); the contiguous entries build theirs with rrv_image_view_contiguous' formulas.
 * rrv_image_view_contiguous fills *v with the strides of the contiguous form the other entries take for H x W frames; RRV_E_ARG for a
 * descriptor no entry knows (or H, W < 1).  rrv_image_view_check says whether B frames of H x W (the frame as passed for an input, the
 * delivered Ho x Wo frame for an output) can be addressed through *v: RRV_OK or RRV_E_ARG.  Neither needs a handle or a GPU.  The rules:
 *   1  every stride and offset is >= 0 (and, so that no address arithmetic can wrap, a pitch is at most 2^31 - 1 elements, a plane
 *      offset and the frame stride at most 2^40);
 *   2  pitch[k] >= the row length of plane k;
 *   3  dtype, layout and space are a combination the descriptor entries accept (uint8 and the integer YUV layouts in RRV_SP_PIXEL only;
 *      RRV_DT_U16 with the two uint16 layouts only);
 *   4  for an output only: the element extents [plane_offset[k], plane_offset[k] + (rows - 1) * pitch[k] + row length) of the planes of one
 *      frame are pairwise disjoint, and for B > 1 frame_stride >= the end of the last extent.  Row-interleaved output planes are therefore
 *      refused.  An input may overlap itself: three equal plane_offsets on RRV_LAY_CHW_RGB read a grey image as R = G = B, frame_stride 0
 *      reads one frame B times.
 * The view entries mirror rrv_transfer_image_device, _image_blend_device, _image_mask_device and rrv_add_image_device: the same flags, stream
 * ordering, slots, limits (1..64 frames) and error codes; masks and weights stay contiguous.  The transfer entries run both checks before any
 * GPU work; a refusal is RRV_E_ARG, rrv_last_error names the offending field (e.g. "out.pitch[1]") and the handle stays usable.  The ranges
 * that d_in / in and d_out / out address must not overlap each other: this is NOT checked.  Frames of a batch above the launch group (16 for
 * the frame-mode, blended and masked models) are found by frame_stride.  rrv_add_view_device compacts the frame into the pending sampled
 * frames with one 2-D device copy per plane, in the order of hip_stream; everything after that is rrv_add_image_device. */
typedef struct {
    rrv_image_desc desc;       /* dtype, layout, space: every layout, the YUV ones included, on either side */
    int64_t frame_stride;      /* elements of desc.dtype from frame b to frame b + 1 */
    int64_t plane_offset[3];   /* elements from the frame's start to row 0 of plane k */
    int64_t pitch[3];          /* elements from one row of plane k to the next */
} rrv_image_view;
int rrv_image_view_contiguous(rrv_image_desc d, int H, int W, rrv_image_view* v);
int rrv_image_view_check(const rrv_image_view* v, int B, int H, int W, int output);
int rrv_transfer_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int H, int W,
                             void* d_out, const rrv_image_view* out, int flags, void* hip_stream);
int rrv_transfer_view_blend_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int H, int W,
                                   const float* style_weight, int n_styles,
                                   void* d_out, const rrv_image_view* out, int flags, void* hip_stream);
int rrv_transfer_view_mask_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int H, int W,
                                  const float* d_mask, int n_styles, int mask_images,
                                  void* d_out, const rrv_image_view* out, int flags, void* hip_stream);
int rrv_add_view_device(rrv_handle h, const void* d_frame, const rrv_image_view* in, int H, int W, void* hip_stream);

/* Scaling: frames resampled to a working size on the GPU, in front of everything else (the "content size" of style-transfer tools: the working
 * resolution sets the stroke size of the stylized picture, and the speed).  The source frames are SH x SW in any form the first kernel reads, through
 * the same views; H x W is the working size, which is also the size of the delivered frame (with RRV_TF_PAD_CROP the resampled H x W frame is what
 * gets reflect-padded and cropped; without it 8*(H/8) x 8*(W/8) are delivered as always), unless the call names a delivered size ("Output size" below).
 * Arithmetic: one separable filter.  For one axis with S source and D destination samples, s = S / D and support = max(s, 1); output sample i has
 *   c = s (i + 0.5),  lo = max(int(c - support + 0.5), 0),  n = min(int(c + support + 0.5), S) - lo   (int truncates)
 *   w_j = tri((lo + j - c + 0.5) / support) / sum_j of the same,  tri(t) = max(0, 1 - |t|),  j = 0 .. n - 1
 * evaluated and normalised in double, each weight rounded once to float32; the tables are built on the host.  For s > 1 this is the antialiased
 * triangle filter (PIL's BILINEAR reduce, torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False)); for s <= 1 plain
 * half-pixel bilinear with edge clamp; for S == D every row is {1, 0} and the resampled value is the source value, bit for bit (the kernel's tables drop a
 * trailing tap of weight 0 and the sums start from -0, so this holds for -0 and for non-finite float32 inputs too).  Per axis
 * S / D <= 8 and D / S <= 8 (else RRV_E_ARG), so a row has at most 16 taps.
 * A source pixel enters as the float32 PIXEL value, BGR, that the first kernel derives from it: uint8 (float)px; float32 PIXEL v; UNIT v * 255.0f;
 * NORM (v * std + mean) * 255.0f (each operation rounded); every YUV layout, depth and chroma format as documented for rrv_transfer_from_yuv (chroma
 * sample (y >> csy, x >> csx), the 3 x 4 input matrix with each operation rounded and no contraction, a clamp to 0..255; matrix and depth are read
 * from the handle when the call launches).  The three channels are filtered in float32, first along rows, then along columns, taps in ascending
 * order with fused multiply-adds, and are NOT rounded to integers: a 10-bit source keeps its precision.  Frame b's result does not depend on B.
 * From there on the frames are a float32 HWC BGR PIXEL input: a scaled call equals, bit for bit in a fixed kernel mode, rrv_resample_view_device
 * followed by the unscaled call on its output.
 *   rrv_resample_taps                the tables of one axis: first[D], count[D], w[D][cap] (zero beyond count); no handle, no GPU; RRV_E_ARG outside
 *                                    the ratio limits or when cap is below the largest count
 *   rrv_resample_view_device         the resampler alone: B (1..64) frames through `in` -> contiguous [B][H][W][3] float32 BGR PIXEL, queued on
 *                                    hip_stream (NULL: the null stream)
 *   rrv_transfer_scaled_view_device  rrv_transfer_view_device on the resampled frames: `in` describes SH x SW frames, `out` the delivered ones;
 *                                    flags RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE | RRV_TF_ON_STREAM; slots, limits and stream ordering as there
 *   rrv_transfer_scaled              the host twin through the host pipeline: contiguous frames, `in` = {RRV_DT_U8, RRV_LAY_HWC_BGR, RRV_SP_PIXEL}
 *                                    or any YUV layout with its sample type; `out` what rrv_transfer_from_yuv delivers; flags within
 *                                    RRV_TF_PAD_CROP | RRV_TF_FRAME_MODE; any B >= 1.  Sub-batches are sized by the working frame as for the unscaled
 *                                    call and hold at most 4 x its pixel budget of SOURCE pixels (fewer frames per sub-batch above 2 x per axis), so
 *                                    the staging per set is at most four times the unscaled call's: 16 x 640 x 640 x 4 source pixels
 *   rrv_add_scaled[_view_device]     rrv_add / rrv_add_view_device for a sampled frame scaled the same way (kept as the float32 working frame)
 * Checks, all before any GPU work: the view against (SH, SW), the frame rules against (H, W), the ratio limits; RRV_E_ARG names the field and the
 * handle stays usable.  The resampled frames of a launch group live in a grow-only float32 buffer per workspace slot (12 bytes per working pixel and
 * frame), reserved with the axis tables before the call's first launch: out of memory is RRV_E_NOMEM and the handle stays usable.
 * Not offered yet: blended and masked twins, a scaled rrv_prepare_style, tickets. */
int rrv_resample_taps(int S, int D, int* first /*[D]*/, int* count /*[D]*/, float* w /*[D][cap]*/, int cap);
int rrv_resample_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW,
                             int H, int W, float* d_out, void* hip_stream);
int rrv_transfer_scaled_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW,
                                    int H, int W, void* d_out, const rrv_image_view* out, int flags, void* hip_stream);
int rrv_transfer_scaled(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW,
                        int H, int W, void* out, rrv_image_desc out_desc, int flags);
int rrv_add_scaled_view_device(rrv_handle h, const void* d_frame, const rrv_image_view* in, int SH, int SW,
                               int H, int W, void* hip_stream);
int rrv_add_scaled(rrv_handle h, const void* frame, rrv_image_desc in, int SH, int SW, int H, int W);

/* Scaling, output size: the stylized working frame resampled to a delivered size DH x DW on the GPU, behind the last kernel, and written in any
 * output form the last kernel has (float32 / uint8, HWC BGR / planar RGB, the three spaces of the float32 forms, every YUV layout, depth and chroma
 * format) through the same views.  "Stylize at the working size, deliver at the source's": a 3840 x 2160 NV12 surface in, worked on at 1920 x 1080,
 * leaves as a 3840 x 2160 NV12 surface, and the host touches no pixel.
 * The frame that is resampled is the delivered working frame as float32 HWC BGR PIXEL values, what the float32 PIXEL call writes: with
 * RRV_TF_PAD_CROP the H x W crop window, without it the 8*(H/8) x 8*(W/8) frame.  Call it OH x OW.
 * Arithmetic.  Resample: exactly the input resampler's, with the rrv_resample_taps tables of (OH -> DH) and (OW -> DW): the three channels in
 * float32, first along rows, then along columns, taps in ascending order with fused multiply-adds, the sums starting from -0; per axis
 * OH / DH <= 8 and DH / OH <= 8 (else RRV_E_ARG).  The resampled value v of a pixel and channel is therefore the same bits whatever the output form,
 * and for DH == OH, DW == OW it is the working frame's value.  From v, with each operation rounded to float32 and none contracted:
 *   float32 PIXEL   v, not clamped (a bilinear upscale stays within the range of its inputs, 0..255)
 *   float32 UNIT    v / 255.0f
 *   float32 NORM    (v / 255.0f - mean_c) / std_c: the normalised form of the DELIVERED pixel, the inverse of what the first kernel does to a
 *                   uint8 pixel.  It is not the pre-clamp network output the unscaled NORM form delivers: a resampled frame has none.
 *   uint8           rint(min(max(v, 0), 255)), half to even
 *   YUV             the last kernel's store, applied to v over the delivered frame: c_k = ((m[k][0] R + m[k][1] G) + m[k][2] B) + m[k][3];
 *                   Y code = rint(min(max(c_0, 0), 2^d - 1)); a chroma code the same of ((tl + tr) + (bl + br)) * 0.25f (4:2:0), (l + r) * 0.5f
 *                   (4:2:2) or the pixel's own value (4:4:4) of the unclamped c_1 / c_2, a pixel outside the DH x DW frame (odd last row or
 *                   column) replaced by its nearest one inside; the code shifted left by 16 - d for the P forms.  Matrix and depth are read
 *                   from the handle when the call launches.
 * Frame b's result does not depend on B.  A delivering call equals, bit for bit in a fixed kernel mode, the float32 HWC BGR PIXEL call followed by
 * rrv_deliver_view_device into the form asked for.  DH x DW equal to OH x OW is the plain call: no kernel is added and every bit is what it was.
 *   rrv_deliver_view_device           the delivery stage alone: B (1..64) contiguous float32 [H][W][3] BGR PIXEL frames -> DH x DW frames through
 *                                     `out`, queued on hip_stream (NULL: the null stream); nothing of the handle's own streams takes part
 *   rrv_transfer_deliver_view_device  rrv_transfer_scaled_view_device with a delivered size: `out` describes DH x DW frames; SH = SW = 0: the frames
 *                                     are H x W (no input scaling); DH = DW = 0: the working frame is delivered.  Flags RRV_TF_PAD_CROP |
 *                                     RRV_TF_FRAME_MODE | RRV_TF_ON_STREAM; the caller's stream waits for the delivery, not for the last kernel
 *   rrv_transfer_deliver              the host twin through the host pipeline, as rrv_transfer_scaled; flags within RRV_TF_PAD_CROP |
 *                                     RRV_TF_FRAME_MODE.  The output staging per set is sized by the delivered frame, and a sub-batch additionally
 *                                     holds at most 4 x the pixel budget of DELIVERED pixels (the rule of the source side)
 * Checks, all before any GPU work: the output view against (DH, DW), the ratio limits between OH x OW and DH x DW, and everything the scaled entries
 * check; RRV_E_ARG names the field and the handle stays usable.  The working frames of a launch group live in a second grow-only float32 buffer per
 * workspace slot (12 bytes per working pixel and frame), reserved with the tables before the call's first launch: out of memory is RRV_E_NOMEM and
 * the handle stays usable.
 * Not offered yet: blended and masked delivery, tickets and the one-frame entries. */
int rrv_deliver_view_device(rrv_handle h, const float* d_in, int B, int H, int W, int DH, int DW,
                            void* d_out, const rrv_image_view* out, void* hip_stream);
int rrv_transfer_deliver_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W,
                                     int DH, int DW, void* d_out, const rrv_image_view* out, int flags, void* hip_stream);
int rrv_transfer_deliver(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W,
                         int DH, int DW, void* out, rrv_image_desc out_desc, int flags);

/* Guided delivery: the stylized working frame upsampled to the delivered size along the SOURCE's edges, on the GPU, in place of the half-pixel
 * bilinear resampling of "Output size".  Joint upsampling with the fast guided filter (He & Sun, "Fast Guided Filter", 2015; He, Sun & Tang,
 * "Guided Image Filtering", 2013): a local linear model stylized = a * luma + b is fitted at the working size, the smooth coefficients are
 * upsampled instead of the picture, and they are applied to the luma of the full-resolution source.  The network still runs at the working size.
 * Inputs, per frame, all float32 HWC BGR PIXEL: the stylized working frame P [OH][OW][3] (what the float32 PIXEL call delivers), the source at the
 * working size X_lo [OH][OW][3] and at the delivered size X_hi [DH][DW][3].
 * Parameters: the radius r in working pixels, 1..16, and eps > 0 in the units of a 0..1 image; internally e = eps * 65025.
 * Arithmetic.
 *   guide         g = (0.114f B + 0.587f G) + 0.299f R of a float32 PIXEL value, each operation rounded to float32: g_lo from X_lo, g_hi from X_hi
 *   box mean      M_r(f)(y, x): the mean of f over the window [y - r, y + r] x [x - r, x + r] clipped to the frame, divided by the number of
 *                 pixels actually inside it
 *   coefficients  per channel c, at the working size:
 *                   a_c = (M_r(g_lo P_c) - M_r(g_lo) M_r(P_c)) / (M_r(g_lo^2) - M_r(g_lo)^2 + e)
 *                   b_c = M_r(P_c) - a_c M_r(g_lo)
 *                   A_c = M_r(a_c), B_c = M_r(b_c)
 *   upsample      A_c and B_c resampled OH x OW -> DH x DW with the rrv_resample_taps tables of (OH -> DH) and (OW -> DW) in the delivery stage's
 *                 separable order: along rows first, then along columns, taps ascending
 *   apply         Q_c = up(A_c) g_hi + up(B_c), not clamped: Q is a float32 HWC BGR PIXEL frame of DH x DW
 * Q then reaches the output form asked for through the delivery stage at equal size, which is the identity on values ("Output size": for
 * DH == OH, DW == OW the resampled value is the input's): uint8, planar RGB, the three value spaces and every YUV layout, depth and chroma
 * format are, word for word, those of "Output size" applied to v = Q.
 * Per axis DH >= OH and DH / OH <= 8 (else RRV_E_ARG naming the field).  Equal size is allowed: the stage is then an edge-aware smoothing.
 * This stage is bit-exact to nothing: the moments are float32 sums (of values offset by a per-tile anchor, which leaves covariance and variance
 * what they are and keeps their cancellation small where the picture is smooth), and the tests hold it to a float64 restatement of the
 * arithmetic above.  Frame b's result does not depend on B.
 *   rrv_deliver_guided_view_device   the stage alone: B (1..64) frames d_P, d_guide_lo (both [H][W][3]) and d_guide_hi ([DH][DW][3]), contiguous
 *                                    float32 BGR PIXEL, -> DH x DW frames through `out`, queued on hip_stream (NULL: the null stream); nothing of
 *                                    the handle's own streams takes part.  Its coefficient planes and Q live in the handle: calls on different
 *                                    streams must be ordered by the caller
 *   rrv_transfer_guided_view_device  rrv_transfer_deliver_view_device with r and eps: the guide is the call's own source frames, X_hi the source
 *                                    through the input resampler at equal size (the first kernel's float32 PIXEL value of each source pixel, bit
 *                                    for bit) and X_lo the resampled working input of a scaled call (X_hi itself without input scaling).  Needs
 *                                    DH x DW == SH x SW, or SH = SW = 0 and DH x DW == H x W; and a delivered working frame of H x W:
 *                                    RRV_TF_PAD_CROP, or H and W multiples of 8.  Anything else is RRV_E_ARG
 *   rrv_transfer_guided              the host twin through the host pipeline; sub-batches by the sizing rules of rrv_transfer_deliver
 *   rrv_guided_tile                  the tile the stage launches its second kernel with for a working frame H x W, a delivered frame DH x DW and
 *                                    radius r: delivered columns per tile (tw; 16 rows), the working rows and columns a tile stages (sy, sx) and
 *                                    the dynamic LDS of the second and the first kernel in bytes; no handle, no GPU; RRV_E_ARG for a null pointer
 *                                    and for sizes or a radius the entries above refuse
 * A guided call equals, bit for bit in a fixed kernel mode, the float32 HWC BGR PIXEL call at the working size, the resampler alone for the
 * two guides, and rrv_deliver_guided_view_device into the form asked for.  r and eps travel with the call, never in the handle.
 * Checks, all before any GPU work, as "Output size"; RRV_E_ARG names the field and the handle stays usable.  Per workspace slot the stage
 * keeps three more grow-only float32 buffers (X_hi and Q: 12 bytes per delivered pixel and frame each; the coefficient planes: 24 bytes per
 * working pixel and frame), reserved with the tables before the call's first launch: out of memory is RRV_E_NOMEM and the handle stays usable.
 * Not offered: blended and masked guided delivery, tickets and the one-frame entries. */
int rrv_deliver_guided_view_device(rrv_handle h, const float* d_P, const float* d_guide_lo, const float* d_guide_hi, int B, int H, int W,
                                   int DH, int DW, int r, float eps, void* d_out, const rrv_image_view* out, void* hip_stream);
int rrv_transfer_guided_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W,
                                    int DH, int DW, int r, float eps, void* d_out, const rrv_image_view* out, int flags, void* hip_stream);
int rrv_transfer_guided(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W,
                        int DH, int DW, int r, float eps, void* out, rrv_image_desc out_desc, int flags);
int rrv_guided_tile(int H, int W, int DH, int DW, int r, int* tw, int* sy, int* sx, int* apply_lds_bytes, int* coeff_lds_bytes);

/* Compositing: the stylized frame mixed with its own source on the GPU, behind the delivery or guided stage and in front of the output form:
 * how strongly the style applies (strength, per frame), where (a matte, per pixel) and whether the source keeps its colours or its luminance.
 * Inputs, per frame, float32 HWC BGR PIXEL of the delivered size DH x DW: P, the stylized frame at the delivered size (the working frame itself,
 * the delivery stage's bilinear result, or the guided stage's Q), and S, the source at the delivered size.
 * Arithmetic, each operation rounded to float32 and none contracted:
 *   g(v)   = (0.114f v_B + 0.587f v_G) + 0.299f v_R                the guided stage's luma
 *   keep RRV_KEEP_NONE:    C_c = P_c
 *   keep RRV_KEEP_COLOUR:  d = g(P) - g(S);  C_c = S_c + d         source colours, stylized luminance (the luminance-only transfer of Gatys et
 *                                                                  al., "Preserving Color in Neural Artistic Style Transfer", 2016)
 *   keep RRV_KEEP_LUMA:    d = g(S) - g(P);  C_c = P_c + d         stylized colours, source luminance
 *   alpha  = strength_b                                            without a matte
 *          = strength_b * m(y, x)                                  float32 matte
 *          = strength_b * ((float)u(y, x) / 255.0f)                uint8 matte
 *   out_c  = (1.0f - alpha) * S_c + alpha * C_c                    two products and one sum; not clamped
 * For finite inputs alpha == 0 returns S_c numerically equal and alpha == 1 returns C_c bit for bit: inside a hard matte the result is the
 * stylized frame's bits, outside it the source's.  strength_b must lie in [0, 1]; anything else, NaN included, is RRV_E_ARG.  Matte values are
 * device data and are not checked: values outside 0..1 extrapolate.  The result then reaches the output form asked for through the delivery
 * stage at equal size (the identity on values, as Q does in "Guided delivery"), so every output form, YUV layout, bit depth and pitched view
 * is, word for word, that of "Output size" applied to v = out.  Frame b's result does not depend on B.
 *   rrv_composite              the request: per-frame strengths in HOST memory (NULL: 1 for every frame), the matte ([matte_frames][DH][DW]
 *                              contiguous, RRV_DT_F32 or RRV_DT_U8, matte_frames 1 = one matte for every frame, or B; device memory for the
 *                              device entries, host memory for the host twin; NULL: none) and keep
 *   rrv_composite_view_device  the stage alone: B (1..64) contiguous frames d_P and d_src -> DH x DW frames through `out`, queued on hip_stream
 *                              (NULL: the null stream); nothing of the handle's own streams takes part.  The mixed frame lives in a buffer of the
 *                              handle: calls on different streams must be ordered by the caller.  The buffers need only be element aligned
 *   rrv_transfer_composite_view_device
 *                              rrv_transfer_deliver_view_device (r = 0) or rrv_transfer_guided_view_device (r, eps) with a request: S is the
 *                              call's own source frames through the input resampler to the delivered size -- at equal size the first kernel's
 *                              float32 PIXEL value of each source pixel, bit for bit, whatever the input form; the resampled working input of a
 *                              scaled call when the working frame is the one delivered; the guided stage's X_hi.  The source need not have the
 *                              delivered size: any ratio the resampler accepts (<= 8 per axis).  Needs a delivered working frame of H x W
 *                              (RRV_TF_PAD_CROP, or H and W multiples of 8) and the GLOBAL or FRAME model.  c == NULL, or no matte with every
 *                              strength 1 and keep RRV_KEEP_NONE, is exactly the call without a request: no kernel is added, every bit is what
 *                              it was
 *   rrv_transfer_composite     the host twin through the host pipeline, any B; sub-batches by the sizing rules of rrv_transfer_deliver; the matte
 *                              rides each sub-batch's staging with its frames; strengths and a per-frame matte are indexed by the frame's
 *                              position in the whole call
 *   rrv_composite_grid         the launch rule of the stage for B frames of DH x DW: a thread takes 4 consecutive pixels of the flat run of
 *                              B * DH * DW per step, 256 threads per workgroup, grid = min(ceil(B DH DW / 1024), 2048) workgroups and
 *                              pixels_per_pass = grid * 1024; larger runs are grid-strided.  No handle, no GPU; RRV_E_ARG for a null pointer or
 *                              sizes below 1
 * A compositing call equals, bit for bit in a fixed kernel mode, the float32 HWC BGR PIXEL call with the same sizes and guide, the resampler
 * alone for the source at the delivered size, and rrv_composite_view_device into the form asked for.
 * Checks, all before any GPU work: those of the entry without a request, then the request (strength, keep, matte_dtype, matte_frames); RRV_E_ARG
 * names the field and the handle stays usable.  Per workspace slot the stage shares the guided stage's X_hi and Q buffers (12 bytes per
 * delivered pixel and frame each), reserved with the tables before the call's first launch: out of memory is RRV_E_NOMEM and the handle stays
 * usable.
 * Not offered: blended and masked compositing, tickets and the one-frame entries, a matte at any size but the delivered one. */
#define RRV_KEEP_NONE 0
#define RRV_KEEP_COLOUR 1
#define RRV_KEEP_LUMA 2
typedef struct rrv_composite {
    const float* strength;   /* host memory, one per frame of the call; NULL: 1 for every frame */
    const void* matte;       /* NULL: none.  [matte_frames][DH][DW] contiguous; device memory for the device entries, host for the host twin */
    int matte_dtype;         /* RRV_DT_F32 or RRV_DT_U8 */
    int matte_frames;        /* 1 (one matte for every frame) or B */
    int keep;                /* RRV_KEEP_* */
} rrv_composite;
int rrv_composite_view_device(rrv_handle h, const float* d_P, const float* d_src, int B, int DH, int DW, const rrv_composite* c,
                              void* d_out, const rrv_image_view* out, void* hip_stream);
int rrv_transfer_composite_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W,
                                       int DH, int DW, int r, float eps, const rrv_composite* c, void* d_out, const rrv_image_view* out,
                                       int flags, void* hip_stream);
int rrv_transfer_composite(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W,
                           int DH, int DW, int r, float eps, const rrv_composite* c, void* out, rrv_image_desc out_desc, int flags);
int rrv_composite_grid(int B, int DH, int DW, unsigned* grid, int* pixels_per_pass);

/* JPEG output: float32 frames encoded as baseline JPEG on the GPU, one stream per frame, so that a compressed frame is what leaves HBM.
 * Input, per frame, float32 HWC BGR PIXEL values v of H x W, contiguous: what the float32 forms of the other stages deliver.
 * Parameters travel with the call in an rrv_jpeg, never in the handle: quality 1..100; chroma 420, 422 or 444; restart, the MCUs per restart
 * interval, 1..65535, or 0 for the library's choice, one MCU row per interval (rrv_jpeg_plan reports the interval actually used).
 * Samples.  Per component the 8-bit code the YUV output forms define, with the BT.601 full-range matrix (rrv_yuv_matrix's values for
 * RRV_YUV_BT601, full_range = 1) whatever matrix the handle holds: c_k, the chroma box mean of the unrounded c_1 / c_2, the clamp and rint half
 * to even of "Output size".  The planes coded are therefore, bit for bit, the I420 / I422 / I444 frame the delivery stage writes for the same
 * frames with that matrix set.  Rows and columns beyond a plane, up to the next whole MCU (16 x 16, 16 x 8 or 8 x 8 pixels), repeat the
 * plane's last sample.
 * Transform and quantisation.  Sample - 128; the 8 x 8 DCT-II with JPEG's normalisation, F(u,v) = C(u) C(v) / 4 sum_xy f(x,y) cos((2x+1) u pi/16)
 * cos((2y+1) v pi/16), C(0) = 1/sqrt 2, in float32; the Annex K tables scaled the IJG way (s = 5000 / quality below 50, else 200 - 2 quality;
 * (base s + 50) / 100 in integers, clamped to 1..255); coefficient = rint(F / Q).  The contract is the rounding of the exact quotient: a value
 * within float32 error of a rounding boundary may go either way.
 * Coefficient blocks: int16 [B][blocks][64], a block's 64 values in zigzag order, the blocks of a frame in scan order: MCUs row by row, in an
 * MCU Y's blocks row by row, then Cb, then Cr.
 * Stream.  One baseline sequential frame: SOI, APP0 (JFIF 1.01, no density), two DQT (luma 0, chroma 1), SOF0 (8 bits, three components, Y
 * sampled 2x2 / 2x1 / 1x1, chroma 1x1), four DHT with the Annex K tables (DC 0, AC 0, DC 1, AC 1), DRI, one interleaved SOS, the
 * entropy-coded intervals, EOI.  An interval is padded with 1-bits to a byte and followed by RST0..7 in rotation, except the last; DC prediction
 * restarts at every interval; every 0xFF data byte is followed by 0x00.  The bytes are a function of the coefficient blocks and the three
 * parameters only.  A DC coefficient outside -1024..1023 or an AC one outside -1023..1023 (the first half produces none) is coded as the
 * nearest end of its range.
 * Where it is written.  Frame b goes to d_out + b * cap and its byte count to d_sizes[b].  Nothing is ever written at or beyond cap bytes of a
 * slot.  A frame that does not fit gets d_sizes[b] = -(the bytes it needs), its slot's content is unspecified, the other frames are unaffected
 * and the call still returns RRV_OK: the sizes are device results.
 *   rrv_jpeg_tables          the two quantisation tables of a quality, natural order; no handle, no GPU
 *   rrv_jpeg_bound           a capacity no frame of H x W can exceed: every block at its longest code with every byte stuffed; no handle, no GPU
 *   rrv_jpeg_plan            MCU columns and rows, the interval used, blocks per frame and header bytes; no handle, no GPU
 *   rrv_jpeg_blocks_device   the first half alone: B (1..64) contiguous frames d_in -> d_coef (16-byte aligned), queued on hip_stream (NULL: the
 *                            null stream); nothing of the handle's own streams takes part
 *   rrv_jpeg_entropy_device  the second half alone: coefficient blocks -> streams and sizes, queued the same way.  Interval lengths and offsets
 *                            live in a buffer of the handle (8 bytes per interval and frame, grow-only): calls on different streams must be
 *                            ordered by the caller
 *   rrv_jpeg_encode_device   both halves, the blocks in a buffer of the handle (128 bytes per block, grow-only); equals the two calls above bit
 *                            for bit
 *   rrv_transfer_jpeg_view_device
 *                            rrv_transfer_composite_view_device with JPEG as the output form: its arguments up to the request c (NULL: none), then
 *                            the rrv_jpeg, the slots d_out, cap and d_sizes in place of the output buffer and view.  Every combination of SH x SW,
 *                            DH x DW, guide (r, eps) and compositing that entry accepts; the frame encoded is the float32 HWC BGR PIXEL frame it
 *                            would deliver, which stays in the workspace slot.  GLOBAL or (RRV_TF_FRAME_MODE) FRAME model
 *   rrv_transfer_jpeg        the host twin, any B: host frames (uint8 HWC BGR or a YUV layout, as rrv_transfer_composite takes them), host `out`
 *                            and host `sizes`, a host matte.  Sub-batches alternate over two compute slots and two staging sets: a
 *                            sub-batch's sizes are read back, then sizes[b] bytes of every frame that fitted are copied, so only those bytes
 *                            cross PCIe, while the GPU runs the next sub-batch
 * A transfer with JPEG output equals, bit for bit in a fixed kernel mode, the float32 HWC BGR PIXEL call with the same sizes, guide and request
 * followed by rrv_jpeg_encode_device; a frame's bytes do not depend on B or on its position in the call.
 * Checks, all before any GPU work: the batch, the sizes (1..65535, and rrv_jpeg_bound below 2^31), quality, chroma, restart, cap (at least the
 * header and EOI), null or misaligned buffers, and for the transfer entries those of the entry without JPEG; RRV_E_ARG names the field and the
 * handle stays usable.  Scratch (128 bytes per block for the coefficients, 8 per interval) is grow-only, per workspace slot for the transfer
 * entries and in the handle for the stage alone, and reserved with the other stage buffers before the call's first launch: out of memory is
 * RRV_E_NOMEM and the handle stays usable.  Results do not depend on what the scratch held before.  These buffers are plain allocations: the
 * guard bands of rrv_set_debug do not cover them.
 * Not offered: blended and masked models, tickets and the one-frame entries. */
typedef struct rrv_jpeg {
    int quality;             /* 1..100 */
    int chroma;              /* 420, 422 or 444 */
    int restart;             /* MCUs per restart interval, 1..65535; 0: one MCU row */
} rrv_jpeg;
int rrv_jpeg_tables(int quality, uint16_t luma[64], uint16_t chroma[64]);
int rrv_jpeg_bound(int H, int W, int chroma, int restart, size_t* bytes);
int rrv_jpeg_plan(int H, int W, int chroma, int restart, int* mcu_cols, int* mcu_rows, int* interval, int* blocks, int* header_bytes);
int rrv_jpeg_blocks_device(rrv_handle h, const float* d_in, int B, int H, int W, const rrv_jpeg* p, int16_t* d_coef, void* hip_stream);
int rrv_jpeg_entropy_device(rrv_handle h, const int16_t* d_coef, int B, int H, int W, const rrv_jpeg* p, uint8_t* d_out, size_t cap,
                            int* d_sizes, void* hip_stream);
int rrv_jpeg_encode_device(rrv_handle h, const float* d_in, int B, int H, int W, const rrv_jpeg* p, uint8_t* d_out, size_t cap,
                           int* d_sizes, void* hip_stream);
int rrv_transfer_jpeg_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int H, int W,
                                  int DH, int DW, int r, float eps, const rrv_composite* c, const rrv_jpeg* p, uint8_t* d_out, size_t cap,
                                  int* d_sizes, int flags, void* hip_stream);
int rrv_transfer_jpeg(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int H, int W, int DH, int DW, int r,
                      float eps, const rrv_composite* c, const rrv_jpeg* p, uint8_t* out, size_t cap, int* sizes, int flags);

/* JPEG input: one baseline JPEG stream per frame decoded on the GPU into the 8-bit planar frame the YUV-input forms read ("8-bit YUV 4:2:0
 * INPUT", "Chroma formats"), so that a compressed frame is what enters HBM.
 * Streams taken.  Baseline sequential (SOF0), 8 bits; three components (any ids) that are YCbCr, Y sampled 1x1, 2x1 or 2x2 and both chroma
 * components 1x1 (chroma 444, 422, 420), or one component (grey, chroma 400); one scan, interleaved for three components, Ss = 0, Se = 63,
 * Ah = Al = 0; any number of DQT / DHT segments with 8-bit quantisers and table ids 0..1, the last definition before SOS holding; no DHT at all
 * means the Annex K tables (MJPG in AVI); DRI present or not; APPn / COM segments and fill bytes; a missing EOI, or bytes behind it.
 * rrv_jpeg_parse refuses everything else in words (why): progressive, extended, lossless and arithmetic frames, 12-bit samples, 16-bit
 * quantisers, other sampling factors, two or four components, an APP14 Adobe segment whose transform is not YCbCr, a scan that does not code
 * all components (several scans), a table a scan names and nobody defined, code lengths that over-subscribe the code space, H or W of 0, a
 * header that ends early.  It reads SOI .. SOS only, on any byte string, and needs no handle and no GPU: RRV_OK, RRV_E_DATA with the reason, or
 * RRV_E_ARG for a null pointer.  All frames of one call share H, W and chroma; tables and restart intervals may differ frame by frame.
 * Entropy half.  The scan's bytes become coefficient blocks in the layout of "JPEG output": int16 [B][blocks][64], a block's values in zigzag
 * order, the blocks in scan order (grey: one block per MCU).  It is a function of the stream alone, so for this library's own streams it is
 * the inverse of rrv_jpeg_entropy_device bit for bit.  A marker is FF followed by a byte that is neither 00 nor FF.  With DRI the scan has
 * `intervals` intervals: marker k < intervals - 1 must be RST(k mod 8) and ends interval k; the next marker (EOI as a rule; it must not be a
 * restart marker) or the stream's end ends the last; nothing behind it is read.  Without DRI the one interval ends at the first marker or the
 * stream's end.  DC prediction starts from 0 in every interval; FF 00 is the data byte FF.
 * Pixel half.  Per block: coefficient x the component's quantiser; the 8 x 8 inverse DCT with JPEG's normalisation, f(x,y) = 1/4 sum_uv C(u)
 * C(v) F(u,v) cos((2x+1) u pi/16) cos((2y+1) v pi/16), C(0) = 1/sqrt 2, in float32; + 128, clamped to 0..255, rint half to even.  The contract
 * is the rounding of the exact value: a value within float32 error of a half-integer may go either way.
 * Planes.  Y is H x W, Cb and Cr CH x CW with CH = ceil(H / vs), CW = ceil(W / hs); the MCU padding is dropped.  A frame is [Y][Cb][Cr],
 * frame_bytes = H W + 2 CH CW, frame b at b * frame_bytes: RRV_LAY_I420 / _I422 / _I444 of "YUV input".  Grey is an I444 frame whose chroma
 * planes hold 128.  The stage upsamples no chroma: a decoded frame enters the network through the YUV-input arithmetic (which replicates
 * chroma, and says why nothing better would show), with rrv_yuv_input_matrix(RRV_YUV_BT601, full_range = 1), JFIF's colour space.
 * Status.  d_status[b] is 0 for a decoded frame, else one of RRV_JPEG_ST_* (rrv_jpeg_status_words gives the words).  A failed frame leaves
 * unspecified content in its own blocks and planes only; the other frames of the call are unaffected and the call still returns RRV_OK: the
 * statuses are device results, as the encoder's sizes are.  Corrupt bytes cannot make a kernel loop or store outside the frame's own blocks:
 * every loop runs over block and coefficient counts, never over the data.
 *   rrv_jpeg_parse           stream -> rrv_jpeg_info
 *   rrv_jpeg_scan_device     the entropy half alone: B (1..64) streams, frame b at d_streams + b * cap, with their parsed infos (host) -> d_coef
 *                            (16-byte aligned) and d_status, queued on hip_stream (NULL: the null stream); nothing of the handle's own streams
 *                            takes part.  The frame descriptors (about 4 KB per frame) and the interval starts live in buffers of the handle
 *                            (grow-only): calls on different streams must be ordered by the caller
 *   rrv_jpeg_planes_device   the pixel half alone: coefficient blocks -> planes, queued the same way (the infos give the size and quantisers)
 *   rrv_jpeg_decode_device   both halves, the blocks in a buffer of the handle (128 bytes per block, grow-only); equals the two calls above bit
 *                            for bit
 * Checks, all before any GPU work: the batch, the infos (one size and chroma format; fields that hold together, as rrv_jpeg_parse fills them),
 * cap against every frame's scan, null or misaligned buffers; RRV_E_ARG names the field and the handle stays usable.  Scratch is reserved
 * before the call's first launch: out of memory is RRV_E_NOMEM and the handle stays usable.  Results do not depend on what the scratch held
 * before.  These buffers are plain allocations: the guard bands of rrv_set_debug do not cover them.
 * As an input form.  rrv_transfer_from_jpeg_view_device is rrv_transfer_composite_view_device with JPEG streams in place of the input buffer and
 * view: d_streams, cap and the parsed infos (B 1..64), then the working size (0, 0: the streams' own size; else the decoded frames are resampled
 * to it, "Scaling"), then that entry's DH, DW, r, eps, request c (NULL: none), output buffer and view, then d_status, the flags and the stream.
 * The decode is queued on hip_stream (NULL: the null stream) into a buffer of the handle and the transfer is ordered behind it on that stream
 * (RRV_TF_ON_STREAM is implied); GLOBAL or (RRV_TF_FRAME_MODE) FRAME model; every output form.  rrv_transfer_jpeg_from_jpeg_view_device is its twin
 * with JPEG as the output form too (the arguments of rrv_transfer_jpeg_view_device behind the request).  A transfer from JPEG equals, bit for bit
 * in a fixed kernel mode, rrv_jpeg_decode_device followed by the same entry reading those planes (RRV_LAY_I420 / _I422 / _I444) with
 * rrv_yuv_input_matrix(RRV_YUV_BT601, 1) installed -- whatever matrix the handle holds, which is put aside while the call queues its launches
 * and is unchanged afterwards.  All checks, the decode's and those of the transfer behind
 * it (sizes, guide, request, output view or rrv_jpeg and cap, flags, the model's state), run before anything is queued or copied; the host
 * twins make them on their first sub-batch's request once every stream is parsed.  (rrv_add_from_jpeg judges the stream first and the frame
 * rules of rrv_add after the decode has run into the handle's scratch.)
 * Host twins, any B: rrv_transfer_from_jpeg and rrv_transfer_jpeg_from_jpeg take B host pointers and sizes, parse every stream first (a stream
 * the parser refuses: RRV_E_DATA, the message names the frame and the reason, nothing has run), copy each frame's own bytes, run sub-batches of
 * sixteen one after the other on the handle's first stream and read the statuses back per sub-batch: a corrupt frame is RRV_E_DATA naming its
 * index (frames of earlier sub-batches have been written), and the handle stays usable.  `out`: a contiguous output of descriptor `od`
 * (rrv_transfer_from_jpeg), or slots of out_cap bytes and host sizes (rrv_transfer_jpeg_from_jpeg, which takes strengths and keep but no matte).
 * A host matte of rrv_transfer_from_jpeg is uploaded per sub-batch.  rrv_add_from_jpeg: rrv_add for a sampled frame that is a host JPEG stream
 * (working size 0, 0: its own): decoded on the GPU and added as the float32 PIXEL frame "Scaling" makes of the planes with the same matrix (at
 * the stream's own size every tap weight is 1), not deferred; RRV_E_DATA for a refused or corrupt stream.  Not offered: blended and masked
 * models, tickets, the one-frame entries.
 * A stream without restart intervals is decoded by one lane per frame: correct, and slow (DESIGN.md says how slow); the frames of a call still
 * run side by side. */
#define RRV_JPEG_ST_DATA 1               /* the entropy-coded data ran out */
#define RRV_JPEG_ST_CODE 2               /* invalid Huffman code */
#define RRV_JPEG_ST_RUN 3                /* a run past coefficient 63 */
#define RRV_JPEG_ST_CATEGORY 4           /* magnitude category out of range (DC above 11, AC above 10) */
#define RRV_JPEG_ST_MARKER_MISSING 5     /* fewer restart markers than the plan has intervals */
#define RRV_JPEG_ST_MARKER_WRONG 6       /* a marker that is not the restart marker expected in rotation */
#define RRV_JPEG_ST_MARKER_SURPLUS 7     /* a restart marker behind the last interval */
typedef struct rrv_jpeg_info {
    int H, W;
    int chroma;                  /* 400, 420, 422 or 444 */
    int components;              /* 1 or 3 */
    int interval;                /* MCUs per restart interval; 0: none */
    int mcu_cols, mcu_rows;
    int blocks;                  /* per frame */
    int intervals;               /* per frame; 1 without DRI */
    int reserved;
    size_t scan_offset;          /* of the scan's bytes in the stream ... */
    size_t scan_bytes;           /* ... and from there to the stream's end */
    uint8_t q[3][64];            /* the quantisers per component, natural order */
    uint8_t huff_dc[3];          /* per component: which DC specification (0 / 1) ... */
    uint8_t huff_ac[3];          /* ... and which AC one */
    uint8_t huff_given;          /* 0: no DHT in the stream, the specifications are Annex K's */
    uint8_t pad;
    uint8_t huff_bits[4][16];    /* the four Huffman specifications, DC 0, DC 1, AC 0, AC 1: codes per length 1..16 ... */
    uint8_t huff_vals[4][256];   /* ... and the symbols in code order */
} rrv_jpeg_info;
int rrv_jpeg_parse(const uint8_t* stream, size_t size, rrv_jpeg_info* info, char* why, size_t why_len);
const char* rrv_jpeg_status_words(int status);
int rrv_jpeg_scan_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, int16_t* d_coef, int* d_status,
                         void* hip_stream);
int rrv_jpeg_planes_device(rrv_handle h, const int16_t* d_coef, const rrv_jpeg_info* infos, int B, uint8_t* d_planes, void* hip_stream);
int rrv_jpeg_decode_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, uint8_t* d_planes, int* d_status,
                           void* hip_stream);
int rrv_transfer_from_jpeg_view_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, int work_H, int work_W, int DH,
                                       int DW, int r, float eps, const rrv_composite* c, void* d_out, const rrv_image_view* out, int* d_status, int flags,
                                       void* hip_stream);
int rrv_transfer_jpeg_from_jpeg_view_device(rrv_handle h, const uint8_t* d_streams, size_t cap, const rrv_jpeg_info* infos, int B, int work_H, int work_W,
                                            int DH, int DW, int r, float eps, const rrv_composite* c, const rrv_jpeg* p, uint8_t* d_out, size_t out_cap,
                                            int* d_sizes, int* d_status, int flags, void* hip_stream);
int rrv_transfer_from_jpeg(rrv_handle h, const uint8_t* const* streams, const size_t* sizes, int B, int work_H, int work_W, int DH, int DW, int r, float eps,
                           const rrv_composite* c, void* out, rrv_image_desc od, int flags);
int rrv_add_from_jpeg(rrv_handle h, const uint8_t* stream, size_t size, int work_H, int work_W);
int rrv_transfer_jpeg_from_jpeg(rrv_handle h, const uint8_t* const* streams, const size_t* sizes, int B, int work_H, int work_W, int DH, int DW, int r,
                                float eps, const rrv_composite* c, const rrv_jpeg* p, uint8_t* out, size_t out_cap, int* out_sizes, int flags);

/* ---- Shots: the signature a cut detector compares, computed on the GPU for every frame of a video.
 * The saved state (statistics, clamp range, predicted filters) belongs to one sequence.  A file with cuts is several: the driver detects the
 * cuts, then runs clean / add / compute once per shot (INTEGRATION.md "Shots").  The library supplies what has to see every frame: the
 * signature.  The rule that turns signatures into cuts is host arithmetic (video.shot_distances, video.detect_cuts).
 * Signature.  uint32 sig[16][32] per frame = RRV_SHOT_SIG_WORDS words: a 32-bin luma histogram for each cell of a 4 x 4 grid over a float32
 * [H][W][3] BGR PIXEL frame, H, W >= 4 (smaller: RRV_E_ARG), cell cy * 4 + cx.  Integer arithmetic from the first step on, so it is exact
 * (video.shot_signature restates it in numpy and the GPU equals it word for word):
 *   per channel  c8 = clamp(rint(v), 0, 255), rint half to even; written so that !(v > 0) gives 0: NaN and -inf give 0, +inf gives 255;
 *   luma         Y = (29 B8 + 150 G8 + 77 R8 + 128) >> 8, 0..255;   bin = Y >> 3;
 *   cell         pixel (y, x) lies in cell ((4 y) / H, (4 x) / W), integer division: cell row cy holds the rows ceil(cy H / 4) ..
 *                ceil((cy + 1) H / 4) - 1, the columns alike.
 * Every cell's counts sum to its pixel count.  The kernel uses no global atomics and zeroes nothing: every output word is written exactly once
 * by one thread, so the result is deterministic and depends neither on B nor on what d_sig held before.
 * Thumbnail.  The signature is taken from a thumbnail, so that its cost does not grow with the frame and film grain does not reach it.
 * rrv_shot_plan (no handle, no GPU): f = the smallest integer in 1..8 with ceil(max(SH, SW) / f) <= 512, or 8 if there is none; th =
 * ceil(SH / f), tw = ceil(SW / f).  512 x 512 stays, 1080 x 1920 and 2160 x 3840 become 270 x 480, 4320 x 7680 becomes 540 x 960.  The ratio
 * of either axis is at most 8, the resampler's limit ("Scaling"); a frame whose thumbnail falls below 4 x 4 is RRV_E_ARG.
 *   rrv_shot_signature_device          the kernel alone: B (1..64) contiguous frames at d_frames -> d_sig [B][16][32], queued on hip_stream
 *                                      (NULL: the null stream); nothing of the handle's own streams takes part
 *   rrv_shot_signature_view_device     B (1..64) frames of SH x SW in any input form, view or surface the resampler reads, resampled to the
 *                                      plan's thumbnail, then the kernel; by definition rrv_resample_view_device to (th, tw) followed by
 *                                      rrv_shot_signature_device, bit for bit.  The thumbnails live in a buffer of the handle (float32,
 *                                      grow-only), reserved with the tap tables before anything is queued: out of memory is RRV_E_NOMEM and
 *                                      the handle stays usable.  Calls on different streams must be ordered by the caller
 *   rrv_shot_signature                 the host twin, any B >= 1: uint8 HWC BGR frames or any YUV layout with its sample type, as
 *                                      rrv_transfer_scaled takes them, contiguous; sub-batches of sixteen through a staging buffer, one after
 *                                      the other on the handle's first stream; synchronous (sig is written when it returns)
 *   rrv_shot_signature_from_jpeg       the host twin for baseline JPEG streams ("JPEG input"): every stream parsed first (a stream the parser
 *                                      refuses: RRV_E_DATA naming the frame, nothing has run), decoded by the JPEG input stage, the signature
 *                                      taken from the planes with rrv_yuv_input_matrix(RRV_YUV_BT601, 1) installed for the call (the handle's
 *                                      matrix is put aside and unchanged afterwards).  One size and chroma format per call (RRV_E_ARG naming
 *                                      the frame); a corrupt frame is RRV_E_DATA naming its index, and the handle stays usable
 * All checks run before any GPU work.  What is reserved before anything is queued is the thumbnail buffer, the tap tables and the host twins'
 * staging; the JPEG twin's decode scratch is reserved per sub-batch behind the upload of its streams, as in the other from-JPEG host twins
 * (out of memory there is RRV_E_NOMEM too, and the handle stays usable).  Not offered: tickets, pipelined host twins. */
#define RRV_SHOT_SIG_WORDS 512
int rrv_shot_plan(int SH, int SW, int* th, int* tw);
int rrv_shot_signature_device(rrv_handle h, const float* d_frames, int B, int H, int W, uint32_t* d_sig, void* hip_stream);
int rrv_shot_signature_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, uint32_t* d_sig, void* hip_stream);
int rrv_shot_signature(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, uint32_t* sig);
int rrv_shot_signature_from_jpeg(rrv_handle h, const uint8_t* const* streams, const size_t* sizes, int B, uint32_t* sig);

/* ---- Picture area: the active picture of letterboxed and pillarboxed frames, found on the GPU and stylized as a window of the frame.
 * A 2.39:1 film in a 16:9 container is a quarter black.  Stylized whole, the bars enter the saved state's statistics, come out as texture,
 * bend the stroke pattern at their edge, take a quarter of every kernel's time, and subtitles inside them are painted over.  A matte fixes
 * only what is shown.  The library supplies what has to see every frame (the line profile), the window as part of a call, and the
 * entries that stylize inside it; the rule that turns profiles into a window is host arithmetic (video.detect_picture).
 * Line profile.  uint32 prof[H + W] per frame: row_cnt[H], the number of lit pixels of every row, then col_cnt[W], of every column, of a
 * float32 [H][W][3] BGR PIXEL frame, H, W >= 8 (smaller: RRV_E_ARG).  Integer arithmetic from the rounding on, with the shot signature's luma,
 * so it is exact (video.picture_profile restates it in numpy and the GPU equals it word for word):
 *   per channel  c8 = clamp(rint(v), 0, 255), rint half to even; written so that !(v > 0) gives 0: NaN and -inf give 0, +inf gives 255;
 *   luma         Y = (29 B8 + 150 G8 + 77 R8 + 128) >> 8, 0..255;   a pixel is lit iff Y > threshold, threshold in 0..254 (else RRV_E_ARG).
 * Per frame sum(row_cnt) == sum(col_cnt).  RRV_PICTURE_THRESHOLD = 10 is ffmpeg cropdetect's default of 24 on limited-range codes, moved to
 * the full-range values the first kernel produces; like the rule's defaults it has not been tuned on real footage.  The kernels use no global
 * atomics and zero nothing: every output word is written exactly once by one thread, so the result is deterministic and depends neither on
 * B nor on what d_prof held before.
 * Window.  rrv_picture {y0, x0, h, w}: rows y0 .. y0 + h - 1 and columns x0 .. x0 + w - 1 of an SH x SW frame.  One rule for every layout,
 * so that a chroma sample never straddles the edge (rrv_picture_check; no handle, no GPU; RRV_OK or RRV_E_ARG, and the entries below name
 * the field in rrv_last_error): y0, x0 even and >= 0; h, w >= 8; y0 + h <= SH, x0 + w <= SW; h even unless y0 + h == SH; w even unless
 * x0 + w == SW.
 * rrv_picture_view (no handle, no GPU) turns the view of the whole frames into the view of the window: plane offsets move by y0 rows and x0
 * samples (three elements per pixel for RRV_LAY_HWC_BGR), for chroma planes by the layout's subsampling (y0 >> csy rows, x0 >> csx samples,
 * times two for interleaved CbCr); pitches and the frame stride stay.  The result with the frame size h x w is an ordinary view: "a view
 * has no semantics of its own".  RRV_E_ARG for a null pointer, an unknown descriptor or a refused window.
 *   rrv_picture_profile_device         the kernels alone: B (1..64) contiguous frames at d_frames -> d_prof [B][H + W], queued on hip_stream
 *                                      (NULL: the null stream); the column scratch lives in a grow-only buffer of the handle
 *   rrv_picture_profile_view_device    B (1..64) frames of SH x SW in any input form, view or surface the resampler reads; by definition
 *                                      rrv_resample_view_device to (SH, SW), the equal-size identity, followed by rrv_picture_profile_device,
 *                                      bit for bit.  The float frames and the scratch live in grow-only buffers of the handle, reserved with
 *                                      the tap tables before anything is queued: out of memory is RRV_E_NOMEM and the handle stays usable.
 *                                      Calls on different streams must be ordered by the caller
 *   rrv_scan_frames                    the host twin of the whole detection pass, any B >= 1: host frames as rrv_shot_signature takes them;
 *                                      every sub-batch (at most sixteen frames and 16 x 640 x 640 x 4 source pixels, the scaled host twins'
 *                                      budget) is uploaded once, one after the other on the handle's first stream.  sig (NULL: none) is, word
 *                                      for word, what rrv_shot_signature returns for the same frames, [B][512]; prof (NULL: none) what the
 *                                      view entry returns, [B][SH + SW].  Both NULL is RRV_E_ARG.  Synchronous
 * Add.  rrv_add_picture_view_device / rrv_add_picture are by definition rrv_add_scaled_view_device with the window's view, SH := p->h,
 * SW := p->w, bit for bit in the saved state; H, W is the working size, 0, 0 the window's own.  (The host twin uploads the whole frame.)
 * Transfer.  The delivered frame has the source's size SH x SW.  By definition, bit for bit in a fixed kernel mode:
 *   1  canvas = the resampler alone on the whole source at equal size: the float32 HWC BGR PIXEL value the first kernel derives from each
 *      source pixel, whatever the input form;
 *   2  canvas[:, y0:y0+h, x0:x0+w] = the float32 HWC BGR PIXEL result of rrv_transfer_composite_view_device on the window's view with
 *      SH := h, SW := w, the working size H x W (0, 0: the window's), DH := h, DW := w, and the call's r, eps (the guide is the window of the
 *      source), c (a matte has the window's size [.][h][w]) and flags;
 *   3  the output = canvas through the delivery stage at equal size into `out`: every output form, YUV layout, depth, chroma format and
 *      pitched view is word for word that of "Output size".
 * So outside the window a uint8 BGR output of a uint8 BGR source is the source's bytes.  RRV_TF_PAD_CROP is forced; the other flags taken
 * are RRV_TF_FRAME_MODE and RRV_TF_ON_STREAM (models: the global and the frame-mode one).  A window equal to the whole frame is exactly
 * the composite entry without a window: no kernel is added and every bit is what it was.  The request is placed by the delivery stage
 * writing a float32 view with the canvas's pitch (or by the last kernel itself where nothing is staged), so no kernel of the other six
 * libraries changes.  The canvas lives in a grow-only buffer per workspace slot (12 bytes per source pixel and frame of a launch group).
 * rrv_transfer_picture is the host twin through the host pipeline like rrv_transfer_composite, any B >= 1; its sub-batches follow the whole
 * frame's pixel count.  All checks run before any GPU work, the buffers are reserved before the first launch, RRV_E_NOMEM leaves the handle
 * usable.  Not offered: JPEG input and output forms with a window, blended and masked models, tickets and the one-frame entries. */
#define RRV_PICTURE_THRESHOLD 10
typedef struct rrv_picture { int y0, x0, h, w; } rrv_picture;     /* window of an SH x SW frame, in pixels */
int rrv_picture_check(int SH, int SW, const rrv_picture* p);
int rrv_picture_view(const rrv_image_view* full, int SH, int SW, const rrv_picture* p, rrv_image_view* win);
int rrv_picture_profile_device(rrv_handle h, const float* d_frames, int B, int H, int W, int threshold, uint32_t* d_prof, void* hip_stream);
int rrv_picture_profile_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, int threshold, uint32_t* d_prof,
                                    void* hip_stream);
int rrv_scan_frames(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, int threshold, uint32_t* sig, uint32_t* prof);
int rrv_add_picture_view_device(rrv_handle h, const void* d_frame, const rrv_image_view* in, int SH, int SW, const rrv_picture* p, int H, int W,
                                void* hip_stream);
int rrv_add_picture(rrv_handle h, const void* frame, rrv_image_desc in, int SH, int SW, const rrv_picture* p, int H, int W);
int rrv_transfer_picture_view_device(rrv_handle h, const void* d_in, const rrv_image_view* in, int B, int SH, int SW, const rrv_picture* p, int H, int W,
                                     int r, float eps, const rrv_composite* c, void* d_out, const rrv_image_view* out, int flags, void* hip_stream);
int rrv_transfer_picture(rrv_handle h, const void* frames, rrv_image_desc in, int B, int SH, int SW, const rrv_picture* p, int H, int W,
                         int r, float eps, const rrv_composite* c, void* out, rrv_image_desc out_desc, int flags);

/* Debug/parity taps: pre-clamp network output (normalised RGB, NHWC [H][W][3]) of the last
 * transfer, copied to host. */
int rrv_get_preclamp(rrv_handle h, float* out, int H, int W);
/* The same tap for image `b` of the last launch (a batched entry runs up to 64 frames per launch; for the host-buffer
 * entries the last launch is the last sub-batch of the call). */
int rrv_get_preclamp_image(rrv_handle h, float* out, int H, int W, int b);

int rrv_sync(rrv_handle h);

/* Consecutive rrv_transfer[_batch]_device calls alternate over n_slots (1..RRV_MAX_SLOTS, default 2) internal
 * (HIP stream, workspace) pairs, so n_slots independent batches are in flight and one batch's kernel
 * tails overlap the other's kernels.  Callers must give consecutive calls distinct output buffers
 * and call rrv_sync() before reading them.  Host-buffer entries and blend transfers are serialised. */
int rrv_set_pipeline(rrv_handle h, int n_slots);

/* The persistent grids of the transform-domain kernels normally take every CU (one workgroup each).  share = 2..4 gives
 * each launch 1/share of them, so that the launches of `share` streams run side by side instead of queueing behind each
 * other's last partial round — for callers that keep several SMALL batches in flight (one frame per call with
 * look-ahead).  Results do not depend on it. */
int rrv_set_grid_share(rrv_handle h, int share);

/* How the host-buffer entries (rrv_transfer, _batch, _frames, _async) cross PCIe.  0 (default): staged — H2D copy into
 * HBM, kernels, D2H copy, on dedicated copy streams.  1: zero copy — the first kernel reads the uint8 frames straight
 * from page-locked host memory and the last one stores the stylized frame there (caller buffers if they are
 * page-locked, the library's pinned staging otherwise): no copy kernels, no copy-stream events.  2 / 3: zero copy for the
 * input / the output only, the other direction staged.  Same results bit for bit. */
int rrv_set_host_io(rrv_handle h, int mode);

/* Debugging aid: activation tensor `index` (0..8 encoder c11 p1 c21 p2 c31 c32 c33 p3 c41, 9..22 decoder d f1 f2 f3 xs4 a4
 * o4 xs3 a3 o3 xs2 a2 o2 dpart) of workspace slot `slot` for frames of H x W, first image, ring layout [H'+2][W'+2][C],
 * copied to the host after a full synchronisation.  *floats receives its size (nothing is copied when cap is smaller). */
int rrv_debug_copy_tensor(rrv_handle h, int slot, int index, int H, int W, float* host, size_t cap, size_t* floats);

/* Layer-parity tap: as rrv_debug_copy_tensor, for image `image` of the plan, with indices 23..32 the channel-chunk-major
 * twins q11 q1 q21 q2 q31 q32 q33 (encoder) and qa4 qa3 qa2 (ResidualBlock.conv1 outputs), and indices 33..36 the level
 * masks of a masked multi-style launch at stride 1, 2, 4, 8 of the network's frame: RRV_MAX_STYLES-channel ring-layout
 * tensors, row y + 1 holding the w * S weights of that row's pixels (S innermost) from its first interior pixel on, every
 * other float 0.  *layout = 0: ring-layout NHWC [H'+2][W'+2][C]; 1: "P8" [C/8][H'+2][W'+8][8], pixel x at stored column
 * x + 4.  *channels = C.  RRV_E_STATE when the most recent launch on that workspace plan did not write the tensor for that
 * image (stale data, the other layout, a level mask after a launch without masks, image 1.. of a launch with one mask for
 * every image), so a caller never reads stale data. */
int rrv_debug_copy_tensor_ex(rrv_handle h, int slot, int index, int image, int H, int W, float* host, size_t cap, size_t* floats,
                             int* layout, int* channels);

/* Layer-parity read-back of the per-image numbers of a launch, copied to the host after a full synchronisation; nothing
 * else changes.
 *   what = RRV_DBG_STATE_SET: the state set of image `image` as the most recent launch on workspace slot `slot` (0 or 1)
 *     wrote it — a frame-mode launch (every image's statistics, predicted filters and the identity Decoder.norm[1] entry)
 *     or a grouped multi-style launch (every image's blended state).  Same blob layout as rrv_get_state,
 *     n == RRV_STATE_FLOATS.  RRV_E_STATE when the last launch on that slot kept no per-image state or did not write
 *     that image.
 *   what = RRV_DBG_STYLE_PRED: the style half of the filter predictions of prepared style `image` (mean over H x W of
 *     Filter1..3's F1 / F2 down_sample of the normalised style map: [6][32] floats, n == 192); `slot` must be 0.
 *     RRV_E_STATE when that style has not been prepared. */
/*   what = RRV_DBG_STYLE_BLOB: the state blob of prepared style `image` as it stands, computed or not (after a pass that
 *     rrv_debug_prep_stop ended early: the entries up to that sync point and the style statistics); `slot` must be 0,
 *     n == RRV_STATE_FLOATS.  RRV_E_STATE when that style has not been prepared. */
#define RRV_DBG_STATE_SET 0
#define RRV_DBG_STYLE_PRED 1
#define RRV_DBG_STYLE_BLOB 2
int rrv_debug_copy_state(rrv_handle h, int what, int slot, int image, float* out, int n);

/* Layer-parity stop of the preparation pass.  stage = -1 (default): off.  stage = 0..13, one of the pass's sync points in
 * order (0 Decoder.norm[0]; 1..3 Filter1..3: both predictions, the fold, frame 0's two folded convolutions and the residual
 * add; 4 Decoder.norm[1]; 5 + 3k, 6 + 3k, 7 + 3k: norm1, norm2 and the AdaIN norm of residual block k): rrv_compute launches
 * what it always launches up to and including that sync point's statistic and nothing further, for every prepared style,
 * resident or streaming.  Below 13 the styles stay "not computed" (the transfer entries refuse them); 13 is a full pass.
 * Either way the pass's workspace is kept for rrv_debug_copy_prep_tensor until the next rrv_compute, rrv_clean,
 * rrv_destroy, or this knob being switched off. */
int rrv_debug_prep_stop(rrv_handle h, int stage);

/* One image of a tensor of the preparation pass, ring layout [H+2][W+2][C], copied to the host after a full
 * synchronisation; *floats receives its size (nothing is copied when cap is smaller), *H, *W, *C its geometry.
 *   index 0..19: the workspace kept under rrv_debug_prep_stop, in the order cn nxt t32 d32 u xs4 a4 o4 xs3 a3 o3 xs2 a2 o2
 *     content grp f0 su1 su2 su3 (d32, u, f0, su*: one image; content: resident passes; grp, f0, su*: streaming passes);
 *   RRV_DBG_PREP_PATCH: the stored relu4_1 feature of sampled frame `image`;
 *   RRV_DBG_PREP_STYLE_C11 .. + 3: relu1_1, relu2_1, relu3_1, relu4_1 of the style image the last rrv_prepare_style encoded;
 *   RRV_DBG_PREP_MAP: the relu4_1 map of prepared style `image`.
 * RRV_E_STATE for a tensor the last pass did not allocate and for an image beyond the batch. */
#define RRV_DBG_PREP_PATCH 20
#define RRV_DBG_PREP_STYLE_C11 21
#define RRV_DBG_PREP_MAP 25
int rrv_debug_copy_prep_tensor(rrv_handle h, int index, int image, float* host, size_t cap, size_t* floats, int* H, int* W, int* C);

/* Weight read-back (tests/test_gpu_packs.py): every weight buffer the handle holds in HBM after rrv_finalize_weights, as the
 * kernels read it.  rrv_debug_weight_count returns how many there are (>= 0), RRV_E_ARG for a null handle, RRV_E_STATE before
 * rrv_finalize_weights.  Buffer `index` (0 .. count - 1, in a fixed order: the convolutions by checkpoint key, conv1_1, Decoder.slice1,
 * the folded KernelFilters) is described by rrv_debug_weight_info: *key (at most keycap bytes with the terminator; RRV_E_ARG when it
 * does not fit) is the checkpoint prefix of the convolution ("Decoder.Filter<f>.fold_down" / ".fold_up" for a folded KernelFilter),
 * *form one of
 *   RRV_DBG_W_RAW         OIHW as in the checkpoint (a fold: the folded product), Cout * Cin * taps floats
 *   RRV_DBG_W_PK          the direct-form pack [Cout/BN][Cin/16][taps][BN][16], *BN its tile
 *   RRV_DBG_W_PK_WINO     the F(2x2,3x3) pack [Cout/32][Cin/16][16][32][16]
 *   RRV_DBG_W_PK_UPS      the nine-product upsample pack [Cout/32][Cin/16][9][32][16]
 *   RRV_DBG_W_PK_UPS_SC   the five-product upsample pack with the 1 x 1 shortcut [Cout/32][Cin/16][26][32][16]
 *   RRV_DBG_W_PK_F43      the F(4x4,3x3) pack [Cout/32][Cin/8][36][16][4][2][2]
 *   RRV_DBG_W_BIAS        [Cout] (zeros for a bias-free convolution; a folded down_sample: 256 floats, 32 biases and zeros)
 *   RRV_DBG_W_FIRST       conv1_1 as [27][64];  RRV_DBG_W_FIRST_GREY its grey fold, 1216 floats
 *   RRV_DBG_W_LAST        Decoder.slice1 as conv_last_k's MFMA operands [2][4][64][4];  its RRV_DBG_W_BIAS has 4 floats
 * *Cout, *Cin, *taps the convolution's shape, *sets the number of state sets that have a buffer of their own (1: a checkpoint weight;
 * the folded KernelFilters: the handle's state sets), *floats the size of one.  Any out pointer may be null.
 * rrv_debug_copy_weights copies buffer `index` of state set `set` (0 unless *sets > 1) to the host after a full synchronisation;
 * *floats receives its size, nothing is copied when cap is smaller.  RRV_E_ARG for a bad index or set, RRV_E_STATE for the folded
 * weights of a set no launch or state change has folded yet; rrv_last_error says which. */
#define RRV_DBG_W_RAW 0
#define RRV_DBG_W_PK 1
#define RRV_DBG_W_PK_WINO 2
#define RRV_DBG_W_PK_UPS 3
#define RRV_DBG_W_PK_UPS_SC 4
#define RRV_DBG_W_PK_F43 5
#define RRV_DBG_W_BIAS 6
#define RRV_DBG_W_FIRST 7
#define RRV_DBG_W_FIRST_GREY 8
#define RRV_DBG_W_LAST 9
int rrv_debug_weight_count(rrv_handle h);
int rrv_debug_weight_info(rrv_handle h, int index, char* key, size_t keycap, int* form, int* Cout, int* Cin, int* taps, int* BN, int* sets,
                          size_t* floats);
int rrv_debug_copy_weights(rrv_handle h, int index, int set, float* host, size_t cap, size_t* floats);

/* Stream-ordered use of the *_device entries from a caller that produces / consumes the buffers on its own HIP
 * stream (e.g. torch.cuda.current_stream().cuda_stream): see ORDERING above.  enable = 0 switches it off. */
int rrv_set_caller_stream(rrv_handle h, void* hip_stream, int enable);

/* Page-locked host memory for the host-buffer entries (no staging copy, true async DMA): allocate, or pin an
 * existing range in place.  Plain wrappers of hipHostMalloc / hipHostFree / hipHostRegister / hipHostUnregister so
 * that a caller without HIP bindings (ctypes, cgo, JNI) can use them. */
int rrv_host_alloc(size_t bytes, void** out);
int rrv_host_free(void* p);
int rrv_host_register(void* p, size_t bytes);
int rrv_host_unregister(void* p);

/* Bounds-checked debug mode (also RRV_DEBUG=<level> in the environment at rrv_create).  Every activation tensor is
 * allocated between two 64 KB guard bands filled with a canary; level 1 synchronises and checks after every API call,
 * level 2 after every kernel launch (an asynchronous fault or a violation is reported with the kernel's name):
 * guard bands intact, the one-pixel zero ring and the slack rows of every tensor still zero (the kernels rely on both
 * and must never store outside the valid pixels).  A violation returns RRV_E_DEBUG.  Changing the level drops the
 * workspaces (saved state and prepared styles are kept).  rrv_debug_selftest plants one ring store and one guard-band
 * store and returns RRV_OK only if the checker reports both. */
int rrv_set_debug(rrv_handle h, int level);
int rrv_debug_selftest(rrv_handle h);
/* Failure injection: the nth next device allocation of this handle (1 = the very next one) reports out-of-memory
 * (RRV_E_NOMEM, as a real hipErrorOutOfMemory does); 0 disarms.  Workspaces are built transactionally — complete or
 * released — so the call after a failed one starts over instead of finding a half-built plan. */
int rrv_debug_fail_alloc(rrv_handle h, int nth);

/* Per-launch timing with HIP events recorded on the handle's own stream.
 * rrv_profile_begin() clears the log and starts bracketing every kernel launch with
 * events; rrv_profile_end() syncs and freezes the log.  Entry i: kernel name (with "@CinxCout@HxW"
 * for convolutions), elapsed ms, ALGORITHMIC FLOPs (the reference's direct convolution:
 * 2*B*H*W*Cin*Cout*taps) and algorithmic HBM bytes of that launch, and the FLOPs the kernel actually
 * executes (fewer for the Winograd and upsample-folded kernels). */
int rrv_profile_begin(rrv_handle h);
int rrv_profile_end(rrv_handle h);
int rrv_profile_count(rrv_handle h);
int rrv_profile_entry(rrv_handle h, int i, const char** name, float* ms, double* flops, double* bytes,
                      double* flops_executed);
/* The grid of entry i, for the persistent kernels (the transform-domain convolutions and conv_last walk their work items
 * with gridDim.x workgroups): *grid = the launch's grid.x, *xcd_slabs = which of the two item walks a transform-domain
 * launch took (1: the slabs of a pixel tile on one XCD; 0: the plain walk), -1 for a launch that has none (conv_last, the
 * direct-form convolutions).  Every other launch reports *grid = 0, *xcd_slabs = -1. */
int rrv_profile_entry_grid(rrv_handle h, int i, unsigned* grid, int* xcd_slabs);

#ifdef __cplusplus
}
#endif
#endif /* REREVST_HIP_H */

"""ctypes binding of librerevst_hip.so (C ABI: include/rerevst_hip.h).

There is NO CPU fallback: if the shared library is missing or does not load, importing
the symbols raises.  (The numpy oracle under oracle/ is test infrastructure and is never
used from here.)
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# RRV_LIB_PATH: another build of the same library (A/B runs of kernel variants: `python -m rerevst-code_amd.build` with extra -D flags, which
# reach the main library only).  It finds its companion librerevst_stages.so next to ITSELF (rpath $ORIGIN): a library in another directory
# needs a copy of it there (and of librerevst_compose.so, librerevst_jpeg.so, librerevst_jpeg_in.so, librerevst_shots.so and librerevst_picture.so).
LIB_PATH = os.environ.get("RRV_LIB_PATH") or os.path.join(HERE, "librerevst_hip.so")
STATE_FLOATS = 17536
MAX_STYLES = 8

_lib = None


class ImageDesc(C.Structure):
    """rrv_image_desc: element type, layout and value space of the images of rrv_transfer_image_device."""
    _fields_ = [("dtype", C.c_int), ("layout", C.c_int), ("space", C.c_int)]


class ImageView(C.Structure):
    """rrv_image_view: an image descriptor plus where the rows of its planes lie, in elements of desc.dtype (torch's stride unit)."""
    _fields_ = [("desc", ImageDesc), ("frame_stride", C.c_int64), ("plane_offset", C.c_int64 * 3), ("pitch", C.c_int64 * 3)]


class Composite(C.Structure):
    """rrv_composite: a compositing request (per-frame strengths in host memory, the matte, what the source keeps)."""
    _fields_ = [("strength", C.POINTER(C.c_float)), ("matte", C.c_void_p), ("matte_dtype", C.c_int), ("matte_frames", C.c_int), ("keep", C.c_int)]


class Picture(C.Structure):
    """rrv_picture: the window (y0, x0, h, w) of a frame, in pixels (include/rerevst_hip.h "Picture area")."""
    _fields_ = [("y0", C.c_int), ("x0", C.c_int), ("h", C.c_int), ("w", C.c_int)]


class Jpeg(C.Structure):
    """rrv_jpeg: the parameters of a JPEG encode (quality 1..100; chroma 420, 422 or 444; MCUs per restart interval, 0 = one MCU row)."""
    _fields_ = [("quality", C.c_int), ("chroma", C.c_int), ("restart", C.c_int)]


class JpegInfo(C.Structure):
    """rrv_jpeg_info: what rrv_jpeg_parse reads from a baseline JPEG stream's header (include/rerevst_hip.h "JPEG input")."""
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("chroma", C.c_int), ("components", C.c_int), ("interval", C.c_int), ("mcu_cols", C.c_int),
                ("mcu_rows", C.c_int), ("blocks", C.c_int), ("intervals", C.c_int), ("reserved", C.c_int), ("scan_offset", C.c_size_t),
                ("scan_bytes", C.c_size_t), ("q", C.c_uint8 * 64 * 3), ("huff_dc", C.c_uint8 * 3), ("huff_ac", C.c_uint8 * 3), ("huff_given", C.c_uint8),
                ("pad", C.c_uint8), ("huff_bits", C.c_uint8 * 16 * 4), ("huff_vals", C.c_uint8 * 256 * 4)]


E_DATA = -8                       # RRV_E_DATA: a JPEG stream the parser refuses, or a frame whose entropy-coded data is corrupt
DT_U8, DT_F32 = 0, 1
DT_U16 = 2                        # uint16 samples: only with LAY_I420_16 / LAY_P016
LAY_HWC_BGR, LAY_CHW_RGB = 0, 1
LAY_I420, LAY_NV12 = 2, 3         # 8-bit YUV 4:2:0, planar / semi-planar (an ImageDesc names them for an output; an ImageView on either side)
LAY_I420_16, LAY_P016 = 8, 9      # 10 / 12 / 16-bit YUV 4:2:0 in uint16 samples: planar with the code in the low bits / semi-planar with it in the high bits
# chroma subsampling flags, OR-ed onto one of the four YUV layouts above: 4:2:2 (CW = (W+1)/2, CH = H) and 4:4:4 (CW = W, CH = H)
LAY_422, LAY_444 = 0x10, 0x20
LAY_I422, LAY_NV16, LAY_I422_16, LAY_P216 = LAY_I420 | LAY_422, LAY_NV12 | LAY_422, LAY_I420_16 | LAY_422, LAY_P016 | LAY_422      # 18, 19, 24, 25
LAY_I444, LAY_NV24, LAY_I444_16, LAY_P416 = LAY_I420 | LAY_444, LAY_NV12 | LAY_444, LAY_I420_16 | LAY_444, LAY_P016 | LAY_444      # 34, 35, 40, 41
YUV_BT601, YUV_BT709 = 0, 1
SP_PIXEL, SP_UNIT, SP_NORM = 0, 1, 2
KEEP_NONE, KEEP_COLOUR, KEEP_LUMA = 0, 1, 2
TF_PAD_CROP, TF_FRAME_MODE, TF_ON_STREAM, TF_WEIGHTS_DEVICE = 1, 2, 4, 8
DBG_STATE_SET, DBG_STYLE_PRED, DBG_STYLE_BLOB = 0, 1, 2
# rrv_debug_copy_prep_tensor: 0..19 the preparation workspace in this order, then a sampled frame's stored feature, the style
# encoder's four taps and a style's map
PREP_TENSORS = ("cn", "nxt", "t32", "d32", "u", "xs4", "a4", "o4", "xs3", "a3", "o3", "xs2", "a2", "o2", "content", "grp", "f0",
                "su1", "su2", "su3", "patch", "style_c11", "style_c21", "style_c31", "style_c41", "map")
DBG_PREP_PATCH, DBG_PREP_STYLE_C11, DBG_PREP_MAP = 20, 21, 25
# rrv_debug_weight_info: the forms of a weight buffer (RRV_DBG_W_*), by value
WEIGHT_FORMS = ("raw", "pk", "pk_wino", "pk_ups", "pk_ups_sc", "pk_f43", "bias", "first", "first_grey", "last")

# name -> (restype, argtypes); must list every symbol declared in include/rerevst_hip.h
SYMBOLS = {
    "rrv_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "rrv_destroy": (C.c_int, [C.c_void_p]),
    "rrv_last_error": (C.c_char_p, [C.c_void_p]),
    "rrv_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "rrv_finalize_weights": (C.c_int, [C.c_void_p]),
    "rrv_prepare_style": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rrv_clean": (C.c_int, [C.c_void_p]),
    "rrv_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "rrv_compute": (C.c_int, [C.c_void_p]),
    "rrv_set_workspace_cap": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rrv_last_compute_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "rrv_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "rrv_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "rrv_comm_unique_id": (C.c_int, [C.c_char_p]),
    "rrv_comm_init_rank": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rrv_comm_destroy": (C.c_int, [C.c_void_p]),
    "rrv_broadcast_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rrv_transfer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_long)]),
    "rrv_transfer_wait": (C.c_int, [C.c_void_p, C.c_long]),
    "rrv_transfer_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_blend_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "rrv_transfer_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_blend": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "rrv_transfer_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_generate_content_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "rrv_generate_content_features_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "rrv_add_patch": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_transfer_features": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "rrv_transfer_features_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p]),
    "rrv_release_features": (C.c_int, [C.c_void_p]),
    "rrv_set_multistyle_group": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_set_f43": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_set_feature_cache_cap": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rrv_feature_cache_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "rrv_transfer_frame_mode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_frame_mode_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_frame_mode_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_frame_mode_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_frame_mode_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_image_device": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_void_p, ImageDesc,
                                            C.c_int, C.c_void_p]),
    "rrv_transfer_image_blend_device": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                  C.c_void_p, ImageDesc, C.c_int, C.c_void_p]),      # style_weight: host or device address
    "rrv_transfer_blend_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_image_mask_device": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_void_p, ImageDesc, C.c_int, C.c_void_p]),      # d_mask: device address
    "rrv_transfer_mask_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_yuv_matrix": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rrv_set_yuv_matrix": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rrv_transfer_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_transfer_blend_batch_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int,
                                               C.c_void_p]),
    "rrv_transfer_mask_batch_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p]),
    "rrv_yuv_input_matrix": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rrv_set_yuv_input_matrix": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    # 8-bit YUV 4:2:0 input: (h, in, in_layout, B, H, W, [weights, n_styles | mask, n_styles, mask_images,] out, ImageDesc out, flags[, hip_stream])
    "rrv_transfer_from_yuv_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, ImageDesc, C.c_int, C.c_void_p]),
    "rrv_transfer_blend_from_yuv_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                     C.c_void_p, ImageDesc, C.c_int, C.c_void_p]),      # style_weight: host or device address
    "rrv_transfer_mask_from_yuv_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                    C.c_void_p, ImageDesc, C.c_int, C.c_void_p]),       # d_mask: device address
    "rrv_transfer_from_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, ImageDesc, C.c_int]),
    "rrv_transfer_blend_from_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int,
                                              C.c_void_p, ImageDesc, C.c_int]),
    "rrv_transfer_mask_from_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int,
                                             C.c_void_p, ImageDesc, C.c_int]),
    "rrv_add_from_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rrv_add_from_yuv_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_set_yuv_depth": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rrv_yuv_matrix_depth": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rrv_yuv_input_matrix_depth": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rrv_set_yuv16_matrix": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rrv_set_yuv16_input_matrix": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rrv_prepare_style_image_device": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_add_image_device": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_void_p]),
    "rrv_image_view_contiguous": (C.c_int, [ImageDesc, C.c_int, C.c_int, C.POINTER(ImageView)]),
    "rrv_image_view_check": (C.c_int, [C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int]),
    # strided views: (h, in, ImageView* in, B, H, W, [weights, n_styles | mask, n_styles, mask_images,] out, ImageView* out, flags, hip_stream)
    "rrv_transfer_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(ImageView),
                                           C.c_int, C.c_void_p]),
    "rrv_transfer_view_blend_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_void_p]),      # style_weight: host or device address
    "rrv_transfer_view_mask_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_void_p]),       # d_mask: device address
    "rrv_add_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_void_p]),
    # scaling: (h, in, ImageView* in, [B,] SH, SW, H, W, ...): the source frames are SH x SW, H x W is the working size
    "rrv_resample_taps": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]),
    "rrv_resample_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rrv_transfer_scaled_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.POINTER(ImageView), C.c_int, C.c_void_p]),
    "rrv_transfer_scaled": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, ImageDesc, C.c_int]),
    "rrv_add_scaled_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_add_scaled": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_int]),
    # output size: (..., H, W, DH, DW, out, ImageView* / ImageDesc out, ...): the working frame is resampled to DH x DW on its way out
    "rrv_deliver_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(ImageView), C.c_void_p]),
    "rrv_transfer_deliver_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_void_p]),
    "rrv_transfer_deliver": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, ImageDesc,
                                       C.c_int]),
    # guided delivery: (..., H, W, DH, DW, r, eps, out, ...): the working frame reaches DH x DW along the edges of the source's luma
    "rrv_deliver_guided_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_float, C.c_void_p, C.POINTER(ImageView), C.c_void_p]),
    "rrv_transfer_guided_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_float, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_void_p]),
    "rrv_transfer_guided": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_void_p, ImageDesc, C.c_int]),
    "rrv_guided_tile": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 5),      # no handle: (H, W, DH, DW, r, tw, sy, sx, apply LDS, coeff LDS)
    # compositing: (..., DH, DW[, r, eps], Composite* c, out, ...): the delivered frame mixed with its source by strength, matte and keep (r = 0: bilinear delivery)
    "rrv_composite_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Composite), C.c_void_p, C.POINTER(ImageView),
                                            C.c_void_p]),
    "rrv_transfer_composite_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_float, C.POINTER(Composite), C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_void_p]),
    "rrv_transfer_composite": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.POINTER(Composite), C.c_void_p, ImageDesc, C.c_int]),
    "rrv_composite_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_int)]),      # no handle: (B, DH, DW, grid, pixels per pass)
    # JPEG output: tables, bound and plan need no handle; (h, in, B, H, W, Jpeg* p, out[, cap, sizes], hip_stream)
    "rrv_jpeg_tables": (C.c_int, [C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]),
    "rrv_jpeg_bound": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "rrv_jpeg_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 5),      # (H, W, chroma, restart, MCU columns, MCU rows, interval, blocks, header bytes)
    "rrv_jpeg_blocks_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Jpeg), C.c_void_p, C.c_void_p]),
    "rrv_jpeg_entropy_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Jpeg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rrv_jpeg_encode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Jpeg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    # (h, in, ImageView* / ImageDesc in, B, SH, SW, H, W, DH, DW, r, eps, Composite* c, Jpeg* p, out, cap, sizes, flags[, hip_stream])
    "rrv_transfer_jpeg_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_float, C.POINTER(Composite), C.POINTER(Jpeg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "rrv_transfer_jpeg": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.POINTER(Composite), C.POINTER(Jpeg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    # JPEG input: the parser needs no handle; (h, streams, cap, JpegInfo* infos, B, coef / planes, status, hip_stream)
    "rrv_jpeg_parse": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(JpegInfo), C.c_char_p, C.c_size_t]),
    "rrv_jpeg_status_words": (C.c_char_p, [C.c_int]),
    "rrv_jpeg_scan_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(JpegInfo), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rrv_jpeg_planes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(JpegInfo), C.c_int, C.c_void_p, C.c_void_p]),
    "rrv_jpeg_decode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(JpegInfo), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # JPEG as the input form: (h, streams, cap, infos, B, work H, W, DH, DW, r, eps, Composite* c, [Jpeg* p,] out, view | cap, sizes, status, flags, hip_stream)
    "rrv_transfer_from_jpeg_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(JpegInfo), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_float, C.POINTER(Composite), C.c_void_p, C.POINTER(ImageView), C.c_void_p, C.c_int, C.c_void_p]),
    "rrv_transfer_jpeg_from_jpeg_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(JpegInfo), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                          C.c_float, C.POINTER(Composite), C.POINTER(Jpeg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                                          C.c_void_p]),
    # the host twins: (h, char** streams, size_t* sizes, B, work H, W, DH, DW, r, eps, Composite* c, [Jpeg* p,] out, desc | cap, sizes, flags)
    "rrv_transfer_from_jpeg": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.POINTER(Composite), C.c_void_p, ImageDesc, C.c_int]),
    "rrv_add_from_jpeg": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int]),
    "rrv_transfer_jpeg_from_jpeg": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                              C.POINTER(Composite), C.POINTER(Jpeg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    # shots: the plan needs no handle; (h, frames, [view | desc,] B, [SH, SW | H, W,] sig[, hip_stream]); sig: uint32 [B][16][32]
    "rrv_shot_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rrv_shot_signature_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rrv_shot_signature_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rrv_shot_signature": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rrv_shot_signature_from_jpeg": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_void_p]),
    # picture area: the check and the view need no handle; (h, frames, [view | desc,] B, SH, SW, threshold, prof[, hip_stream]); prof: uint32 [B][SH + SW]
    "rrv_picture_check": (C.c_int, [C.c_int, C.c_int, C.POINTER(Picture)]),
    "rrv_picture_view": (C.c_int, [C.POINTER(ImageView), C.c_int, C.c_int, C.POINTER(Picture), C.POINTER(ImageView)]),
    "rrv_picture_profile_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rrv_picture_profile_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rrv_scan_frames": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rrv_add_picture_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.POINTER(Picture), C.c_int, C.c_int, C.c_void_p]),
    "rrv_add_picture": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.POINTER(Picture), C.c_int, C.c_int]),
    "rrv_transfer_picture_view_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_int, C.c_int, C.POINTER(Picture), C.c_int, C.c_int,
                                                   C.c_int, C.c_float, C.POINTER(Composite), C.c_void_p, C.POINTER(ImageView), C.c_int, C.c_void_p]),
    "rrv_transfer_picture": (C.c_int, [C.c_void_p, C.c_void_p, ImageDesc, C.c_int, C.c_int, C.c_int, C.POINTER(Picture), C.c_int, C.c_int, C.c_int, C.c_float,
                                       C.POINTER(Composite), C.c_void_p, ImageDesc, C.c_int]),
    "rrv_get_preclamp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "rrv_get_preclamp_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rrv_sync": (C.c_int, [C.c_void_p]),
    "rrv_set_pipeline": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_set_host_io": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_debug_copy_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rrv_debug_copy_tensor_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rrv_debug_copy_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rrv_debug_prep_stop": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_debug_copy_prep_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rrv_debug_weight_count": (C.c_int, [C.c_void_p]),
    "rrv_debug_weight_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "rrv_debug_copy_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rrv_set_grid_share": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_set_caller_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rrv_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "rrv_host_free": (C.c_int, [C.c_void_p]),
    "rrv_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rrv_host_unregister": (C.c_int, [C.c_void_p]),
    "rrv_set_debug": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_debug_selftest": (C.c_int, [C.c_void_p]),
    "rrv_debug_fail_alloc": (C.c_int, [C.c_void_p, C.c_int]),
    "rrv_profile_begin": (C.c_int, [C.c_void_p]),
    "rrv_profile_end": (C.c_int, [C.c_void_p]),
    "rrv_profile_count": (C.c_int, [C.c_void_p]),
    "rrv_profile_entry": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rrv_profile_entry_grid": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_int)]),
}

# the entries that write a stylized frame; each has a _u8 twin with the same arguments and a uint8 output (its float
# twin's output rounded half to even on the GPU)
U8_TWINS = ("rrv_transfer", "rrv_transfer_async", "rrv_transfer_batch", "rrv_transfer_frames", "rrv_transfer_device",
            "rrv_transfer_batch_device", "rrv_transfer_frames_device", "rrv_transfer_blend", "rrv_transfer_blend_device",
            "rrv_transfer_features", "rrv_transfer_features_batch", "rrv_transfer_frame_mode", "rrv_transfer_frame_mode_batch",
            "rrv_transfer_frame_mode_batch_device", "rrv_transfer_frame_mode_frames", "rrv_transfer_frame_mode_frames_device",
            "rrv_transfer_blend_batch", "rrv_transfer_mask_batch")
SYMBOLS.update({name + "_u8": SYMBOLS[name] for name in U8_TWINS})


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (SONAME libamdhip64.so.7, NEEDED by torch as "libamdhip64.so"); if our library pulled
    /opt/rocm's copy in first, a later `import torch` would load a SECOND runtime that sees
    no GPU.  Pre-loading torch's copy (when torch is installed) makes both bind to it,
    whatever the import order.  RRV_SYSTEM_HIP=1 skips this."""
    if os.environ.get("RRV_SYSTEM_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.submodule_search_locations:
            libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
            cand = os.path.join(libdir, "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            # rrv_broadcast_state dlopens RCCL lazily: point it at the copy built against the same HIP runtime
            rccl = os.path.join(libdir, "librccl.so")
            if os.path.exists(rccl):
                os.environ.setdefault("RRV_RCCL_PATH", rccl)
    except Exception:
        pass


def load():
    """Load the HIP library (once).  Raises OSError with a build hint when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s not found: build it with `python __graft_entry__.py build` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    _share_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)     # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib

"""ctypes binding of libzignal_hip.so — the C ABI declared in include/zignal_hip.h.

There is no CPU fallback anywhere in this package: if the HIP library is missing or an entry point
fails, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZIGNAL_HIP_LIBRARY") or os.path.join(_HERE, "libzignal_hip.so")  # the override is for A/B runs of two builds

# enums (ordinals as in include/zignal_hip.h == the reference's declaration order)
PIXEL_U8, PIXEL_F32, PIXEL_RGB_U8, PIXEL_RGBA_U8, PIXEL_RGB_F32, PIXEL_RGBA_F32 = range(6)
BORDER_ZERO, BORDER_REPLICATE, BORDER_MIRROR, BORDER_WRAP = range(4)
INTERP_NEAREST, INTERP_BILINEAR, INTERP_BICUBIC, INTERP_CATMULL_ROM, INTERP_MITCHELL, INTERP_LANCZOS = range(6)
TRANSFORM_SIMILARITY, TRANSFORM_AFFINE, TRANSFORM_PROJECTIVE = range(3)
CS_GRAY, CS_RGB, CS_RGBA, CS_OKLAB, CS_XYZ, CS_YCBCR, CS_HSL, CS_HSV, CS_LAB, CS_LCH, CS_LMS, CS_OKLCH, CS_XYB = range(13)

OK, ERR_DIMENSION_MISMATCH, ERR_INVALID_ARGUMENT, ERR_OUT_OF_MEMORY, ERR_HIP, ERR_UNSUPPORTED, ERR_CODEC = range(7)


class ZgImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_size_t), ("rows", C.c_uint32),
                ("cols", C.c_uint32), ("pixel", C.c_int32)]


class ZgMethod(C.Structure):
    _fields_ = [("kind", C.c_int32), ("b", C.c_float), ("c", C.c_float), ("lanczos_lut", C.c_void_p)]


class ZgStep(C.Structure):
    """zg_step: one step of zg_batch_pipeline (the CLI's `pipeline` recipe steps, src/cli/pipeline.zig:20-24, plus convert and warp)."""
    _fields_ = [("kind", C.c_int), ("sigma", C.c_float), ("radius", C.c_uint32), ("out_rows", C.c_uint32), ("out_cols", C.c_uint32),
                ("method", ZgMethod), ("dst_pixel", C.c_int), ("dst_space", C.c_int), ("srgb_lut", C.c_void_p), ("transform", C.c_int),
                ("m", C.c_float * 9), ("motion", C.c_int), ("angle", C.c_float), ("cos_a", C.c_float), ("sin_a", C.c_float), ("distance", C.c_uint32),
                ("center_x", C.c_float), ("center_y", C.c_float), ("strength", C.c_float), ("edges", C.c_int), ("low", C.c_float), ("high", C.c_float),
                ("window", C.c_uint32), ("use_nms", C.c_int)]


STEP_GAUSSIAN_BLUR, STEP_BOX_BLUR, STEP_RESIZE, STEP_CONVERT, STEP_WARP, STEP_MEDIAN_BLUR, STEP_MOTION_BLUR, STEP_EDGES = range(8)
MOTION_LINEAR, MOTION_RADIAL_ZOOM, MOTION_RADIAL_SPIN = range(3)
EDGES_SOBEL, EDGES_CANNY, EDGES_SHEN_CASTAN = range(3)


class ZgPngHeader(C.Structure):
    """zg_png_header == png.Header (png.zig:135-149)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_uint8), ("color_type", C.c_uint8),
                ("compression_method", C.c_uint8), ("filter_method", C.c_uint8), ("interlace_method", C.c_uint8),
                ("has_gamma", C.c_uint8), ("has_srgb", C.c_uint8), ("srgb_intent", C.c_uint8), ("gamma", C.c_float)]


class ZgPngLimits(C.Structure):
    """zg_png_limits == png.DecodeLimits (png.zig:23-41)."""
    _fields_ = [("max_png_bytes", C.c_size_t), ("max_chunk_bytes", C.c_size_t), ("max_idat_bytes", C.c_size_t),
                ("max_chunks", C.c_size_t), ("max_width", C.c_uint32), ("max_height", C.c_uint32),
                ("max_pixels", C.c_uint64), ("max_decompressed_bytes", C.c_size_t)]


class ZgPngEncodeOptions(C.Structure):
    """zg_png_encode_options == png.EncodeOptions (png.zig:1296-1316)."""
    _fields_ = [("filter", C.c_int), ("compression_level", C.c_int), ("has_gamma", C.c_int), ("gamma", C.c_float),
                ("srgb_intent", C.c_int)]


class ZgJpegHeader(C.Structure):
    """zg_jpeg_header == jpeg.Header (jpeg.zig:61-74)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("precision", C.c_uint8), ("num_components", C.c_uint8),
                ("progressive", C.c_uint8), ("subsampling", C.c_int8)]


class ZgJpegLimits(C.Structure):
    """zg_jpeg_limits == jpeg.DecodeLimits (jpeg.zig:19-33)."""
    _fields_ = [("max_jpeg_bytes", C.c_size_t), ("max_marker_bytes", C.c_size_t), ("max_width", C.c_uint32), ("max_height", C.c_uint32),
                ("max_pixels", C.c_uint64), ("max_blocks", C.c_size_t), ("max_scans", C.c_size_t)]


class ZgJpegEncodeOptions(C.Structure):
    """zg_jpeg_encode_options == jpeg.EncodeOptions (jpeg.zig:284-290)."""
    _fields_ = [("quality", C.c_int), ("subsampling", C.c_int), ("density_dpi", C.c_int), ("comment", C.c_char_p), ("comment_len", C.c_size_t)]


class ZgKeypoint(C.Structure):
    """zg_keypoint == KeyPoint (src/features/KeyPoint.zig:9-28)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float), ("response", C.c_float),
                ("octave", C.c_int32), ("class_id", C.c_int32)]


class ZgBinaryDescriptor(C.Structure):
    """zg_binary_descriptor == BinaryDescriptor (src/features/BinaryDescriptor.zig:10)."""
    _fields_ = [("bits", C.c_uint8 * 32)]


class ZgOrbParams(C.Structure):
    """zg_orb_params == Orb's fields (src/features/orb.zig:87-109) and the optional orientation weight table."""
    _fields_ = [("n_features", C.c_uint32), ("scale_factor", C.c_float), ("n_levels", C.c_uint32), ("edge_threshold", C.c_uint32),
                ("first_level", C.c_uint32), ("wta_k", C.c_uint32), ("fast_threshold", C.c_uint32), ("score_type", C.c_int32),
                ("orientation_weights", C.c_void_p)]


ORB_HARRIS_SCORE, ORB_FAST_SCORE = range(2)


class ZgMatch(C.Structure):
    """zg_match == Match (src/features/matcher.zig:10-19) with 32-bit indices."""
    _fields_ = [("query_idx", C.c_uint32), ("train_idx", C.c_uint32), ("distance", C.c_float)]


class ZgDescriptorSet(C.Structure):
    """zg_descriptor_set: a descriptor array, its capacity and the optional word that holds how many of them count."""
    _fields_ = [("data", C.c_void_p), ("capacity", C.c_uint32), ("count", C.c_void_p)]


class ZgMatcherParams(C.Structure):
    """zg_matcher_params == BruteForceMatcher's fields (matcher.zig:33-41)."""
    _fields_ = [("cross_check", C.c_int32), ("max_distance", C.c_uint32), ("ratio_threshold", C.c_float)]


class ZgMatchStatistics(C.Structure):
    """zg_match_statistics == MatchStats (matcher.zig:237-241)."""
    _fields_ = [("total_matches", C.c_size_t), ("mean_distance", C.c_float), ("min_distance", C.c_float), ("max_distance", C.c_float)]


class ZgHoughLine(C.Structure):
    """zg_hough_line == HoughTransform.Line (src/image/hough.zig:13-25), field for field."""
    _fields_ = [("angle", C.c_float), ("radius", C.c_float), ("score", C.c_uint32), ("p1", C.c_float * 2), ("p2", C.c_float * 2)]


class ZgFloodFillOptions(C.Structure):
    """zg_flood_fill_options == FloodFillOptions (src/image/flood_fill.zig:5-26): connectivity 4 | 8, mode 0 seed | 1 neighbor."""
    _fields_ = [("threshold", C.c_double), ("connectivity", C.c_int), ("mode", C.c_int)]


FLOOD_MODE_SEED, FLOOD_MODE_NEIGHBOR = range(2)


class ZgDrawCmd(C.Structure):
    """zg_draw_cmd: one call of the reference's Canvas(T) (include/zignal_hip_canvas.h). 40 bytes."""
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("width", C.c_uint32), ("color", C.c_uint8 * 4), ("p", C.c_float * 4),
                ("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32)]


DRAW_LINE, DRAW_RECT, DRAW_FILL_RECT, DRAW_CIRCLE, DRAW_FILL_CIRCLE, DRAW_POLYGON, DRAW_FILL_POLYGON = range(7)
DRAW_ARC, DRAW_FILL_ARC = 16, 17  # zg_canvas_draw_arcs and the host form only; 7-15 are no kinds
DRAW_QUAD_BEZIER, DRAW_CUBIC_BEZIER, DRAW_SPLINE_POLYGON, DRAW_FILL_SPLINE_POLYGON = range(18, 22)
DRAW_FAST, DRAW_SOFT = range(2)
CANVAS_MAX_VERTICES, CANVAS_MAX_COORD, CANVAS_MAX_WIDTH, CANVAS_MAX_SIZE, CANVAS_MAX_COMMANDS = 64, 65536.0, 65536, 32768, 1 << 24  # ZG_CANVAS_MAX_*
CANVAS_MAX_CURVE_POINTS = 512


class ZgGlyph(C.Structure):
    """zg_glyph: one entry of a variable-width font's glyph table (include/zignal_hip_text.h). 16 bytes."""
    _fields_ = [("codepoint", C.c_uint32), ("bitmap_offset", C.c_uint32), ("width", C.c_uint8), ("height", C.c_uint8), ("x_offset", C.c_int16),
                ("y_offset", C.c_int16), ("device_width", C.c_int16)]


class ZgFont(C.Structure):
    """zg_font: a BitmapFont by value; data and glyphs are host or device addresses, as the call takes them. 32 bytes."""
    _fields_ = [("data", C.c_void_p), ("glyphs", C.c_void_p), ("data_len", C.c_uint32), ("n_glyphs", C.c_uint32), ("char_width", C.c_uint8),
                ("char_height", C.c_uint8), ("first_char", C.c_uint8), ("last_char", C.c_uint8), ("reserved", C.c_uint32)]


class ZgTextCmd(C.Structure):
    """zg_text_cmd: one drawText call. 28 bytes."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("scale", C.c_float), ("mode", C.c_int32), ("color", C.c_uint8 * 4),
                ("first_codepoint", C.c_uint32), ("n_codepoints", C.c_uint32)]


TEXT_MAX_SCALE, TEXT_MAX_CODEPOINTS, TEXT_MAX_COMMANDS, TEXT_MAX_TOTAL = 64.0, 65536, 65536, 1 << 24  # ZG_TEXT_MAX_*


class ZgMetricResult(C.Structure):
    """zg_metric_result: the left-to-right f64 sum, the number of terms, the metric's value and how many terms were added serially."""
    _fields_ = [("sum", C.c_double), ("count", C.c_uint64), ("value", C.c_double), ("serial_terms", C.c_uint64)]


class ZgMetricOptions(C.Structure):
    """zg_metric_options: the caller's 121 SSIM weights (host memory) and the SSIM map to fill, both optional."""
    _fields_ = [("ssim_window", C.c_void_p), ("ssim_map", C.c_void_p)]


class ZgFdmMoments(C.Structure):
    """zg_fdm_moments: the exact integer moments of one frame (include/zignal_hip_fdm.h). 104 bytes."""
    _fields_ = [("n", C.c_uint64), ("sum", C.c_uint64 * 3), ("prod", C.c_uint64 * 6), ("lum_sum", C.c_uint64), ("lum_sq", C.c_uint64),
                ("not_gray", C.c_uint32), ("pixel", C.c_int32)]


class ZgFdmTarget(C.Structure):
    """zg_fdm_target: what setTarget keeps (fdm.zig:29-32). 136 bytes."""
    _fields_ = [("mean", C.c_double * 3), ("u", C.c_double * 9), ("s", C.c_double * 3), ("is_gray", C.c_int32), ("status", C.c_int32),
                ("pixel", C.c_int32), ("reserved", C.c_int32)]


class ZgFdmTransform(C.Structure):
    """zg_fdm_transform: what update applies to every pixel. 120 bytes."""
    _fields_ = [("route", C.c_int32), ("status", C.c_int32), ("w", C.c_double * 9), ("bias", C.c_double * 3), ("scale", C.c_double),
                ("offset", C.c_double)]


FDM_ROUTE_COLOR, FDM_ROUTE_SCALAR, FDM_ROUTE_GRAY_TARGET = range(3)
FDM_STATUS_TYPE_MISMATCH = -1


class ZgTransformFit(C.Structure):
    """zg_transform_fit: the result of a fit (include/zignal_hip_transform.h). 128 bytes."""
    _fields_ = [("kind", C.c_int32), ("status", C.c_int32), ("n_points", C.c_uint32), ("svd_converged", C.c_uint32), ("m64", C.c_double * 9),
                ("m32", C.c_float * 9), ("reserved", C.c_uint32)]


SCALAR_F32, SCALAR_F64 = range(2)
FIT_OK, FIT_NOT_CONVERGED, FIT_RANK_DEFICIENT, FIT_BAD_COUNT, FIT_BAD_INPUT = range(5)
FIT_MAX_POINTS, FIT_MAX_POINTS_AFFINE = 65536, 4096  # ZG_FIT_MAX_*


class ZignalError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"zignal_hip status {status}: {message}")
        self.status = status


class DimensionMismatch(ZignalError):
    """error.DimensionMismatch (reference src/image.zig:636,927,947,962)."""


class InvalidArgument(ZignalError, ValueError):
    """error.InvalidSigma / InvalidScaleFactor / InvalidDimensions."""


class CodecError(ZignalError):
    """An error of a codec's error set (src/codecs/png.zig); `.name` is the Zig error name, e.g. "InvalidCrc"."""

    def __init__(self, status: int, message: str):
        super().__init__(status, message)
        self.name = message.split(" ", 1)[0]


_lib = None

_IMG = C.POINTER(ZgImage)
_METHOD = C.POINTER(ZgMethod)
_F32P = C.POINTER(C.c_float)
_U32P = C.POINTER(C.c_uint32)

# name -> argtypes (restype is int unless listed in _RESTYPES)
_SIGNATURES = {
    "zg_init": [C.c_int],
    "zg_shutdown": [],
    "zg_last_error": [],
    "zg_version": [],
    "zg_device_count": [],
    "zg_malloc": [C.POINTER(C.c_void_p), C.c_size_t],
    "zg_free": [C.c_void_p],
    "zg_memcpy_h2d": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "zg_memcpy_d2h": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "zg_set_device": [C.c_int],
    "zg_get_device": [C.POINTER(C.c_int)],
    "zg_malloc_host": [C.POINTER(C.c_void_p), C.c_size_t],
    "zg_free_host": [C.c_void_p],
    "zg_memcpy_h2d_async": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "zg_memcpy_d2h_async": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "zg_image_upload": [_IMG, _IMG, C.c_void_p],
    "zg_image_download": [_IMG, _IMG, C.c_void_p],
    "zg_stream_wait_event": [C.c_void_p, C.c_void_p],
    "zg_event_create": [C.POINTER(C.c_void_p)],
    "zg_event_destroy": [C.c_void_p],
    "zg_event_record": [C.c_void_p, C.c_void_p],
    "zg_event_synchronize": [C.c_void_p],
    "zg_event_elapsed_ms": [C.c_void_p, C.c_void_p, _F32P],
    "zg_graph_begin_capture": [C.c_void_p],
    "zg_graph_end_capture": [C.c_void_p, C.POINTER(C.c_void_p)],
    "zg_graph_launch": [C.c_void_p, C.c_void_p],
    "zg_graph_destroy": [C.c_void_p],
    "zg_release_graph_scratch": [],
    "zg_trim_scratch": [],
    "zg_devmath_apply": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "zg_lanczos_plane_weights": [C.c_uint32, C.c_uint32, _F32P],
    "zg_resize_lanczos_weights": [_IMG, _IMG, _F32P, _F32P, C.c_void_p],
    "zg_resize_lanczos_weights_host": [_IMG, _IMG, _F32P, _F32P],
    "zg_resize_convert": [_IMG, C.c_int, _IMG, C.c_int, _METHOD, _F32P, C.c_void_p],
    "zg_resize_convert_host": [_IMG, C.c_int, _IMG, C.c_int, _METHOD, _F32P],
    "zg_batch_pipeline_shape": [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(ZgStep), C.c_uint32, _U32P, _U32P, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "zg_batch_pipeline": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(ZgStep), C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_pyramid_build": [_IMG, _IMG, _F32P, C.c_uint32, C.c_void_p],
    "zg_multi_create": [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)],
    "zg_multi_destroy": [C.c_void_p],
    "zg_multi_device_count": [C.c_void_p],
    "zg_multi_wait_stream": [C.c_void_p, C.c_void_p],
    "zg_multi_batch_blur_resize": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_void_p, C.c_uint32, C.c_uint32, _METHOD, _F32P],
    "zg_multi_batch_pipeline": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(ZgStep), C.c_uint32, C.c_void_p, _F32P],
    "zg_multi_piece_range": [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, _U32P, _U32P],
    "zg_sizeof_step": [],
    "zg_stream_create": [C.POINTER(C.c_void_p)],
    "zg_stream_destroy": [C.c_void_p],
    "zg_stream_synchronize": [C.c_void_p],
    "zg_pixel_size": [C.c_int],
    "zg_conv_separable": [_IMG, _IMG, _F32P, C.c_uint32, _F32P, C.c_uint32, C.c_int, C.c_void_p],
    "zg_conv_separable_host": [_IMG, _IMG, _F32P, C.c_uint32, _F32P, C.c_uint32, C.c_int],
    "zg_gaussian_blur": [_IMG, _IMG, C.c_float, C.c_void_p],
    "zg_gaussian_blur_host": [_IMG, _IMG, C.c_float],
    "zg_gaussian_kernel": [C.c_float, _F32P, C.c_uint32],
    "zg_conv_separable_planes": [_IMG, _IMG, C.c_uint32, _F32P, C.c_uint32, _F32P, C.c_uint32, C.c_int, C.c_void_p],
    "zg_gaussian_blur_planes": [_IMG, _IMG, C.c_uint32, C.c_float, C.c_void_p],
    "zg_convolve": [_IMG, _IMG, _F32P, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p],
    "zg_convolve_host": [_IMG, _IMG, _F32P, C.c_uint32, C.c_uint32, C.c_int],
    "zg_box_blur": [_IMG, _IMG, C.c_uint32, C.c_void_p],
    "zg_box_blur_host": [_IMG, _IMG, C.c_uint32],
    "zg_resize": [_IMG, _IMG, _METHOD, C.c_void_p],
    "zg_resize_host": [_IMG, _IMG, _METHOD],
    "zg_letterbox": [_IMG, _IMG, _METHOD, _U32P, C.c_void_p],
    "zg_letterbox_host": [_IMG, _IMG, _METHOD, _U32P],
    "zg_warp": [_IMG, _IMG, C.c_int, _F32P, _METHOD, C.c_void_p],
    "zg_warp_host": [_IMG, _IMG, C.c_int, _F32P, _METHOD],
    "zg_rotate_into": [_IMG, _IMG, C.c_float, C.c_float, C.c_float, _METHOD, C.c_int, C.c_void_p],
    "zg_rotate_into_host": [_IMG, _IMG, C.c_float, C.c_float, C.c_float, _METHOD, C.c_int],
    "zg_rotate_bounds": [C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, _U32P, _U32P],
    "zg_extract": [_IMG, _IMG, _F32P, C.c_float, C.c_float, C.c_float, _METHOD, C.c_int, C.c_void_p],
    "zg_extract_host": [_IMG, _IMG, _F32P, C.c_float, C.c_float, C.c_float, _METHOD, C.c_int],
    "zg_crop": [_IMG, _IMG, _F32P, C.c_void_p],
    "zg_crop_host": [_IMG, _IMG, _F32P],
    "zg_crop_dims": [_F32P, _U32P, _U32P],
    "zg_flip_left_right": [_IMG, C.c_void_p],
    "zg_flip_top_bottom": [_IMG, C.c_void_p],
    "zg_flip_left_right_host": [_IMG],
    "zg_flip_top_bottom_host": [_IMG],
    "zg_insert": [_IMG, _IMG, _F32P, C.c_float, C.c_float, C.c_float, _METHOD, C.c_int, C.c_void_p],
    "zg_insert_host": [_IMG, _IMG, _F32P, C.c_float, C.c_float, C.c_float, _METHOD, C.c_int],
    "zg_copy": [_IMG, _IMG, C.c_void_p],
    "zg_fill": [_IMG, C.c_void_p, C.c_void_p],
    "zg_set_border": [_IMG, _U32P, C.c_void_p, C.c_void_p],
    "zg_fill_host": [_IMG, C.c_void_p],
    "zg_set_border_host": [_IMG, _U32P, C.c_void_p],
    "zg_convert": [_IMG, C.c_int, _IMG, C.c_int, _F32P, C.c_void_p],
    "zg_convert_host": [_IMG, C.c_int, _IMG, C.c_int, _F32P],
    "zg_sharpen": [_IMG, _IMG, C.c_uint32, C.c_void_p],
    "zg_sharpen_host": [_IMG, _IMG, C.c_uint32],
    "zg_integral": [_IMG, _F32P, C.c_void_p],
    "zg_integral_host": [_IMG, _F32P],
    "zg_invert": [_IMG, C.c_void_p],
    "zg_invert_host": [_IMG],
    "zg_order_statistic_blur": [_IMG, _IMG, C.c_uint32, C.c_int, C.c_double, C.c_int, C.c_void_p],
    "zg_order_statistic_blur_host": [_IMG, _IMG, C.c_uint32, C.c_int, C.c_double, C.c_int],
    "zg_autocontrast": [_IMG, C.c_float, C.c_void_p],
    "zg_autocontrast_host": [_IMG, C.c_float],
    "zg_equalize": [_IMG, C.c_void_p],
    "zg_equalize_host": [_IMG],
    "zg_threshold_otsu": [_IMG, _IMG, C.POINTER(C.c_uint8), C.c_void_p],
    "zg_threshold_otsu_host": [_IMG, _IMG, C.POINTER(C.c_uint8)],
    "zg_threshold_adaptive_mean": [_IMG, _IMG, C.c_uint32, C.c_float, C.c_void_p],
    "zg_threshold_adaptive_mean_host": [_IMG, _IMG, C.c_uint32, C.c_float],
    "zg_morph": [_IMG, _IMG, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p],
    "zg_morph_host": [_IMG, _IMG, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int],
    "zg_sobel": [_IMG, _IMG, C.c_void_p],
    "zg_sobel_host": [_IMG, _IMG],
    "zg_canny": [_IMG, _IMG, C.c_float, C.c_float, C.c_float, C.c_void_p],
    "zg_canny_host": [_IMG, _IMG, C.c_float, C.c_float, C.c_float],
    "zg_isef_smooth": [_IMG, _IMG, C.c_float, C.c_void_p],
    "zg_fast_detect": [_IMG, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_fast_detect_host": [_IMG, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, _U32P],
    "zg_fast_detect_batch": [_IMG, C.c_uint32, _U32P, C.c_uint32, C.c_int, C.c_void_p, _U32P, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p],
    "zg_shen_castan": [_IMG, _IMG, C.c_float, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p],
    "zg_shen_castan_host": [_IMG, _IMG, C.c_float, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_int],
    "zg_motion_blur_linear": [_IMG, _IMG, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_void_p],
    "zg_motion_blur_linear_host": [_IMG, _IMG, C.c_float, C.c_float, C.c_float, C.c_uint32],
    "zg_motion_blur_radial": [_IMG, _IMG, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p],
    "zg_motion_blur_radial_host": [_IMG, _IMG, C.c_float, C.c_float, C.c_float, C.c_int],
    "zg_pyramid_scale": [C.c_float, C.c_uint32],
    "zg_pyramid_build_level": [_IMG, _IMG, C.c_float, C.c_void_p],
    "zg_pyramid_level": [C.c_uint32, C.c_uint32, C.c_float, C.c_float, _U32P, _U32P, _F32P],
    "zg_batch_blur_resize": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float,
                             C.c_void_p, C.c_uint32, C.c_uint32, _METHOD, C.c_void_p],
    "zg_png_default_limits": [C.POINTER(ZgPngLimits)],
    "zg_png_default_encode_options": [C.POINTER(ZgPngEncodeOptions)],
    "zg_png_info": [C.c_void_p, C.c_size_t, C.POINTER(ZgPngLimits), C.POINTER(ZgPngHeader)],
    "zg_png_probe": [C.c_void_p, C.c_size_t, C.POINTER(ZgPngLimits), C.POINTER(ZgPngHeader), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "zg_png_scan_hash": [C.c_void_p, C.c_size_t, C.POINTER(ZgPngLimits), C.POINTER(C.c_uint64), C.POINTER(C.c_int)],
    "zg_png_decode": [C.c_void_p, C.c_size_t, C.POINTER(ZgPngLimits), _IMG, C.c_int, C.POINTER(C.c_int), C.c_void_p],
    "zg_png_decode_host": [C.c_void_p, C.c_size_t, C.POINTER(ZgPngLimits), _IMG, C.c_int, C.POINTER(C.c_int)],
    "zg_png_filter": [_IMG, C.c_int, C.c_void_p, C.c_void_p],
    "zg_png_encode": [_IMG, C.c_int, C.POINTER(ZgPngEncodeOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p],
    "zg_png_encode_host": [_IMG, C.c_int, C.POINTER(ZgPngEncodeOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "zg_png_compress": [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "zg_png_free": [C.c_void_p],
    "zg_jpeg_default_limits": [C.POINTER(ZgJpegLimits)],
    "zg_jpeg_info": [C.c_void_p, C.c_size_t, C.POINTER(ZgJpegLimits), C.POINTER(ZgJpegHeader)],
    "zg_jpeg_probe": [C.c_void_p, C.c_size_t, C.POINTER(ZgJpegLimits), C.POINTER(ZgJpegHeader), C.POINTER(C.c_int)],
    "zg_jpeg_coefficient_hash": [C.c_void_p, C.c_size_t, C.POINTER(ZgJpegLimits), C.POINTER(C.c_uint64)],
    "zg_jpeg_decode": [C.c_void_p, C.c_size_t, C.POINTER(ZgJpegLimits), _IMG, C.c_int, C.POINTER(C.c_int), C.c_void_p],
    "zg_jpeg_decode_host": [C.c_void_p, C.c_size_t, C.POINTER(ZgJpegLimits), _IMG, C.c_int, C.POINTER(C.c_int)],
    "zg_jpeg_default_encode_options": [C.POINTER(ZgJpegEncodeOptions)],
    "zg_jpeg_encode": [_IMG, C.c_int, C.POINTER(ZgJpegEncodeOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p],
    "zg_jpeg_encode_host": [_IMG, C.c_int, C.POINTER(ZgJpegEncodeOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "zg_jpeg_encode_blocks": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(ZgJpegEncodeOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "zg_jpeg_free": [C.c_void_p],
}
_RESTYPES = {"zg_last_error": C.c_char_p, "zg_shutdown": None, "zg_pixel_size": C.c_size_t, "zg_sizeof_step": C.c_size_t, "zg_pyramid_scale": C.c_float,
             "zg_png_default_limits": None, "zg_png_default_encode_options": None, "zg_png_free": None, "zg_jpeg_default_limits": None, "zg_jpeg_default_encode_options": None, "zg_jpeg_free": None}

# every symbol include/zignal_hip.h declares; tests check the library exports all of them
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# the ORB module: every symbol include/zignal_hip_orb.h declares
_ORB_SIGNATURES = {
    "zg_orb_default_params": [C.POINTER(ZgOrbParams)],
    "zg_orb_features_per_level": [C.POINTER(ZgOrbParams), _U32P],
    "zg_orb_adaptive_threshold": [C.POINTER(ZgOrbParams), C.c_uint32],
    "zg_orb_detect_and_compute": [_IMG, C.POINTER(ZgOrbParams), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_orb_compute": [_IMG, C.POINTER(ZgOrbParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_orb_detect_and_compute_host": [_IMG, C.POINTER(ZgOrbParams), C.c_void_p, C.c_void_p, C.c_uint32, _U32P],
    "zg_orb_compute_host": [_IMG, C.POINTER(ZgOrbParams), C.c_void_p, C.c_uint32, C.c_void_p],
}
_ORB_RESTYPES = {"zg_orb_default_params": None}
ORB_EXPORTED_SYMBOLS = tuple(_ORB_SIGNATURES)


# the matcher module: every symbol include/zignal_hip_match.h declares
_SET = C.POINTER(ZgDescriptorSet)
_MATCH_SIGNATURES = {
    "zg_matcher_default_params": [C.POINTER(ZgMatcherParams)],
    "zg_match_train_chunk": [],
    "zg_match_descriptors": [_SET, _SET, C.POINTER(ZgMatcherParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_match_knn": [_SET, _SET, C.POINTER(ZgMatcherParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_match_radius": [_SET, _SET, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_match_descriptors_host": [_SET, _SET, C.POINTER(ZgMatcherParams), C.c_void_p, C.c_uint32, _U32P],
    "zg_match_knn_host": [_SET, _SET, C.POINTER(ZgMatcherParams), C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_match_radius_host": [_SET, _SET, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, _U32P],
    "zg_match_stats": [C.c_void_p, C.c_size_t, C.POINTER(ZgMatchStatistics)],
}
_MATCH_RESTYPES = {"zg_matcher_default_params": None, "zg_match_train_chunk": C.c_uint32}
MATCH_EXPORTED_SYMBOLS = tuple(_MATCH_SIGNATURES)


# the Hough module: every symbol include/zignal_hip_hough.h declares
_I32P = C.POINTER(C.c_int32)
_HOUGH_SIGNATURES = {
    "zg_hough_lds_max_size": [],
    "zg_hough_pixel_chunk": [],
    "zg_hough_tables_host": [C.c_uint32, _I32P, _I32P],
    "zg_hough_create": [C.c_uint32, C.POINTER(C.c_void_p)],
    "zg_hough_create_with_tables": [C.c_uint32, _I32P, _I32P, C.POINTER(C.c_void_p)],
    "zg_hough_destroy": [C.c_void_p],
    "zg_hough_size": [C.c_void_p],
    "zg_hough_compute": [C.c_void_p, _IMG, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p],
    "zg_hough_find_lines": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_uint32,
                            C.c_void_p, C.c_void_p],
    "zg_hough_compute_host": [C.c_void_p, _IMG, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t],
    "zg_hough_find_lines_host": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_uint32, _U32P],
}
_HOUGH_RESTYPES = {"zg_hough_lds_max_size": C.c_uint32, "zg_hough_pixel_chunk": C.c_uint32, "zg_hough_size": C.c_uint32}
HOUGH_EXPORTED_SYMBOLS = tuple(_HOUGH_SIGNATURES)
HOUGH_MAX_SIZE, HOUGH_MAX_CANDIDATES = 32768, 1 << 20  # ZG_HOUGH_MAX_SIZE, ZG_HOUGH_MAX_CANDIDATES

# the flood-fill module: every symbol include/zignal_hip_flood.h declares
_FLOOD_SIGNATURES = {
    "zg_flood_fill_tile": [],
    "zg_flood_fill_bound_host": [C.c_int, C.c_double, C.POINTER(C.c_double)],
    "zg_flood_fill": [_IMG, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(ZgFloodFillOptions), C.c_void_p, C.c_void_p],
    "zg_flood_fill_host": [_IMG, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(ZgFloodFillOptions), _U32P],
}
_FLOOD_RESTYPES = {"zg_flood_fill_tile": C.c_uint32}
FLOOD_EXPORTED_SYMBOLS = tuple(_FLOOD_SIGNATURES)

# the metrics module: every symbol include/zignal_hip_metrics.h declares
_F64P = C.POINTER(C.c_double)
_METRIC_OPT = C.POINTER(ZgMetricOptions)
_METRICS_SIGNATURES = {
    "zg_sum_f64_chunk": [],
    "zg_ssim_window_host": [_F64P],
    "zg_psnr_from_mse": [C.c_double, C.c_double],
    "zg_exp_f64_host": [C.c_double],
    "zg_log10_f64_host": [C.c_double],
    "zg_sum_f64_sequential": [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_psnr": [_IMG, _IMG, _METRIC_OPT, C.c_void_p, C.c_void_p],
    "zg_mean_pixel_error": [_IMG, _IMG, _METRIC_OPT, C.c_void_p, C.c_void_p],
    "zg_ssim": [_IMG, _IMG, _METRIC_OPT, C.c_void_p, C.c_void_p],
    "zg_psnr_host": [_IMG, _IMG, _METRIC_OPT, _F64P, C.POINTER(ZgMetricResult)],
    "zg_mean_pixel_error_host": [_IMG, _IMG, _METRIC_OPT, _F64P, C.POINTER(ZgMetricResult)],
    "zg_ssim_host": [_IMG, _IMG, _METRIC_OPT, _F64P, C.POINTER(ZgMetricResult)],
}
_METRICS_RESTYPES = {"zg_sum_f64_chunk": C.c_uint32, "zg_psnr_from_mse": C.c_double, "zg_exp_f64_host": C.c_double, "zg_log10_f64_host": C.c_double}
METRICS_EXPORTED_SYMBOLS = tuple(_METRICS_SIGNATURES)

# the quantisation module: every symbol include/zignal_hip_quantize.h declares
_U8P = C.POINTER(C.c_uint8)
_QUANTIZE_SIGNATURES = {
    "zg_color_histogram": [_IMG, C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_median_cut_from_histogram_host": [_U32P, _U32P, C.c_uint32, C.c_uint32, _U8P, _U32P],
    "zg_median_cut": [_IMG, C.c_uint32, C.c_uint32, _U8P, _U32P],
    "zg_build_palette": [_IMG, C.c_int, C.c_uint32, _U8P, _U32P],
    "zg_palette_lut": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_palette_lut_host": [_U8P, C.c_uint32, _U8P],
    "zg_dither_geometry": [_U32P, _U32P, _U32P],
    "zg_dither": [_IMG, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p],
    "zg_dither_frames": [_IMG, C.c_uint32, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p],
    "zg_palette_map": [_IMG, _IMG, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p],
}
_QUANTIZE_RESTYPES = {"zg_dither_geometry": None}
QUANTIZE_EXPORTED_SYMBOLS = tuple(_QUANTIZE_SIGNATURES)
HISTOGRAM_CELLS, HISTOGRAM_UNTOUCHED = 32768, 0xFFFFFFFF  # ZG_HISTOGRAM_CELLS, ZG_HISTOGRAM_UNTOUCHED
DITHER_NONE, DITHER_FLOYD_STEINBERG, DITHER_ATKINSON, DITHER_ORDERED, DITHER_AUTO = range(5)
PALETTE_FIXED_6X7X6, PALETTE_FIXED_VGA16, PALETTE_FIXED_WEB216, PALETTE_ADAPTIVE = range(4)

# the Canvas module: every symbol include/zignal_hip_canvas.h declares
_CANVAS_SIGNATURES = {
    "zg_sizeof_draw_cmd": [],
    "zg_canvas_tile": [],
    "zg_canvas_draw": [_IMG, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "zg_canvas_draw_arcs": [_IMG, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "zg_canvas_draw_host": [_IMG, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32],
    "zg_canvas_cmds_from_hough_lines": [C.c_void_p, C.c_void_p, C.c_uint32, _U8P, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_canvas_cmds_from_keypoints": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, _U8P, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
}
_CANVAS_RESTYPES = {"zg_sizeof_draw_cmd": C.c_size_t, "zg_canvas_tile": C.c_uint32}
CANVAS_EXPORTED_SYMBOLS = tuple(_CANVAS_SIGNATURES)

# the text module: every symbol include/zignal_hip_text.h declares
_FONT = C.POINTER(ZgFont)
_TEXT_SIGNATURES = {
    "zg_sizeof_font": [],
    "zg_sizeof_glyph": [],
    "zg_sizeof_text_cmd": [],
    "zg_font_check": [_FONT],
    "zg_font_upload": [_FONT, _FONT],
    "zg_font_free": [_FONT],
    "zg_text_bounds_host": [_FONT, C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_float)],
    "zg_canvas_draw_text": [_IMG, _FONT, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "zg_canvas_draw_text_host": [_IMG, _FONT, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32],
}
_TEXT_RESTYPES = {"zg_sizeof_font": C.c_size_t, "zg_sizeof_glyph": C.c_size_t, "zg_sizeof_text_cmd": C.c_size_t}
TEXT_EXPORTED_SYMBOLS = tuple(_TEXT_SIGNATURES)

# the feature-distribution-matching module: every symbol include/zignal_hip_fdm.h declares
_FDM_M, _FDM_T, _FDM_X = C.POINTER(ZgFdmMoments), C.POINTER(ZgFdmTarget), C.POINTER(ZgFdmTransform)
_FDM_SIGNATURES = {
    "zg_fdm_sizeof_moments": [],
    "zg_fdm_sizeof_target": [],
    "zg_fdm_sizeof_transform": [],
    "zg_fdm_lane_run": [],
    "zg_fdm_frames_per_launch": [],
    "zg_fdm_compute_moments": [_IMG, C.c_void_p, C.c_void_p],
    "zg_fdm_compute_moments_frames": [_IMG, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_fdm_target_from_moments": [C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_fdm_transform_from_moments": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_fdm_transform_from_moments_frames": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_fdm_target_host": [C.c_int, _F64P, _F64P, C.c_int, _FDM_T],
    "zg_fdm_transform_host": [C.c_int, _FDM_T, _F64P, _F64P, _FDM_X],
    "zg_fdm_stats_from_moments_host": [_FDM_M, C.c_int, _F64P, _F64P],
    "zg_fdm_apply": [_IMG, C.c_void_p, C.c_void_p],
    "zg_fdm_apply_frames": [_IMG, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_fdm_match": [_IMG, _IMG, C.c_void_p],
    "zg_fdm_match_frames": [_IMG, C.c_uint32, _IMG, C.c_void_p, C.c_void_p],
    "zg_fdm_match_host": [_IMG, _IMG],
    "zg_fdm_match_frames_host": [_IMG, C.c_uint32, _IMG],
}
_FDM_RESTYPES = {"zg_fdm_sizeof_moments": C.c_size_t, "zg_fdm_sizeof_target": C.c_size_t, "zg_fdm_sizeof_transform": C.c_size_t,
                 "zg_fdm_lane_run": C.c_uint32, "zg_fdm_frames_per_launch": C.c_uint32}
FDM_EXPORTED_SYMBOLS = tuple(_FDM_SIGNATURES)


class ZgTracerOptions(C.Structure):
    """zg_tracer_options == Tracer's two fields (src/features/Tracer.zig:20-25)."""
    _fields_ = [("min_path_length", C.c_uint32), ("simplification_epsilon", C.c_float)]


# the Tracer module: every symbol include/zignal_hip_tracer.h declares
_TRACER_SIGNATURES = {
    "zg_trace_scratch_bytes": [C.c_uint32, C.c_uint32],
    "zg_trace_paths": [_IMG, C.POINTER(ZgTracerOptions), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_trace_paths_host": [_IMG, C.POINTER(ZgTracerOptions), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _U32P],
    "zg_canvas_cmds_from_paths": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, _U8P, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
}
_TRACER_RESTYPES = {"zg_trace_scratch_bytes": C.c_size_t}
TRACER_EXPORTED_SYMBOLS = tuple(_TRACER_SIGNATURES)


class ZgQrFinder(C.Structure):
    """zg_qr_finder == FinderPattern (src/qrcode/detector.zig:170-175)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("module_size", C.c_float), ("hits", C.c_float)]


class ZgQrFourth(C.Structure):
    """zg_qr_fourth == Fourth (detector.zig:410-413)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("is_alignment", C.c_uint32)]


class ZgQrDetection(C.Structure):
    """zg_qr_detection: every intermediate result of detectAndDecode (detector.zig:86-156)."""
    _fields_ = [("finders", ZgQrFinder * 64), ("finder_count", C.c_uint32), ("merged_count", C.c_uint32), ("triple_found", C.c_uint32),
                ("triple", ZgQrFinder * 3), ("version_estimate", C.c_uint32), ("version_count", C.c_uint32), ("versions", C.c_uint8 * 8),
                ("fourth_count", C.c_uint32), ("fourths", ZgQrFourth * 5), ("grids_total", C.c_uint32), ("grids_written", C.c_uint32),
                ("modules_written", C.c_uint32)]


class ZgQrGrid(C.Structure):
    """zg_qr_grid: one trial that passed the timing check and sampleGrid."""
    _fields_ = [("version", C.c_uint32), ("dim", C.c_uint32), ("fourth_index", C.c_uint32), ("modules_offset", C.c_uint32), ("version_hint", C.c_int32),
                ("corners", C.c_float * 8), ("reserved", C.c_uint32), ("transform", C.c_double * 9)]


QR_ADAPTIVE, QR_OTSU, QR_BINARY = 0, 1, 2
QR_MAX_MODULES = 177 * 177

# the QR module: every symbol include/zignal_hip_qr.h declares
_QR_SIGNATURES = {
    "zg_qr_sizeof_detection": [],
    "zg_qr_sizeof_grid": [],
    "zg_qr_scratch_bytes": [C.c_uint32, C.c_uint32],
    "zg_qr_detect": [_IMG, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p],
    "zg_qr_detect_host": [_IMG, C.c_int, C.POINTER(ZgQrDetection), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32],
    "zg_canvas_cmds_from_qr": [C.c_void_p, C.c_void_p, C.c_uint32, _U8P, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
}
_QR_RESTYPES = {"zg_qr_sizeof_detection": C.c_size_t, "zg_qr_sizeof_grid": C.c_size_t, "zg_qr_scratch_bytes": C.c_size_t}
QR_EXPORTED_SYMBOLS = tuple(_QR_SIGNATURES)

# the geometry-fitting module: every symbol include/zignal_hip_transform.h declares
_FIT = C.POINTER(ZgTransformFit)
_TRANSFORM_SIGNATURES = {
    "zg_transform_sizeof_fit": [],
    "zg_transform_chunk": [],
    "zg_transform_fit_points": [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "zg_transform_fit_matches": [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p],
    "zg_transform_fit_points_host": [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, _U32P, _FIT],
    "zg_transform_fit_matches_host": [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _U32P, C.c_int, _FIT],
    "zg_transform_project_points": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "zg_transform_project_points_host": [_FIT, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32],
    "zg_transform_invert": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "zg_transform_invert_host": [_FIT, C.c_int, _FIT],
    "zg_warp_fitted": [_IMG, _IMG, C.c_void_p, _METHOD, C.c_void_p],
}
_TRANSFORM_RESTYPES = {"zg_transform_sizeof_fit": C.c_size_t, "zg_transform_chunk": C.c_uint32}
TRANSFORM_EXPORTED_SYMBOLS = tuple(_TRANSFORM_SIGNATURES)

# the seam-carving module: every symbol include/zignal_hip_seam.h declares
_SEAM_SIGNATURES = {
    "zg_seam_band_rows": [],
    "zg_seam_strip_cols": [],
    "zg_seam_energy": [_IMG, C.c_void_p, C.c_void_p],
    "zg_seam_find": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p],
    "zg_seam_remove": [_IMG, C.c_void_p, _IMG, C.c_void_p],
    "zg_seam_carve": [_IMG, _IMG, C.c_uint32, C.c_int, _IMG, C.c_void_p, C.c_void_p],
    "zg_seam_energy_host": [_IMG, C.c_void_p],
    "zg_seam_find_host": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "zg_seam_remove_host": [_IMG, C.c_void_p, _IMG],
    "zg_seam_carve_host": [_IMG, _IMG, C.c_uint32, C.c_int, _IMG, C.c_void_p],
}
_SEAM_RESTYPES = {"zg_seam_band_rows": C.c_uint32, "zg_seam_strip_cols": C.c_uint32}
SEAM_EXPORTED_SYMBOLS = tuple(_SEAM_SIGNATURES)
SEAM_VERTICAL, SEAM_HORIZONTAL = range(2)  # ZG_SEAM_VERTICAL, ZG_SEAM_HORIZONTAL


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). zignal_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for table, restypes in ((_SIGNATURES, _RESTYPES), (_ORB_SIGNATURES, _ORB_RESTYPES), (_MATCH_SIGNATURES, _MATCH_RESTYPES),
                                (_HOUGH_SIGNATURES, _HOUGH_RESTYPES), (_FLOOD_SIGNATURES, _FLOOD_RESTYPES), (_METRICS_SIGNATURES, _METRICS_RESTYPES),
                                (_QUANTIZE_SIGNATURES, _QUANTIZE_RESTYPES), (_CANVAS_SIGNATURES, _CANVAS_RESTYPES),
                                (_TEXT_SIGNATURES, _TEXT_RESTYPES), (_FDM_SIGNATURES, _FDM_RESTYPES),
                                (_TRACER_SIGNATURES, _TRACER_RESTYPES), (_QR_SIGNATURES, _QR_RESTYPES),
                                (_TRANSFORM_SIGNATURES, _TRANSFORM_RESTYPES), (_SEAM_SIGNATURES, _SEAM_RESTYPES)):
            for name, argtypes in table.items():
                fn = getattr(l, name)  # AttributeError if the library does not export it
                fn.argtypes = argtypes
                fn.restype = restypes.get(name, C.c_int)
        if l.zg_sizeof_step() != C.sizeof(ZgStep):  # zg_step has no size field: a library built from another header must not be handed ZgStep arrays
            raise ImportError(f"{LIB_PATH}: sizeof(zg_step) is {l.zg_sizeof_step()} in the library, {C.sizeof(ZgStep)} in this binding: rebuild the library")
        if l.zg_sizeof_draw_cmd() != C.sizeof(ZgDrawCmd):  # the same rule for zg_draw_cmd arrays
            raise ImportError(f"{LIB_PATH}: sizeof(zg_draw_cmd) is {l.zg_sizeof_draw_cmd()} in the library, {C.sizeof(ZgDrawCmd)} in this binding: rebuild the library")
        for name, struct in (("zg_sizeof_font", ZgFont), ("zg_sizeof_glyph", ZgGlyph), ("zg_sizeof_text_cmd", ZgTextCmd)):  # and for the text module's three
            if getattr(l, name)() != C.sizeof(struct):
                raise ImportError(f"{LIB_PATH}: {name}() is {getattr(l, name)()} in the library, {C.sizeof(struct)} in this binding: rebuild the library")
        for name, struct in (("zg_fdm_sizeof_moments", ZgFdmMoments), ("zg_fdm_sizeof_target", ZgFdmTarget), ("zg_fdm_sizeof_transform", ZgFdmTransform)):
            if getattr(l, name)() != C.sizeof(struct):
                raise ImportError(f"{LIB_PATH}: {name}() is {getattr(l, name)()} in the library, {C.sizeof(struct)} in this binding: rebuild the library")
        for name, struct in (("zg_qr_sizeof_detection", ZgQrDetection), ("zg_qr_sizeof_grid", ZgQrGrid)):
            if getattr(l, name)() != C.sizeof(struct):
                raise ImportError(f"{LIB_PATH}: {name}() is {getattr(l, name)()} in the library, {C.sizeof(struct)} in this binding: rebuild the library")
        if l.zg_transform_sizeof_fit() != C.sizeof(ZgTransformFit):
            raise ImportError(f"{LIB_PATH}: zg_transform_sizeof_fit() is {l.zg_transform_sizeof_fit()} in the library, {C.sizeof(ZgTransformFit)} in this binding: rebuild the library")
        _lib = l
    return _lib


def check(status: int) -> None:
    if status == OK:
        return
    msg = (lib().zg_last_error() or b"").decode("utf-8", "replace")
    if status == ERR_DIMENSION_MISMATCH:
        raise DimensionMismatch(status, msg)
    if status == ERR_INVALID_ARGUMENT:
        raise InvalidArgument(status, msg)
    if status == ERR_OUT_OF_MEMORY:
        raise MemoryError(f"zignal_hip: {msg}")
    if status == ERR_CODEC:
        raise CodecError(status, msg)
    raise ZignalError(status, msg)

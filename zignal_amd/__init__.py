"""zignal_amd — MI355X (gfx950) implementation of zignal's per-pixel image hot path.

The product is `libzignal_hip.so` (hand-written HIP kernels behind the C ABI in
include/zignal_hip.h); this package is the thin host-side mirror of the reference's `Image(T)`
surface on top of it. There is no CPU fallback: importing works without a GPU, calling does not.
"""
from ._lib import (BORDER_MIRROR, BORDER_REPLICATE, BORDER_WRAP, BORDER_ZERO, CS_GRAY, CS_HSL, CS_HSV, CS_LAB, CS_LCH, CS_LMS, CS_OKLAB, CS_OKLCH, CS_RGB,
                   CS_RGBA, CS_XYB, CS_XYZ, CS_YCBCR, CodecError, DimensionMismatch, InvalidArgument, ZignalError, lib)
from .image import (BINARY_DESCRIPTOR_DTYPE, KEYPOINT_DTYPE, AffineTransform, BinaryDescriptor, Orb, Blending, BorderMode, Fast, Image, ImagePyramid, Interpolation, ProjectiveTransform,
                    SimilarityTransform, convolve_separable_planes, gaussian_blur_planes, gaussian_kernel, lanczos_plane_weights)
from .flood import FloodFillOptions, flood_fill_bound, flood_fill_tile
from .metrics import METRIC_RESULT_DTYPE, psnr_from_mse, ssim_window, sum_f64_chunk, sum_f64_sequential
from .quantize import DitherMode, PaletteMode, build_palette, dither_geometry, median_cut_from_histogram, palette_lut
from .hough import HOUGH_LINE_DTYPE, HoughLine, HoughTransform
from .match import MATCH_DTYPE, BruteForceMatcher, MatchStats
from .pipeline import Multi, Pipeline, Step
from .canvas import DRAW_CMD_DTYPE, Canvas, canvas_tile
from .text import GLYPH_DTYPE, TEXT_CMD_DTYPE, BitmapFont
from .fdm import FeatureDistributionMatching, NoSourceSet, NoTargetSet
from .tracer import Tracer
from .qr import QrDetector, QrGrid
from .transform import FIT_DTYPE, FitError, FittedTransform
from .seam import seam_band_rows, seam_energy, seam_find, seam_strip_cols

__all__ = ["seam_band_rows", "seam_strip_cols", "seam_energy", "seam_find","FIT_DTYPE", "FitError", "FittedTransform", "transform", "QrDetector", "QrGrid", "Tracer", "FeatureDistributionMatching", "NoTargetSet", "NoSourceSet", "Canvas", "DRAW_CMD_DTYPE", "canvas_tile", "BitmapFont", "GLYPH_DTYPE", "TEXT_CMD_DTYPE", "Image", "ImagePyramid", "Fast", "Orb", "BruteForceMatcher", "MatchStats", "MATCH_DTYPE", "HoughTransform", "HoughLine", "HOUGH_LINE_DTYPE", "FloodFillOptions", "flood_fill_bound", "flood_fill_tile", "METRIC_RESULT_DTYPE", "psnr_from_mse", "ssim_window", "sum_f64_chunk", "sum_f64_sequential", "DitherMode", "PaletteMode", "build_palette", "dither_geometry", "median_cut_from_histogram", "palette_lut", "KEYPOINT_DTYPE", "BINARY_DESCRIPTOR_DTYPE", "BinaryDescriptor", "Interpolation", "BorderMode", "Blending", "ProjectiveTransform", "AffineTransform",
           "SimilarityTransform", "Pipeline", "Step", "Multi", "gaussian_kernel", "gaussian_blur_planes", "convolve_separable_planes", "lanczos_plane_weights", "DimensionMismatch", "InvalidArgument", "CodecError", "ZignalError", "lib", "png", "jpeg"]

from . import fdm, jpeg, png, transform  # noqa: E402,F401

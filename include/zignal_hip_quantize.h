/* zignal_hip_quantize.h — the quantisation module of libzignal_hip.so: the colour histogram, median cut, the nearest-colour lookup table
 * (reference src/image/quantize.zig), the dither modes (src/image/dither.zig) and mapImageToPalette (src/codecs/gif.zig:875-920) as
 * device operations. Included by zignal_hip.h (include that one); zg_image, zg_stream and the status codes come from there.
 * A palette is n entries of three bytes (r, g, b), 1 <= n <= 256; a lookup table is 32768 bytes indexed by r5 << 10 | g5 << 5 | b5.
 * Out of scope, here and in the library: the GIF container and its LZW, sixel output, and Mode.auto's heuristic. */
#ifndef ZIGNAL_HIP_QUANTIZE_H
#define ZIGNAL_HIP_QUANTIZE_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZG_HISTOGRAM_CELLS 32768u            /* 1 << (3 * color_quantize_bits) */
#define ZG_HISTOGRAM_UNTOUCHED 0xFFFFFFFFu   /* `first` of a cell that no pixel falls in */

/* dither.Mode (dither.zig:18-30), the reference's ordinals */
#define ZG_DITHER_NONE 0
#define ZG_DITHER_FLOYD_STEINBERG 1
#define ZG_DITHER_ATKINSON 2
#define ZG_DITHER_ORDERED 3
#define ZG_DITHER_AUTO 4 /* a no-op, as in dither.apply: the caller resolves it */

/* PaletteMode (quantize.zig:476-498), the reference's ordinals */
#define ZG_PALETTE_FIXED_6X7X6 0
#define ZG_PALETTE_FIXED_VGA16 1
#define ZG_PALETTE_FIXED_WEB216 2
#define ZG_PALETTE_ADAPTIVE 3

/* ---- histogram (quantize.zig:188-237) ------------------------------------------------------------------------------------------ */

/* The 5-bit-per-channel histogram medianCut starts from. The key of a pixel is r5 << 10 | g5 << 5 | b5 of convertColor(Rgb, pixel):
 * a u8 replicates to (v, v, v), an Rgba drops its alpha. counts[key] is the cell's population; first[key] is the raster index
 * row * cols + col (cols, not the stride) of the first pixel of the cell in scan order, ZG_HISTOGRAM_UNTOUCHED for an empty cell:
 * ascending `first` is the order of the reference's touched_indices. Both are device arrays of ZG_HISTOGRAM_CELLS words, overwritten.
 * ZG_PIXEL_U8, RGB_U8 and RGBA_U8, views included; other pixel types and rows * cols >= 2^32: ZG_ERR_UNSUPPORTED.
 * Asynchronous on `stream`, two launches, no host synchronisation, recordable into a graph. */
ZG_API int zg_color_histogram(const zg_image *img, uint32_t *counts_device, uint32_t *first_device, zg_stream stream);

/* ---- median cut (quantize.zig:175-412) ----------------------------------------------------------------------------------------- */

/* medianCut from a histogram, host arithmetic, no GPU needed. counts and first are host arrays of ZG_HISTOGRAM_CELLS words as
 * zg_color_histogram leaves them. Up to min(max_colors, capacity) entries are written to palette_rgb (capacity entries of three
 * bytes) and *n receives how many. No touched cell, max_colors == 0 or capacity == 0: ZG_ERR_INVALID_ARGUMENT (error.NoPaletteColors).
 * The boxes are sorted with a restatement of Zig's std.sort.heap, which is unstable: the palette of an image with equal keys in a
 * box's longest dimension rests on that restatement. */
ZG_API int zg_median_cut_from_histogram_host(const uint32_t *counts, const uint32_t *first, uint32_t max_colors, uint32_t capacity,
                                             uint8_t *palette_rgb, uint32_t *n);

/* medianCut of a device image: the histogram, one download of 256 KiB, then the host function (up to 255 dependent heap sorts of up to
 * 32768 entries stay on the host). palette_rgb and n are host memory. Works on the default stream and synchronises it once: not recordable
 * into a graph, and not to be called while another stream of the process is capturing. */
ZG_API int zg_median_cut(const zg_image *img_device, uint32_t max_colors, uint32_t capacity, uint8_t *palette_rgb, uint32_t *n);

/* buildPalette (quantize.zig:502-527): palette_rgb is 256 host entries. The fixed modes are host tables and touch neither img (which
 * may be NULL) nor the device; ZG_PALETTE_ADAPTIVE is zg_median_cut with capacity 256, falling back to the 6x7x6 palette when it fails,
 * as the reference's catch does. Another mode: ZG_ERR_INVALID_ARGUMENT. */
ZG_API int zg_build_palette(const zg_image *img_device, int mode, uint32_t max_colors, uint8_t *palette_rgb, uint32_t *n);

/* ---- lookup table (ColorLookupTable.init, quantize.zig:66-159) ----------------------------------------------------------------- */

/* Every cell's nearest palette entry: the cell's colour is (v << 3 | v >> 2) per channel, the score dist << 8 | index is minimised,
 * so ties go to the lowest index. n outside 1 .. 256: ZG_ERR_INVALID_ARGUMENT. Asynchronous, one launch, recordable into a graph. */
ZG_API int zg_palette_lut(const uint8_t *palette_device, uint32_t n, uint8_t *lut_device, zg_stream stream);
/* The same on the host, no GPU needed. */
ZG_API int zg_palette_lut_host(const uint8_t *palette, uint32_t n, uint8_t *lut);

/* ---- dither (dither.zig:34-331) ------------------------------------------------------------------------------------------------ */

/* The three constants of the error-diffusion kernel (tests put shapes on both sides of each): a wave owns band_rows rows, the waves of
 * a workgroup advance phase_cols columns between barriers, and one launch covers rows_per_launch rows. Any pointer may be NULL. */
ZG_API void zg_dither_geometry(uint32_t *band_rows, uint32_t *phase_cols, uint32_t *rows_per_launch);

/* dither.apply, in place on a ZG_PIXEL_RGB_U8 device image (a view too; bytes outside it stay untouched): every pixel becomes a
 * palette colour. lut_device is the table of that palette (zg_palette_lut). Modes none and auto do nothing. Another pixel type:
 * ZG_ERR_UNSUPPORTED; n outside 1 .. 256 or another mode: ZG_ERR_INVALID_ARGUMENT.
 * Error diffusion is one workgroup per frame and ceil(rows / rows_per_launch) launches, the rows handed from one launch to the next
 * through 8 * (cols + 1) bytes of scratch per launch boundary. Asynchronous, a fixed number of launches, recordable into a graph. */
ZG_API int zg_dither(const zg_image *img, const uint8_t *palette_device, uint32_t n, const uint8_t *lut_device, int mode, zg_stream stream);

/* The same over n_frames frames of img's shape, frame_bytes apart (frame_bytes >= the bytes one frame spans): one workgroup per frame,
 * which is how error diffusion fills the device. */
ZG_API int zg_dither_frames(const zg_image *img, uint32_t n_frames, size_t frame_bytes, const uint8_t *palette_device, uint32_t n,
                            const uint8_t *lut_device, int mode, zg_stream stream);

/* ---- map to palette (mapImageToPalette, gif.zig:875-920) ------------------------------------------------------------------------ */

/* indices (ZG_PIXEL_U8, src's rows and cols, may be a view: bytes outside it stay untouched) receives each pixel's palette index.
 * src is ZG_PIXEL_U8, RGB_U8 or RGBA_U8 and is not written. Without dither: lut.lookup(convertColor(Rgb, pixel)). With use_dither:
 * the pixels are converted to an Rgb frame in scratch, dithered with Floyd-Steinberg, and looked up. transparent_index < 0 means none;
 * 0 .. 255 reserves the palette's last entry: the lookup table is built over the first n - 1 entries (n >= 2 then), and on
 * ZG_PIXEL_RGBA_U8 a pixel whose alpha is below 128 gets transparent_index, on the dither path too (the original alpha decides).
 * The table is built inside the call. Asynchronous, a fixed number of launches, recordable into a graph. */
ZG_API int zg_palette_map(const zg_image *src, const zg_image *indices, const uint8_t *palette_device, uint32_t n, int use_dither,
                          int transparent_index, zg_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_QUANTIZE_H */

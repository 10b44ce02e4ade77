/* zignal_hip_seam.h — the seam-carving module of libzignal_hip.so: the reference's seam_carve example (examples/src/seam_carving.zig:
 * computeEnergy, computeSeam, removeSeam and the iteration that ties them to Image.sobel) as device operations, bit for bit. Included by
 * zignal_hip.h (include that one); zg_image, zg_stream and the status codes come from there. */
#ifndef ZIGNAL_HIP_SEAM_H
#define ZIGNAL_HIP_SEAM_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- content-aware resize (examples/src/seam_carving.zig) ------------------------------------------------------------------- */

#define ZG_SEAM_VERTICAL 0   /* the reference: a seam runs from the top row to the bottom row and every row loses one column */
#define ZG_SEAM_HORIZONTAL 1 /* the library's own: every column loses one row (defined through the transposed frame, see zg_seam_carve) */

/* The tile of the energy kernel (tests put shapes on both sides of them): a launch covers zg_seam_band_rows() rows, a wave owns
 * zg_seam_strip_cols() output columns of them. */
ZG_API uint32_t zg_seam_band_rows(void);
ZG_API uint32_t zg_seam_strip_cols(void);

/* All device forms below: asynchronous on `stream`, no host synchronisation, copy or upload, a number of launches that depends on
 * (rows, cols, n) alone, status codes decided before anything is enqueued, recordable into a graph from a process's first call, scratch
 * from the library's scratch owner. In a process without a device a call answers its argument errors, then ZG_ERR_HIP. */

/* computeEnergy (:22-45). edges is an Image(u8); energy is rows * cols packed words. Row 0 is the edge row; below it
 * energy[r][c] = edges[r][c] + min(energy[r-1][c-1], energy[r-1][c], energy[r-1][c+1]), where column -1 does not exist and column `cols`
 * stands for column cols - 1. An empty image writes nothing. rows * cols must stay below 2^31 (ZG_ERR_UNSUPPORTED). */
ZG_API int zg_seam_energy(const zg_image *edges, uint32_t *energy, zg_stream stream);

/* computeSeam (:47-74). seam[rows - 1] is the first column of the bottom row that holds its minimum. Going up, seam[r] starts as
 * s = seam[r + 1], and the columns s - 1, s, s + 1 (the same two border rules) replace it, in that order, when their energy in row r is
 * strictly below the current choice's: the centre wins ties, then the left, then the right. rows or cols of 0: ZG_ERR_INVALID_ARGUMENT
 * (the reference indexes row rows - 1). rows * cols must stay below 2^31 (ZG_ERR_UNSUPPORTED). */
ZG_API int zg_seam_find(const uint32_t *energy, uint32_t rows, uint32_t cols, uint32_t *seam, zg_stream stream);

/* removeSeam (:76-102), out of place: dst is rows x (cols - 1) of src's pixel type (any of the six) and shares no byte with src
 * (ZG_ERR_INVALID_ARGUMENT); dst[r][c] = src[r][c + (c >= seam[r])]. seam is `rows` device words. An entry >= cols removes nothing from
 * its row and drops the row's last pixel. Nothing outside dst's rows x cols rectangle is written: the bytes between cols and stride are
 * left alone. Shapes that do not fit: ZG_ERR_DIMENSION_MISMATCH; different pixel types: ZG_ERR_INVALID_ARGUMENT. */
ZG_API int zg_seam_remove(const zg_image *src, const uint32_t *seam, const zg_image *dst, zg_stream stream);

/* n iterations of seam_carve (:104-144): Image.sobel of the current frame, computeEnergy, computeSeam, removeSeam; the edge map is
 * computed anew from the carved frame every time. src is left unchanged; dst is rows x (cols - n) of src's pixel type (every type
 * zg_sobel takes: all six) and shares no byte with src. 1 <= n < cols and rows >= 1 (ZG_ERR_INVALID_ARGUMENT), rows * cols < 2^31
 * (ZG_ERR_UNSUPPORTED), dst of another shape: ZG_ERR_DIMENSION_MISMATCH.
 * seams_device, when not NULL, is n * rows device words: seams_device[k * rows + r] is the column removed from row r at iteration k, in
 * that iteration's coordinates (what the reference writes to seam_ptr on its k-th call).
 * axis ZG_SEAM_HORIZONTAL removes rows. It is this library's definition, the reference has none (its exported `transpose` is not a
 * transposition): t[c][r] = src[r][c], t is carved vertically n times, and dst is the transpose of the result. dst is then
 * (rows - n) x cols, 1 <= n < rows, cols >= 1, and seams_device is n * cols words (the row removed from column c at iteration k).
 * energy_source is reserved for a protect / remove mask: anything but NULL is ZG_ERR_UNSUPPORTED.
 * The working frames, the edge map and the energy map are scratch: about 2 * sizeof(pixel) + 5 bytes per pixel (the transposed frames
 * on top of that for the horizontal axis). The result equals the four staged calls in a loop, byte for byte. */
ZG_API int zg_seam_carve(const zg_image *src, const zg_image *dst, uint32_t n, int axis, const zg_image *energy_source, uint32_t *seams_device,
                         zg_stream stream);

/* Host pointers (images, energy, seam, seams), synchronous. */
ZG_API int zg_seam_energy_host(const zg_image *edges, uint32_t *energy);
ZG_API int zg_seam_find_host(const uint32_t *energy, uint32_t rows, uint32_t cols, uint32_t *seam);
ZG_API int zg_seam_remove_host(const zg_image *src, const uint32_t *seam, const zg_image *dst);
ZG_API int zg_seam_carve_host(const zg_image *src, const zg_image *dst, uint32_t n, int axis, const zg_image *energy_source, uint32_t *seams);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_SEAM_H */

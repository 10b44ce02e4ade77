/* zignal_hip_hough.h — the Hough module of libzignal_hip.so: HoughTransform.init / compute / findLines (reference
 * src/image/hough.zig) as device operations on the library's own edge maps. Included by zignal_hip.h (include that one); zg_image,
 * zg_stream and the status codes come from there. */
#ifndef ZIGNAL_HIP_HOUGH_H
#define ZIGNAL_HIP_HOUGH_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- image: HoughTransform (src/image/hough.zig) --------------------------------------------------------------------------- */

/* HoughTransform.Line (hough.zig:13-25), field for field: 28 bytes. angle in degrees, radius from the centre, score the vote count,
 * p1 / p2 (x, y) the segment clipped to [0, size]^2 (unclipped when clipLine returns early). */
typedef struct zg_hough_line {
    float angle, radius;
    uint32_t score;
    float p1[2], p2[2];
} zg_hough_line;

/* A HoughTransform: size, even_size and the two i32 tables, the tables on the device that was current at creation. */
typedef struct zg_hough *zg_hough_t;

/* The largest size: the reference computes rho = x_val * cos[t] + y_val * sin[t] and ((rho >> 1) + (offset << 1)) in i32 (a trap on
 * overflow in Zig's safe builds). |x_val|, |y_val| <= size - 1 and |cos[t]| + |sin[t]| <= 65536 (both are 65536 / sqrt 2 times a
 * cosine and sine of one angle, truncated), so |rho| <= (size - 1) * 65536 < 2^31 needs size <= 32768; offset << 1 is
 * 32768 * even_size, so the sum stays below 2^30 + 2^30 for even_size <= 32768. Larger sizes: ZG_ERR_UNSUPPORTED. */
#define ZG_HOUGH_MAX_SIZE 32768u
/* The largest max_candidates of zg_hough_find_lines (ZG_ERR_UNSUPPORTED above it). */
#define ZG_HOUGH_MAX_CANDIDATES 1048576u

/* The largest size whose voting keeps a strip of theta columns in LDS; above it (or with ZIGNAL_HIP_HOUGH_DIRECT=1 in the environment,
 * read once per process) every vote is a global atomic. The results are the same bytes; tests put sizes on both sides of it. */
ZG_API uint32_t zg_hough_lds_max_size(void);
/* The edge list is shared out among the workgroups of the voting kernel in multiples of this many pixels (tests put the edge count
 * on both sides of a multiple). */
ZG_API uint32_t zg_hough_pixel_chunk(void);

/* The tables of HoughTransform.init (hough.zig:49-56): cos_table[t] = trunc(65536 * cos(theta) / sqrt(2)), theta = t * pi / even_size,
 * in f64, with Zig's cos and sin restated (musl's __cos / __sin / __rem_pio2). `size` entries each. Host arithmetic, no GPU needed.
 * size <= 1: ZG_ERR_INVALID_ARGUMENT; size > ZG_HOUGH_MAX_SIZE: ZG_ERR_UNSUPPORTED. */
ZG_API int zg_hough_tables_host(uint32_t size, int32_t *cos_table, int32_t *sin_table);

/* HoughTransform.init / deinit. The tables are uploaded once, synchronously. zg_hough_create_with_tables takes them from the caller
 * (a Zig host passes the ones its own HoughTransform.init made, so nothing of the restatement is on its path). In a process without a
 * device the transform is still created: its calls answer their argument errors, then ZG_ERR_HIP. */
ZG_API int zg_hough_create(uint32_t size, zg_hough_t *out);
ZG_API int zg_hough_create_with_tables(uint32_t size, const int32_t *cos_table, const int32_t *sin_table, zg_hough_t *out);
ZG_API int zg_hough_destroy(zg_hough_t h);
ZG_API uint32_t zg_hough_size(zg_hough_t h);

/* HoughTransform.compute (hough.zig:75-139). edges is Image(u8) (ZG_ERR_UNSUPPORTED otherwise), the box (l, t, r, b) must be size x
 * size (ZG_ERR_DIMENSION_MISMATCH, the reference's assert), accumulator is size rows of size u32, acc_stride (>= size) words apart.
 * Every non-zero edge byte of box ∩ image votes once per theta column t, at row rr = ((rho >> 1) + (offset << 1)) >> 16 when
 * 0 <= rr < size. The votes are ADDED to what the accumulator holds (clear it first, as with the reference); a box that misses the
 * image adds nothing. Integer adds commute: the result equals the reference's bit for bit in any order of execution. Status codes are
 * decided before anything is enqueued. Asynchronous on `stream`, no host synchronisation, recordable into a graph. */
ZG_API int zg_hough_compute(zg_hough_t h, const zg_image *edges, uint32_t l, uint32_t t, uint32_t r, uint32_t b, uint32_t *accumulator,
                            size_t acc_stride, zg_stream stream);

/* HoughTransform.findLines (hough.zig:142-204) of a size x size accumulator (the reference loops over the accumulator's own
 * dimensions; this narrows it to the transform's). Candidates: interior cells with votes >= threshold and no 8-neighbour strictly
 * greater, in row-major order, then a stable sort by score descending (the key (score desc, row * size + col asc) is unique), then
 * greedy suppression with the reference's two f32 clauses and strict <, so NaN or negative thresholds suppress nothing. Each kept
 * candidate becomes a line through getLineProperties, createLine and clipLine in f32, operation for operation.
 * threshold_device, when not NULL, is a device word read by the kernels in place of `threshold`.
 * counts (device, two words): counts[0] = the full number of candidates. When it exceeds max_candidates (<= ZG_HOUGH_MAX_CANDIDATES)
 * counts[1] = 0 and no line is written: call again with a larger bound. Otherwise counts[1] = the full number of lines and the first
 * min(counts[1], capacity) of the reference's list are in `lines` (device). size < 3 gives [0, 0].
 * Asynchronous on `stream`, no host synchronisation, recordable into a graph. */
ZG_API int zg_hough_find_lines(zg_hough_t h, const uint32_t *accumulator, size_t acc_stride, uint32_t threshold,
                               const uint32_t *threshold_device, float angle_nms_thresh, float radius_nms_thresh, uint32_t max_candidates,
                               zg_hough_line *lines, uint32_t capacity, uint32_t *counts, zg_stream stream);

/* Host pointers throughout (edges->data, accumulator, lines, counts), synchronous. The accumulator is read, added to and written back.
 * lines may be NULL with capacity 0 to ask for the counts alone. */
ZG_API int zg_hough_compute_host(zg_hough_t h, const zg_image *edges, uint32_t l, uint32_t t, uint32_t r, uint32_t b, uint32_t *accumulator,
                                 size_t acc_stride);
ZG_API int zg_hough_find_lines_host(zg_hough_t h, const uint32_t *accumulator, size_t acc_stride, uint32_t threshold, float angle_nms_thresh,
                                    float radius_nms_thresh, uint32_t max_candidates, zg_hough_line *lines, uint32_t capacity, uint32_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_HOUGH_H */

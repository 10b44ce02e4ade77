/* zignal_hip_tracer.h — the Tracer module of libzignal_hip.so: Tracer.trace (reference src/features/Tracer.zig) as a device operation
 * from an Image(u8) edge map to polylines, and the builder that turns those polylines into a Canvas command list. Included by
 * zignal_hip.h (include that one); zg_image, zg_stream and the status codes come from there, zg_draw_cmd from zignal_hip_canvas.h. */
#ifndef ZIGNAL_HIP_TRACER_H
#define ZIGNAL_HIP_TRACER_H

#include "zignal_hip.h"
#include "zignal_hip_canvas.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- features: Tracer (src/features/Tracer.zig) ------------------------------------------------------------------------------ */

/* Tracer's two fields (Tracer.zig:20-25). */
typedef struct zg_tracer_options {
    uint32_t min_path_length;     /* 5: a path of fewer raw points is dropped (its pixels stay visited) */
    float simplification_epsilon; /* 1.0: Ramer-Douglas-Peucker distance; paths are simplified iff this is > 0 (0, negative, NaN: raw paths) */
} zg_tracer_options;

/* The bytes of scratch one zg_trace_paths call on a rows x cols map takes from the library's cache (about 35 per pixel). */
ZG_API size_t zg_trace_scratch_bytes(uint32_t rows, uint32_t cols);

/* Tracer.trace(edges) (Tracer.zig:46-80): the same paths, in the same order, with the same f32 bits as the reference making the same
 * call. edges is Image(u8) on the device (a view is taken as a view: the bytes between cols and stride are never read); a pixel is an
 * edge iff its byte is > 0. A point is (x = col, y = row) as two f32.
 *   points        point_capacity (x, y) pairs; the points of path i are points[2 * path_offsets[i] .. 2 * path_offsets[i + 1])
 *   path_offsets  path_capacity + 1 words
 *   counts        four words: [0] the paths the reference returns, [1] the points they hold (after simplification),
 *                 [2] the paths written, [3] the points written
 * Only whole paths are written, in order, and writing stops at the first path that does not fit either capacity: counts[2] and
 * counts[3] say how far it went, path_offsets[counts[2]] == counts[3], and nothing beyond points[2 * counts[3]) and
 * path_offsets[counts[2] + 1) is written. counts[0] and counts[1] do not depend on the capacities: a second call with them as
 * capacities returns everything. points may be NULL when point_capacity is 0.
 * opt NULL means the defaults (5, 1.0). min_path_length is compared with the raw length, before simplification; paths of fewer than
 * 3 points are copied.
 * A pixel type other than u8, or rows * cols >= 2^31: ZG_ERR_UNSUPPORTED. Status codes are decided before anything is enqueued.
 * Asynchronous on `stream`, a fixed number of launches for a given size, zg_trace_scratch_bytes of scratch, no host synchronisation,
 * copy or upload, recordable into a graph from a process's first call. In a process without a device the call answers its argument
 * errors, then ZG_ERR_HIP. */
ZG_API int zg_trace_paths(const zg_image *edges, const zg_tracer_options *opt, float *points, uint32_t point_capacity, uint32_t *path_offsets,
                          uint32_t path_capacity, uint32_t *counts, zg_stream stream);

/* Host pointers (edges->data, points, path_offsets, counts), synchronous. points may be NULL with point_capacity 0 and path_offsets
 * NULL with path_capacity 0, to ask for counts alone. */
ZG_API int zg_trace_paths_host(const zg_image *edges, const zg_tracer_options *opt, float *points, uint32_t point_capacity, uint32_t *path_offsets,
                               uint32_t path_capacity, uint32_t *counts);

/* The device-side builder from zg_trace_paths's three device outputs to a Canvas command list (see the two builders of
 * zignal_hip_canvas.h): one ZG_DRAW_LINE per consecutive pair of points of every written path, in path order, one lane per segment.
 * A path of one point gives no command. capacity is the length of cmds_out: the first min(segments, capacity) commands are written
 * and *count_out (a device word, the count_device of zg_canvas_draw) receives that number. color: four host bytes, r g b a.
 * Asynchronous on `stream`, one launch, no synchronisation, recordable into a graph. */
ZG_API int zg_canvas_cmds_from_paths(const float *points, const uint32_t *path_offsets, const uint32_t *counts, uint32_t capacity,
                                     const uint8_t *color, uint32_t width, int mode, zg_draw_cmd *cmds_out, uint32_t *count_out, zg_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_TRACER_H */

/* zignal_hip_orb.h — the ORB module of libzignal_hip.so: Orb.detect / compute / detectAndCompute (reference src/features/orb.zig,
 * BinaryDescriptor.zig) as device operations on top of zg_pyramid_build and FAST. Included by zignal_hip.h (include that one); the
 * types it builds on (zg_image, zg_keypoint, zg_stream) and the status codes are declared there. */
#ifndef ZIGNAL_HIP_ORB_H
#define ZIGNAL_HIP_ORB_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- features: ORB (src/features/orb.zig, BinaryDescriptor.zig) --------------------------------------------------------- */

/* BinaryDescriptor (src/features/BinaryDescriptor.zig:10): 256 bits, bit i at bits[i / 8] & (1 << (i % 8)). */
typedef struct zg_binary_descriptor {
    uint8_t bits[32];
} zg_binary_descriptor;
typedef enum zg_orb_score { ZG_ORB_HARRIS_SCORE = 0, ZG_ORB_FAST_SCORE = 1 } zg_orb_score; /* Orb.ScoreType (orb.zig:113-116) */
/* Orb's fields and defaults (orb.zig:87-109). n_levels, edge_threshold, first_level, wta_k and fast_threshold are u8 there: values
 * above 255 are ZG_ERR_INVALID_ARGUMENT, as are n_levels == 0, scale_factor <= 1 (the pyramid's assert), wta_k != 2 (the only
 * descriptor the reference has) and an image whose pyramid stops before n_levels (a level below 8 x 8; the reference then indexes
 * past the pyramid's end). More than 32 levels: ZG_ERR_UNSUPPORTED. orientation_weights: NULL, or a host pointer to the caller's
 * 31 x 31 orientation weight table (orb.zig:340-357; a Zig host passes its comptime @exp values) — such a call uploads the table
 * synchronously and cannot be recorded into a graph; with NULL the kernels build the table from the library's exp. */
typedef struct zg_orb_params {
    uint32_t n_features;     /* 500 */
    float scale_factor;      /* 1.2 */
    uint32_t n_levels;       /* 8 */
    uint32_t edge_threshold; /* 15 */
    uint32_t first_level;    /* 0 */
    uint32_t wta_k;          /* 2 */
    uint32_t fast_threshold; /* 20 */
    int32_t score_type;      /* ZG_ORB_FAST_SCORE */
    const float *orientation_weights;
} zg_orb_params;
ZG_API void zg_orb_default_params(zg_orb_params *params);
/* Orb.computeFeaturesPerLevel (orb.zig:279-334) into out[n_levels] and Orb.computeAdaptiveThreshold (:511-517); host arithmetic
 * with the library's pow. zg_orb_adaptive_threshold returns the threshold, or a negative status for invalid parameters. */
ZG_API int zg_orb_features_per_level(const zg_orb_params *params, uint32_t *out);
ZG_API int zg_orb_adaptive_threshold(const zg_orb_params *params, uint32_t level);
/* Orb.detectAndCompute (orb.zig:250-276) of an Image(u8) as one device operation: the pyramid, FAST on every level, [Harris
 * responses,] the per-level selection, border filter and orientation, and the descriptors; keypoints and descriptors in the
 * reference's order, bit for bit. keypoints / descriptors / count: device pointers; descriptors may be NULL (Orb.detect, :119-130).
 * *count receives the reference's count (<= n_features); the first min(*count, capacity) entries of both arrays are written.
 * Asynchronous on `stream`, no host synchronisation, recordable into a graph (with orientation_weights == NULL). */
ZG_API int zg_orb_detect_and_compute(const zg_image *src, const zg_orb_params *params, zg_keypoint *keypoints,
                                     zg_binary_descriptor *descriptors, uint32_t capacity, uint32_t *count, zg_stream stream);
/* Orb.compute (orb.zig:133-144, 224-247): the descriptors of n caller-supplied keypoints (device pointers), each on level
 * min(max(0, octave), n_levels - 1) at (x / scale, y / scale). */
ZG_API int zg_orb_compute(const zg_image *src, const zg_orb_params *params, const zg_keypoint *keypoints, uint32_t n,
                          zg_binary_descriptor *descriptors, zg_stream stream);
/* Host pointers, synchronous. keypoints (and descriptors) may be NULL with capacity 0 to query the count. */
ZG_API int zg_orb_detect_and_compute_host(const zg_image *src, const zg_orb_params *params, zg_keypoint *keypoints,
                                          zg_binary_descriptor *descriptors, uint32_t capacity, uint32_t *count);
ZG_API int zg_orb_compute_host(const zg_image *src, const zg_orb_params *params, const zg_keypoint *keypoints, uint32_t n,
                               zg_binary_descriptor *descriptors);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_ORB_H */

/* zignal_hip_match.h — the matcher module of libzignal_hip.so: BruteForceMatcher.match / knnMatch / radiusMatch and
 * MatchStats.compute (reference src/features/matcher.zig) as device operations on ORB's descriptor arrays. Included by zignal_hip.h
 * (include that one); zg_binary_descriptor comes from zignal_hip_orb.h, zg_stream and the status codes from zignal_hip.h. */
#ifndef ZIGNAL_HIP_MATCH_H
#define ZIGNAL_HIP_MATCH_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- features: BruteForceMatcher (src/features/matcher.zig) -------------------------------------------------------------- */

/* Match (matcher.zig:10-19) with 32-bit indices: 12 bytes. distance is the Hamming distance, 0 .. 256, as f32. */
typedef struct zg_match {
    uint32_t query_idx, train_idx;
    float distance;
} zg_match;
/* A descriptor array and how much of it counts: n = count ? min(*count, capacity) : capacity. In the device forms data and count are
 * device pointers (count is the word zg_orb_detect_and_compute wrote, which may exceed capacity) and n is read by the kernels; in
 * the _host forms both are host pointers. data must be 4-byte aligned (ZG_ERR_INVALID_ARGUMENT otherwise). */
typedef struct zg_descriptor_set {
    const zg_binary_descriptor *data;
    uint32_t capacity;
    const uint32_t *count;
} zg_descriptor_set;
/* BruteForceMatcher's fields and defaults (matcher.zig:33-41). */
typedef struct zg_matcher_params {
    int32_t cross_check;     /* false */
    uint32_t max_distance;   /* 64 */
    float ratio_threshold;   /* 0.8 */
} zg_matcher_params;
/* MatchStats (matcher.zig:237-241). */
typedef struct zg_match_statistics {
    size_t total_matches;
    float mean_distance, min_distance, max_distance;
} zg_match_statistics;

ZG_API void zg_matcher_default_params(zg_matcher_params *params);
/* The train descriptors one workgroup of the nearest-neighbour kernel stages at a time: results are the same on either side of a
 * multiple of it, which is what the tests put their sizes around. */
ZG_API uint32_t zg_match_train_chunk(void);

/* BruteForceMatcher.match (matcher.zig:44-106): per query the nearest train descriptor (the lowest index among equals) and the second
 * smallest distance; kept when best <= max_distance and (one train descriptor or f32(best) < ratio_threshold * f32(second)), and, with
 * cross_check, when the query is the lowest-index nearest query of that train descriptor (:214-233). Ascending query order. *count
 * (device) receives the full length, the first min(*count, capacity) entries of matches (device) are written. An empty side, known
 * only at run time or not, gives *count = 0. Asynchronous on `stream`, no host synchronisation, recordable into a graph. */
ZG_API int zg_match_descriptors(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params,
                                zg_match *matches, uint32_t capacity, uint32_t *count, zg_stream stream);
/* BruteForceMatcher.knnMatch (:109-162): row q = the first min(k, n_train) train entries ordered by (distance, train index), cut at
 * the first with distance > max_distance, at matches[q * k + j]; row_counts[q] is its length, 0 for the rows from n_query up to
 * query->capacity (row_counts holds query->capacity words). query->capacity * k >= 2^32: ZG_ERR_UNSUPPORTED. */
ZG_API int zg_match_knn(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params, uint32_t k,
                        zg_match *matches, uint32_t *row_counts, zg_stream stream);
/* BruteForceMatcher.radiusMatch (:165-212): row q = every train entry with f32(distance) <= max_dist ordered by (distance, train
 * index); a NaN or negative max_dist gives empty rows. Rows back to back in query order: row_counts[q] (query->capacity words) is
 * the full length of row q, *count their sum, and the first min(*count, capacity) entries of the concatenation are written.
 * query->capacity * train->capacity >= 2^32: ZG_ERR_UNSUPPORTED. */
ZG_API int zg_match_radius(const zg_descriptor_set *query, const zg_descriptor_set *train, float max_dist, zg_match *matches,
                           uint32_t capacity, uint32_t *row_counts, uint32_t *count, zg_stream stream);
/* Host pointers throughout, synchronous. matches may be NULL (with capacity 0 where there is one) to ask for the counts alone;
 * row_counts of zg_match_radius_host may be NULL as well. */
ZG_API int zg_match_descriptors_host(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params,
                                     zg_match *matches, uint32_t capacity, uint32_t *count);
ZG_API int zg_match_knn_host(const zg_descriptor_set *query, const zg_descriptor_set *train, const zg_matcher_params *params, uint32_t k,
                             zg_match *matches, uint32_t *row_counts);
ZG_API int zg_match_radius_host(const zg_descriptor_set *query, const zg_descriptor_set *train, float max_dist, zg_match *matches,
                                uint32_t capacity, uint32_t *row_counts, uint32_t *count);
/* MatchStats.compute (:237-270) of n host matches: a sequential f32 sum divided by f32(n), min from floatMax, max from 0; all zeros
 * for n == 0. Host arithmetic. */
ZG_API int zg_match_stats(const zg_match *matches, size_t n, zg_match_statistics *out);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_MATCH_H */

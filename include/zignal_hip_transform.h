/* zignal_hip_transform.h — the geometry-fitting module of libzignal_hip.so: SimilarityTransform.find, AffineTransform.find and
 * ProjectiveTransform.find (reference src/geometry/transforms.zig:47-112, :155-191, :242-290) as one device operation each, from two
 * point arrays or from a match list and its two keypoint arrays, and Image.warp with the fitted matrix read from device memory. With
 * these "two frames in, aligned frame out" (ORB twice, match, fit, warp) is one enqueued chain with no host visit.
 *   fit        one workgroup per fit. One header (zignal_amd/csrc/zg_transform_fit.h) holds the reference's arithmetic for the host and
 *              the device: the sequential sums, the Golub-Reinsch SVD (src/matrix/svd.zig:149-495) at 2 x 2, 9 x 9 and N x 3, the 8 x 8
 *              Gauss-Jordan solve of the four-point path, the pseudo-inverse. Every rounded operation is the header's, in its order.
 *   record     zg_transform_fit, in device memory: the matrix in f64 and f32 as zg_warp takes it, and a status
 *   warp       zg_warp_fitted: zg_warp with m32 of a device record
 * Results are the reference's bit for bit with one documented departure: AffineTransform.find on 86 or more points. There Matrix.gemm
 * (src/matrix/Matrix.zig:749) hands q.dot(pinv) to its SIMD kernel, whose association depends on the reference build's vector width and on
 * @reduce's unspecified order, so no single reference value exists; this library keeps the scalar chain.
 * Bounds: similarity and projective up to 65536 points, affine up to 4096; at least 2 / 3 / 4 points (the reference's asserts).
 * Included by zignal_hip.h (include that one); zg_image, zg_keypoint, zg_match, zg_method, zg_stream and the status codes come from
 * there. */
#ifndef ZIGNAL_HIP_TRANSFORM_H
#define ZIGNAL_HIP_TRANSFORM_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ZG_SCALAR_F32 = 0, ZG_SCALAR_F64 = 1 }; /* the T of SimilarityTransform(T) ...: the type the fit's arithmetic runs in */

enum {
    ZG_FIT_OK = 0,
    ZG_FIT_NOT_CONVERGED = 1,  /* error.NotConverged: the SVD passed 300 iterations at a singular value (svd_converged says which) */
    ZG_FIT_RANK_DEFICIENT = 2, /* error.RankDeficient: no rank (similarity), rank < 3 (affine), collinear points or a singular 8 x 8 system
                                  (projective); zg_transform_invert: the matrix has no inverse */
    ZG_FIT_BAD_COUNT = 3,      /* fewer points than the kind's minimum, or more than its bound */
    ZG_FIT_BAD_INPUT = 4       /* a match names a keypoint outside its array */
};

#define ZG_FIT_MAX_POINTS 65536u       /* similarity, projective */
#define ZG_FIT_MAX_POINTS_AFFINE 4096u /* affine: its N x 3 U lives in one workgroup's LDS */

/* The result of a fit, 128 bytes.
 *   kind            zg_transform_kind
 *   status          ZG_FIT_*. Anything but ZG_FIT_OK leaves m the identity, the reference's value before find.
 *   n_points        the points the fit ran on: count ? min(*count, capacity) : capacity
 *   svd_converged   the SVD's `converged` (0, or the k it stopped at)
 *   m64, m32        the matrix as zg_warp takes it: {a00,a01,a10,a11, b0,b1, 0,0,0} for similarity and affine, row-major 3 x 3 for
 *                   projective. An f64 fit: m64 is the result and m32 its .as(f32) (@floatCast); an f32 fit: m32 is the result and m64
 *                   holds the same values widened. */
typedef struct zg_transform_fit {
    int32_t kind, status;
    uint32_t n_points, svd_converged;
    double m64[9];
    float m32[9];
    uint32_t reserved;
} zg_transform_fit;

ZG_API size_t zg_transform_sizeof_fit(void);
/* The points one stage of an ordered sum takes: all lanes of the workgroup compute that many points' products into LDS, then one lane per
 * sum adds them in index order. Results are the same on either side of a multiple of it, which is what the tests put their sizes
 * around. */
ZG_API uint32_t zg_transform_chunk(void);

/* find(from, to): the transform that maps from[i] onto to[i]. from, to: `capacity` points of two scalars (x, y) of type `scalar`, device
 * memory; count: NULL or a device word, n = count ? min(*count, capacity) : capacity, read by the kernel; out: a device record, every word
 * of it written. Asynchronous on `stream`, no host synchronisation, recordable into a graph (the scratch comes from the library's
 * stream-ordered cache, as everywhere). capacity above the kind's bound is allowed when a count word keeps n under it. */
ZG_API int zg_transform_fit_points(int kind, int scalar, const void *from, const void *to, uint32_t capacity, const uint32_t *count,
                                   zg_transform_fit *out, zg_stream stream);
/* The same from a match list: point i is (query_kps[matches[i].query_idx], train_kps[matches[i].train_idx]), x and y widened to
 * `scalar`. The fit maps query onto train; with train_to_query != 0 it maps train onto query, which is what zg_warp needs to resample
 * the query frame onto the train frame's grid (warp maps a destination pixel to its source). n_query, n_train: the lengths of the
 * keypoint arrays; an index at or above its length makes the record ZG_FIT_BAD_INPUT and is never followed. All pointers device memory. */
ZG_API int zg_transform_fit_matches(int kind, int scalar, const zg_keypoint *query_kps, uint32_t n_query, const zg_keypoint *train_kps,
                                    uint32_t n_train, const zg_match *matches, uint32_t capacity, const uint32_t *count, int train_to_query,
                                    zg_transform_fit *out, zg_stream stream);
/* The same header on the CPU: host pointers throughout, no GPU needed. The return value is ZG_OK whenever a record was written; the
 * fit's own outcome is the record's status. */
ZG_API int zg_transform_fit_points_host(int kind, int scalar, const void *from, const void *to, uint32_t capacity, const uint32_t *count,
                                        zg_transform_fit *out);
ZG_API int zg_transform_fit_matches_host(int kind, int scalar, const zg_keypoint *query_kps, uint32_t n_query, const zg_keypoint *train_kps,
                                         uint32_t n_train, const zg_match *matches, uint32_t capacity, const uint32_t *count, int train_to_query,
                                         zg_transform_fit *out);

/* project (transforms.zig:39-42, :147-150, :224-231) of n points with a record's matrix, in `scalar` (m32 for f32, m64 for f64), a lane
 * per point; a record whose status is not ZG_FIT_OK is the identity and projects as such. in, out, fit: device memory; in == out is
 * fine. */
ZG_API int zg_transform_project_points(const zg_transform_fit *fit, int scalar, const void *in, void *out, uint32_t n, zg_stream stream);
ZG_API int zg_transform_project_points_host(const zg_transform_fit *fit, int scalar, const void *in, void *out, uint32_t n);
/* ProjectiveTransform.inv (SMatrix.inv of 3 x 3, SMatrix.zig:685-726) in `scalar`: out receives the inverse, or, where the reference
 * returns null (a zero determinant), the identity with ZG_FIT_RANK_DEFICIENT. A record of another kind is ZG_FIT_BAD_INPUT; a record
 * that is not ZG_FIT_OK is copied. fit, out: device memory. */
ZG_API int zg_transform_invert(const zg_transform_fit *fit, int scalar, zg_transform_fit *out, zg_stream stream);
ZG_API int zg_transform_invert_host(const zg_transform_fit *fit, int scalar, zg_transform_fit *out);

/* zg_warp with kind and m32 of a device record: Image.warp (src/image/transforms.zig:522-531) with no host visit between the fit and
 * the resampling. A record whose status is not ZG_FIT_OK leaves dst untouched. src, dst: device images of one pixel type. */
ZG_API int zg_warp_fitted(const zg_image *src, const zg_image *dst, const zg_transform_fit *fit_dev, const zg_method *method,
                          zg_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_TRANSFORM_H */

/* zignal_hip_fdm.h — the feature-distribution-matching module of libzignal_hip.so: FeatureDistributionMatching(T) (reference src/fdm.zig)
 * for T = u8, Rgb(u8), Rgba(u8) as three device stages and the chains over them. It moves the colour statistics (mean and 3 x 3
 * covariance) of a target image onto a source image, in place.
 *   moments    one pass over a frame: exact integer sums (any reduction order gives the same words)
 *   solve      moments -> mean, covariance -> the reference's SVD and products -> a 3 x 3 matrix and a bias, or a scale and an offset;
 *              one header (zignal_amd/csrc/zg_fdm_solve.h) compiled for the host and the device
 *   apply      the per-pixel map, in place, with the reference's roundings
 * The one departure from the reference's bits: its mean and covariance come from Welford's recurrence (src/stats.zig:261-280), a
 * division per sample that no order-free form reproduces; the device's come from the exact moments, each within 2 ulp of the true value.
 * Everything after the statistics is the reference's arithmetic bit for bit, so an output byte can differ only where the reference's own
 * value before @round lies within that noise of a half-integer, or, for the whole image, where a covariance that is exactly zero leaves
 * noise in the recurrence whose sign decides a sign of the reference's SVD. A caller who needs the reference's bytes feeds
 * zg_fdm_target_host / zg_fdm_transform_host its own Welford statistics and uploads the result for zg_fdm_apply.
 * A view (stride != cols) is an image of its own: the result is the reference's on a contiguous copy, and the bytes between cols and
 * stride are never read or written. rows * cols < 2^32. Pixel types other than the three are ZG_ERR_UNSUPPORTED (fdm.zig:20).
 * Included by zignal_hip.h (include that one); zg_image, zg_stream and the status codes come from there. */
#ifndef ZIGNAL_HIP_FDM_H
#define ZIGNAL_HIP_FDM_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The integer moments of one frame, in device memory. Alpha takes no part in any of them.
 *   n                 rows * cols
 *   sum, prod         colour frames: the sums of r, g, b and of rr, rg, rb, gg, gb, bb; zero on a u8 frame
 *   lum_sum, lum_sq   the sum and the sum of squares of the byte itself (u8) or of the luminance byte convertColor(u8, pixel), BT.709 in
 *                     16.16 fixed point (src/color.zig:1031-1041): what the reference takes a colour source's statistics on when the
 *                     target is grey (fdm.zig:155-162)
 *   not_gray          non-zero when some pixel has r != g or g != b (fdm.zig:87); zero on a u8 frame
 *   pixel             the frame's zg_pixel */
typedef struct zg_fdm_moments {
    uint64_t n;
    uint64_t sum[3];
    uint64_t prod[6];
    uint64_t lum_sum, lum_sq;
    uint32_t not_gray;
    int32_t pixel;
} zg_fdm_moments;

/* What setTarget keeps (fdm.zig:29-32). u is row-major and all zeros for a grey target, whose U the reference leaves empty and whose
 * variance is s[0]. status: 0, or the k of the SVD's `converged` (error.NotConverged, fdm.zig:113-115). */
typedef struct zg_fdm_target {
    double mean[3];
    double u[9];
    double s[3];
    int32_t is_gray;
    int32_t status;
    int32_t pixel;
    int32_t reserved;
} zg_fdm_target;

enum { ZG_FDM_ROUTE_COLOR = 0, ZG_FDM_ROUTE_SCALAR = 1, ZG_FDM_ROUTE_GRAY_TARGET = 2 };
#define ZG_FDM_STATUS_TYPE_MISMATCH (-1) /* a transform asked for a frame of another pixel type than its target's */

/* What update applies to every pixel (fdm.zig:177-272).
 *   colour route        res_j = r * w[0][j] + g * w[1][j] + b * w[2][j] + bias[j], added left to right, r = byte / 255.0 in f64;
 *                       @round(255.0 * clamp(res_j, 0, 1)), half away from zero; the alpha of Rgba(u8) stays
 *   scalar route (u8)   val * scale + offset with the same tail
 *   grey-target route   a colour frame against a grey target: the luminance byte through the scalar map, written to r, g and b. On
 *                       Rgba(u8) ALPHA BECOMES 0: the struct literal of fdm.zig:196 leaves `a` at its field default (color.zig:405)
 * A non-zero status leaves the frame untouched: the reference returns error.NotConverged before it writes (fdm.zig:210-212). */
typedef struct zg_fdm_transform {
    int32_t route;
    int32_t status;
    double w[9]; /* row-major */
    double bias[3];
    double scale, offset;
} zg_fdm_transform;

ZG_API size_t zg_fdm_sizeof_moments(void);
ZG_API size_t zg_fdm_sizeof_target(void);
ZG_API size_t zg_fdm_sizeof_transform(void);
/* Steps a lane of the moments kernel adds into 32-bit partial sums before it widens them to 64 bits. A step adds at most 16 * 255^2, so
 * anything up to 4128 cannot wrap. */
ZG_API uint32_t zg_fdm_lane_run(void);
/* Frames one launch of a _frames call serves (their descriptors travel as kernel arguments, which keeps the call recordable). */
ZG_API uint32_t zg_fdm_frames_per_launch(void);

/* ---- 1. moments. Asynchronous on `stream`, recordable into a graph from a process's first call: two launches, every word of the record written, 96
 * bytes of scratch per workgroup (at most about 200 KB a frame). */
ZG_API int zg_fdm_compute_moments(const zg_image *img, zg_fdm_moments *moments_dev, zg_stream stream);
/* frames: n descriptors in host memory (read at the call), any sizes, any of the three types; moments_dev: n records */
ZG_API int zg_fdm_compute_moments_frames(const zg_image *frames, uint32_t n, zg_fdm_moments *moments_dev, zg_stream stream);

/* ---- 2. solve. One-wave kernels around zg_fdm_solve.h; all pointers are device memory. */
ZG_API int zg_fdm_target_from_moments(const zg_fdm_moments *moments_dev, zg_fdm_target *target_dev, zg_stream stream);
/* pixel: the type of the frame the moments are of; it must be the target's (else the transform's status is
 * ZG_FDM_STATUS_TYPE_MISMATCH: the target lives on the device, the call cannot look) */
ZG_API int zg_fdm_transform_from_moments(const zg_fdm_moments *moments_dev, int pixel, const zg_fdm_target *target_dev, zg_fdm_transform *transform_dev,
                                         zg_stream stream);
/* n moments -> n transforms against one target, one lane per frame; each record's own `pixel` is the frame's type */
ZG_API int zg_fdm_transform_from_moments_frames(const zg_fdm_moments *moments_dev, uint32_t n, const zg_fdm_target *target_dev,
                                                zg_fdm_transform *transforms_dev, zg_stream stream);
/* The same code on the host, from statistics as f64: mean[3], cov[9] row-major (for the two scalar routes mean[0] and cov[0] are the
 * byte's, resp. the luminance byte's). No GPU needed. ZG_ERR_UNSUPPORTED for another pixel type; an SVD that does not converge is
 * ZG_ERR_INVALID_ARGUMENT, zg_last_error() starting with "NotConverged", and *out carries the status. is_gray is ignored (taken as 1) for
 * ZG_PIXEL_U8. */
ZG_API int zg_fdm_target_host(int pixel, const double mean[3], const double cov[9], int is_gray, zg_fdm_target *out);
ZG_API int zg_fdm_transform_host(int pixel, const zg_fdm_target *target, const double mean[3], const double cov[9], zg_fdm_transform *out);
/* moments (host memory) -> the statistics the device kernels derive from them. luminance != 0: those of lum_sum / lum_sq, three times
 * over; 0: those of sum / prod. mean = S / (255 n), cov = (n Sxy - Sx Sy) / (65025 n (n - 1)), 0 for n <= 1: numerator and denominator
 * exact in 128-bit integers, each rounded to f64 once, one division. */
ZG_API int zg_fdm_stats_from_moments_host(const zg_fdm_moments *moments, int luminance, double mean[3], double cov[9]);

/* ---- 3. apply, in place; transform(s) in device memory. */
ZG_API int zg_fdm_apply(const zg_image *img, const zg_fdm_transform *transform_dev, zg_stream stream);
ZG_API int zg_fdm_apply_frames(const zg_image *frames, uint32_t n, const zg_fdm_transform *transforms_dev, zg_stream stream);

/* ---- 4. chains: moments of both, target, transform, apply, with no synchronisation, copy or upload; recordable from a process's first
 * call; usable from several streams and host threads. src and target have the same pixel type (else ZG_ERR_INVALID_ARGUMENT); src is
 * matched in place. */
ZG_API int zg_fdm_match(const zg_image *src, const zg_image *target, zg_stream stream);
/* n frames of one pixel type against one target, whose statistics are computed once: `target` (an image), or when it is NULL
 * `prepared_dev` (a device zg_fdm_target of zg_fdm_target_from_moments, or an uploaded zg_fdm_target_host) */
ZG_API int zg_fdm_match_frames(const zg_image *frames, uint32_t n, const zg_image *target, const zg_fdm_target *prepared_dev, zg_stream stream);
/* host pixels, synchronous; NotConverged as in the host forms above */
ZG_API int zg_fdm_match_host(const zg_image *src, const zg_image *target);
ZG_API int zg_fdm_match_frames_host(const zg_image *frames, uint32_t n, const zg_image *target);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_FDM_H */

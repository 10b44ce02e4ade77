/* zignal_hip_flood.h — the flood-fill module of libzignal_hip.so: Image(T).floodFill (reference src/image/flood_fill.zig) as a device
 * operation, in place, on any of the six pixel types. Included by zignal_hip.h (include that one); zg_image, zg_stream and the status
 * codes come from there. */
#ifndef ZIGNAL_HIP_FLOOD_H
#define ZIGNAL_HIP_FLOOD_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- image: floodFill (src/image/flood_fill.zig) ---------------------------------------------------------------------------- */

#define ZG_FLOOD_MODE_SEED 0     /* every candidate is compared with the seed pixel's original value */
#define ZG_FLOOD_MODE_NEIGHBOR 1 /* every candidate is compared with the original value of the pixel it was reached from */

/* FloodFillOptions (flood_fill.zig:5-26). connectivity is 4 ((-1,0) (1,0) (0,-1) (0,1)) or 8 (the four diagonals as well). */
typedef struct zg_flood_fill_options {
    double threshold; /* 0 */
    int connectivity; /* 4 */
    int mode;         /* ZG_FLOOD_MODE_SEED */
} zg_flood_fill_options;

/* The side of the square tiles that are labelled in LDS (tests put shapes on both sides of it). */
ZG_API uint32_t zg_flood_fill_tile(void);

/* The constant the kernels compare with, from the threshold: host arithmetic, no GPU needed. pixelDistance (flood_fill.zig:28-51) is
 * |f64(a) - f64(b)| for scalar pixels and the f64 square root of the f64 sum of squared f64 differences over all fields (alpha
 * included) for struct pixels; sqrt is monotone and correctly rounded, so sqrt(s) <= t is s <= S(t), S(t) the largest f64 whose
 * square root is <= t (found by bisection over bit patterns), and no square root is taken on the device.
 *   ZG_PIXEL_U8                     D, the largest integer in -1 .. 255 with D <= t: the kernels test |a - b| <= D in integers
 *   ZG_PIXEL_RGB_U8 / RGBA_U8       floor(S(t)) clipped to 4 * 255^2, or -1: the integer sum of squares is compared with it
 *   ZG_PIXEL_F32                    t, or -1 when t is negative or NaN: |f64(a) - f64(b)| <= t in f64
 *   ZG_PIXEL_RGB_F32 / RGBA_F32     S(t), or -1: the f64 sum, in field order, is compared with it
 * A negative or NaN threshold gives -1 (nothing joins), -0.0 counts as 0, S(inf) = inf. */
ZG_API int zg_flood_fill_bound_host(int pixel, double threshold, double *bound);

/* Image(T).floodFill (flood_fill.zig:59-131). The reference marks `visited` before it pushes and writes fill_value when it pops, so
 * every value it compares is an original one, and both distances are symmetric: the filled set is the connected component of the seed
 * in the undirected graph whose links are, between adjacent pixels p and q (4- or 8-adjacent),
 *   seed mode       dist(orig[p], orig[seed]) <= threshold and dist(orig[q], orig[seed]) <= threshold, the seed itself always passing
 *   neighbor mode   dist(orig[p], orig[q]) <= threshold
 * Those pixels become *fill_value (one pixel of img's type, read by the host at the call); every other byte of the image is left
 * alone, the bytes between cols and stride included. A NaN distance joins nothing.
 * (row, col) is the seed; outside the image: ZG_ERR_INVALID_ARGUMENT (error.OutOfBounds), nothing is enqueued. seed_device, when not
 * NULL, is two device words (row, col) read by the kernels in place of row and col, which are then ignored; a pair outside the image
 * changes nothing and counts 0. filled_count_device, when not NULL, is a device word that receives the number of filled pixels.
 * opt NULL means the defaults; a connectivity other than 4 or 8, or a mode other than 0 or 1: ZG_ERR_INVALID_ARGUMENT.
 * rows * cols must stay below 2^31 (ZG_ERR_UNSUPPORTED); the call takes about five bytes of scratch per pixel.
 * Status codes are decided before anything is enqueued. Asynchronous on `stream`, a fixed number of launches, no host synchronisation,
 * copy or upload, recordable into a graph from a process's first call. In a process without a device the call answers its argument
 * errors, then ZG_ERR_HIP. */
ZG_API int zg_flood_fill(const zg_image *img, uint32_t row, uint32_t col, const uint32_t *seed_device, const void *fill_value,
                         const zg_flood_fill_options *opt, uint32_t *filled_count_device, zg_stream stream);

/* Host pointers (img->data, filled_count), synchronous. filled_count may be NULL. */
ZG_API int zg_flood_fill_host(const zg_image *img, uint32_t row, uint32_t col, const void *fill_value, const zg_flood_fill_options *opt,
                              uint32_t *filled_count);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_FLOOD_H */

/* zignal_hip_metrics.h — the image-metrics module of libzignal_hip.so: Image(T).psnr, ssim and meanPixelError (reference
 * src/image/metrics.zig) as device operations on any of the six pixel types, and the exact sequential f64 sum they end in.
 * Included by zignal_hip.h (include that one); zg_image, zg_stream and the status codes come from there. */
#ifndef ZIGNAL_HIP_METRICS_H
#define ZIGNAL_HIP_METRICS_H

#include "zignal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- image: psnr, ssim, meanPixelError (src/image/metrics.zig) -------------------------------------------------------------- */

#define ZG_SSIM_WINDOW 11 /* window_size (metrics.zig:73); an image with fewer rows or columns is error.ImageTooSmall */

/* What every metric leaves in device memory, so that a decision taken on it can stay on the device and in a graph.
 *   sum           the reference's left-to-right f64 sum over every term, bit for bit: mse before its division (metrics.zig:26,32),
 *                 total_abs (:131,140), ssim_sum (:106), or the sum of zg_sum_f64_sequential's values
 *   count         component_count (:27,33,132,141), the number of SSIM windows (weight_sum, :107), or the number of values
 *   value         psnr: mse = sum / count (:48); mean_pixel_error: (sum / count) / max_value, 0 for no components (:159-165);
 *                 ssim: sum / weight_sum (:111); zg_sum_f64_sequential: sum
 *   serial_terms  how many terms the sum added one by one (0 on the integer pixel types, whose sums are integer sums) */
typedef struct zg_metric_result {
    double sum;
    uint64_t count;
    double value;
    uint64_t serial_terms;
} zg_metric_result;

/* options of the three metrics; NULL means the defaults */
typedef struct zg_metric_options {
    const double *ssim_window; /* NULL, or the caller's 121 f64 weights (host memory, read at the call), row-major dy * 11 + dx, in place
                                  of zg_ssim_window_host's: a Zig host passes its comptime generateSsimWindow() table */
    double *ssim_map;          /* NULL, or (rows - 10) x (cols - 10) f64, contiguous: the per-window quotients numerator / denominator
                                  (:104-106) in row-major order; device memory for zg_ssim, host memory for zg_ssim_host */
} zg_metric_options;

/* The terms in one chunk of the sequential sum by default (a power of two). */
ZG_API uint32_t zg_sum_f64_chunk(void);

/* generateSsimWindow (metrics.zig:230-249): exp(-(x^2 + y^2) / (2 * 1.5 * 1.5)) for dy, dx in 0 .. 10, their left-to-right sum, then
 * one division each. Host arithmetic, no GPU needed; the exponential restates the published musl algorithm that Zig's compiler-rt
 * ports and is not pinned against Zig at the last ulp (hence zg_metric_options.ssim_window). */
ZG_API int zg_ssim_window_host(double w[121]);

/* 20 * log10(max_value) - 10 * log10(mse), and +inf for mse == 0 (metrics.zig:49-53). Host arithmetic; log10 restates musl's,
 * unpinned at the last ulp like the exponential above. */
ZG_API double zg_psnr_from_mse(double mse, double max_value);

/* The two restated functions themselves, for tests and for a host that wants the library's own numbers. */
ZG_API double zg_exp_f64_host(double x);
ZG_API double zg_log10_f64_host(double x);

/* The sum of n f64 values (device memory) in index order, starting from +0.0, rounded after every addition as a sequential loop rounds
 * it: result->sum has the bits of `for (v) s += v;` for every input. Chunks of 2^chunk_log2 terms are summed speculatively in parallel
 * (as integer multiples of the running sum's unit in the last place, for both parities of the running sum, ties included) and one
 * lane then walks the chunks in order, taking a chunk's record only where the record proves that it applies and adding the chunk term
 * by term where not; result->serial_terms counts those terms. chunk_log2 = 0 selects zg_sum_f64_chunk(); otherwise 6 .. 16
 * (ZG_ERR_INVALID_ARGUMENT outside). n must stay below 2^40 (ZG_ERR_UNSUPPORTED). A NaN sum is a NaN of unspecified payload.
 * Asynchronous on `stream`, four launches, no host synchronisation, copy or upload, recordable into a graph from a process's first
 * call. */
ZG_API int zg_sum_f64_sequential(const double *values, uint64_t n, uint32_t chunk_log2, zg_metric_result *result, zg_stream stream);

/* Image(T).psnr (metrics.zig:10-54) up to the logarithms: result->value is the mse, and zg_psnr_from_mse(value, 255 or 1) the PSNR.
 * Image(T).meanPixelError (metrics.zig:114-166): result->value is the method's return value.
 * Terms are d * d or |d| with d = f64(a) - f64(b), in row-major order, a pixel's fields in declaration order (alpha included).
 * On u8 fields every term is an integer and the f64 sum is the integer sum: shapes whose sum could reach 2^53 are ZG_ERR_UNSUPPORTED.
 * On f32 fields the terms are generated from the two images inside the sequential sum's passes, never stored.
 * a and b: same pixel type (else ZG_ERR_INVALID_ARGUMENT), same rows and cols (else ZG_ERR_DIMENSION_MISMATCH); both strides are
 * honoured and the bytes between cols and stride are never read. Status codes are decided before anything is enqueued. Asynchronous on
 * `stream`, a fixed number of launches, no host synchronisation, copy or upload, recordable into a graph from a process's first call.
 * In a process without a device the calls answer their argument errors, then ZG_ERR_HIP. */
ZG_API int zg_psnr(const zg_image *a, const zg_image *b, const zg_metric_options *opt, zg_metric_result *result, zg_stream stream);
ZG_API int zg_mean_pixel_error(const zg_image *a, const zg_image *b, const zg_metric_options *opt, zg_metric_result *result, zg_stream stream);

/* Image(T).ssim (metrics.zig:56-112): per window the five 121-term f64 accumulations in dy, dx order with the products associated as
 * written, the two @max(0, ...), the quotient by IEEE division; the quotients are then summed in row-major order by the sequential sum.
 * A pixel's scalar is getPixelScalar (:188-203): scalars as they are, Rgb(u8) / Rgba(u8) rgbLuma(r, g, b) * 255 (src/color.zig:1021-
 * 1027), every f32 struct the f64 sum of its fields divided by their number. rows or cols below 11: ZG_ERR_INVALID_ARGUMENT
 * (error.ImageTooSmall); otherwise as zg_psnr. Takes 8 bytes of scratch per window unless opt->ssim_map is given. */
ZG_API int zg_ssim(const zg_image *a, const zg_image *b, const zg_metric_options *opt, zg_metric_result *result, zg_stream stream);

/* Host pointers (a->data, b->data, opt->ssim_map), synchronous: *value is the f64 that the reference's method returns (the PSNR itself
 * for zg_psnr_host); result, when not NULL, receives the whole record. */
ZG_API int zg_psnr_host(const zg_image *a, const zg_image *b, const zg_metric_options *opt, double *value, zg_metric_result *result);
ZG_API int zg_mean_pixel_error_host(const zg_image *a, const zg_image *b, const zg_metric_options *opt, double *value, zg_metric_result *result);
ZG_API int zg_ssim_host(const zg_image *a, const zg_image *b, const zg_metric_options *opt, double *value, zg_metric_result *result);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_METRICS_H */

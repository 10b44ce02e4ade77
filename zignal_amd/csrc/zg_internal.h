// zg_internal.h — every function that one .hip of libzignal_hip defines and another calls, declared once. The defining file
// includes this header too, so a changed parameter or default argument fails to compile instead of failing to link (or worse).
// A try_* function returns -1 when the call is not one of its shapes: the caller goes on to the next route.
#pragma once
#include "zg_common.h"

namespace zg {

// A batch of n equally shaped frames, the one description every route that puts the frame in its grid takes: `src` and `dst` are frame 0,
// frame i is the same image with its data i * src_frame / i * dst_frame BYTES further on. A route converts to its own units (pixels,
// pitches) itself. FrameBatch{src, dst} is the one image (the pointers may be null there: a route's own checks come first).
struct FrameBatch {
    const zg_image *src, *dst;
    uint32_t n = 1;
    size_t src_frame = 0, dst_frame = 0;
    FrameSpan span() const { return FrameSpan{src_frame, dst_frame}; }
};

// ---- image_ops.hip
int copy_impl(const zg_image *src, const zg_image *dst, hipStream_t s);
int fill_outside_impl(const zg_image *img, const void *pixel_value, int l, int t, int r, int b, hipStream_t s);
int set_border_impl(const zg_image *img, const uint32_t rect[4], const void *pixel_value, hipStream_t s);

// ---- geom.hip
int resize_impl(const zg_image *src, const zg_image *dst, const zg_method *method, hipStream_t s);
int resize_frames(const FrameBatch &b, const zg_method *method, hipStream_t s);
int warp_frames(const FrameBatch &b, int kind, const float *mat, const zg_method *method, hipStream_t s);

// ---- resize_planes.hip
int resize_planes_impl(const zg_image *src, const zg_image *dst, const zg_method *method, hipStream_t s);
int resize_lanczos_weights_impl(const zg_image *src, const zg_image *dst, const float *wx, const float *wy, hipStream_t s);
void lanczos_plane_weights(uint32_t src_n, uint32_t dst_n, float *w);
int resize_bilinear_rgba8_frames(const FrameBatch &b, hipStream_t s);
int resize_planes_frames(const FrameBatch &b, const zg_method *method, hipStream_t s);

// ---- convert.hip
int convert_impl(const zg_image *src, int src_space, const zg_image *dst, int dst_space, const float *srgb_lut, hipStream_t s);
int resize_convert_rgba8_frames(const FrameBatch &b, int dst_space, const float *srgb_lut, hipStream_t s);

// ---- colorspaces.hip
int convert_spaces_impl(const zg_image *src, int src_space, const zg_image *dst, int dst_space, const float *srgb_lut_dev, hipStream_t s);

// ---- the separable convolution's routes, tried in conv_separable.hip's order
int try_sep_bytes(const zg_image *src, const zg_image *dst, const int32_t *ix, const int32_t *iy, int nk, int border, hipStream_t s);                        // conv_sep_bytes.hip
int try_sep_bytes2(const zg_image *src, const zg_image *dst, const int32_t *ix, int nkx, const int32_t *iy, int nky, int border, hipStream_t s);             // conv_sep_bytes2.hip
int try_sep_bytes2_frames(const FrameBatch &b, const int32_t *ix, int nkx, const int32_t *iy, int nky, int border, hipStream_t s);                          // conv_sep_bytes2.hip
int try_sep_f32long(const zg_image *src, const zg_image *dst, const float *fx, int nkx, const float *fy, int nky, int border, hipStream_t s);                // conv_sep_f32long.hip
int try_sep_f32long_grey(const zg_image *src, const zg_image *dst, const float *fx, int nkx, const float *fy, int nky, int border, hipStream_t s);           // conv_sep_f32long.hip
int try_sep_f32x4(const zg_image *src, const zg_image *dst, const float *fx, const float *fy, int nk, uint32_t skipx, uint32_t skipy,
                  int border, hipStream_t s);                                                                                                             // conv_sep_f32x4.hip
constexpr uint32_t SF_MAX_PLANES = 8; // planes per launch of conv_sep_tile_f32.hip
int try_sep_tile_f32(const zg_image *src, const zg_image *dst, uint32_t n, const float *fx, const float *fy, int nk, uint32_t skipx, uint32_t skipy,
                     int border, hipStream_t s);                                                                                                          // conv_sep_tile_f32.hip

// The integer taps every u8 Gaussian route multiplies by (conv_separable.hip): scaleKernelToInt of gaussianBlur's f32 taps.
struct GaussianTapsI32 {
    int n = 0;         // the full length, 2 ceil(3 sigma) + 1; the taps are written only when n <= capacity
    int z = 0;         // outer taps that rounded to zero, per end: taps[z .. n - z) is the kernel the single-image routes run
    int64_t sum = 0;   // of all taps
    bool bytes = false; // every tap is in 0 .. 255
};
int gaussian_taps_i32(float sigma, int32_t *taps, int capacity, GaussianTapsI32 &out); // a status: a sigma zg_gaussian_kernel refuses is refused
// What admits taps to the packed-u16 kernels: every tap of both axes is in 0 .. 255 and each axis sums to at most 257, so that a row-pass
// temp (<= 255 * 257 = 65535) fits a u16. The sums come back for the routes' clamp decisions.
struct TapSums { int64_t x = 0, y = 0; };
bool taps_pack_u16(const int32_t *ix, int nkx, const int32_t *iy, int nky, TapSums &sums);

// u8 separable convolution of a batch of frames, one wave per column strip (conv_sep_stream.hip), and the tiled Rgba(u8) form of the
// same (conv_sep_rgba8.hip). A destination of exactly half the source's rows and columns asks for blur then 2:1 bilinear (Rgba(u8) only).
// The u8 strip routes (this one, conv2d_stream.hip, sobel_stream.hip) share their arguments, filler and shape test: zg_stream.h.
int try_sep_stream(const FrameBatch &b, const int32_t *ix, const int32_t *iy, int nk, int border, hipStream_t s);
int try_sep_rgba8_batch(const FrameBatch &b, const int32_t *ix, const int32_t *iy, int nk, int border, hipStream_t s);

// ---- conv2d_stream.hip
int try_conv2d_stream(const zg_image *src, const zg_image *dst, const float *taps, int kh, int kw, int border, hipStream_t s);

// ---- box_blur.hip
int sat_planes_impl(const zg_image *src, float *sat, hipStream_t s, bool integer_valued, size_t plane_stride = 0); // 0: planes contiguous
int sat_planes_multi(const zg_image *const *srcs, float *const *sats, int count, hipStream_t s);
int box_blur_frames(const FrameBatch &b, uint32_t radius, hipStream_t s);

// ---- box_fused.hip
int try_box_fused(const FrameBatch &b, uint32_t radius, bool sharpen, hipStream_t s);

// ---- motion.hip
int motion_linear_frames(const FrameBatch &b, float cos_a, float sin_a, uint32_t distance, hipStream_t s);
int motion_radial_frames(const FrameBatch &b, float center_x, float center_y, float strength, int spin, hipStream_t s);

// ---- edges.hip: sobel's batch entry, and what canny shares with shen_castan.hip (the grey plane also with isef.hip)
int sobel_frames(const FrameBatch &b, hipStream_t s);
int canny_gray_plane(const zg_image *src, float *gray, uint8_t *gray8, hipStream_t s); // as(f32, convertColor(u8, px)) into gray, the same as bytes into gray8; either may be null
size_t hysteresis_work_bytes(uint32_t rows, uint32_t cols);
int run_hysteresis(uint8_t *state, uint32_t rows, uint32_t cols, char *work, const zg_image *dst, hipStream_t s, const char *who);
int launch_emit(const uint8_t *state, int *label, const uint8_t *flag, const zg_image *dst, hipStream_t s);

// ---- sobel_stream.hip
int try_sobel_stream(const FrameBatch &b, hipStream_t s);

// ---- isef.hip
void isef_plane(const float *gray, const uint8_t *gray8, float *sm, float *tmp, float *t1, float *t2, uint32_t *check, uint32_t rows, uint32_t cols, float smooth,
                hipStream_t s);
bool isef_2d_applies(uint32_t rows, uint32_t cols);
size_t isef_check_bytes(uint32_t rows, uint32_t cols);

// ---- the pyramid: pyramid.hip (the host side), conv_sep_bytes2.hip and pyramid_tile.hip (the kernels)
int resize_impl_bilinear_u8(const zg_image *src, const zg_image *dst, hipStream_t s); // pyramid.hip: what zg_resize(.bilinear) runs for a u8 plane
int try_pyramid_levels_u8(const zg_image *src, const zg_image *levels, const float *sigmas, uint32_t n, uint8_t *handled, int which, hipStream_t s); // conv_sep_bytes2.hip: several levels in three launches
int try_pyramid_tiles_u8(const zg_image *src, const zg_image *levels, const float *sigmas, uint32_t n, uint8_t *handled, hipStream_t s); // pyramid_tile.hip: a level per kernel, nothing but the level written
int try_pyramid_level_u8(const zg_image *src, const zg_image *level, const int32_t *taps, int nk, hipStream_t s); // conv_sep_bytes2.hip: blur + bilinear level

// ---- fast.hip: FAST for ORB, 8-byte list entries
int fast_detect_compact(const zg_image *images, uint32_t n, const uint32_t *thresholds, uint32_t *const *pos, uint32_t *const *key,
                        const uint32_t *capacities, uint32_t *const *counts, hipStream_t s);

// ---- flood.hip: the component labelling of a plane of link bytes (bit 0 E, 1 S, 2 SE, 3 SW: the links a pixel owns), for tracer.hip.
// label: rows * cols ints; afterwards label[p] is p's parent in a forest whose roots are the smallest index of each component.
int flood_label_components(const uint8_t *links, int *label, uint32_t rows, uint32_t cols, hipStream_t s);
constexpr uint8_t FLOOD_LINK_E = 1, FLOOD_LINK_S = 2, FLOOD_LINK_SE = 4, FLOOD_LINK_SW = 8;

} // namespace zg

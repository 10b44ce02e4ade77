// batch.hip — a recipe of steps (the CLI's `pipeline` command, reference src/cli/pipeline.zig:153-179) over N independent frames laid out back to
// back. Frames are independent units: this is also the shard a rank processes in the multi-GPU bench (no halo, no collective on the data path).
//
// Two entries, one runner (run_steps): zg_batch_pipeline takes any recipe, zg_batch_blur_resize is the recipe [gaussianBlur(sigma), resize] built on
// the stack. The result of every step equals the Image method on every frame (the tests compare against exactly that).
//   * run_steps walks the batch in groups whose intermediates fit two ping-pong scratch blocks, tries each step together with its successor
//     (run_fused_pair) and then alone; a step is one launch over the group wherever its kernel takes the frame in its grid, frame by frame otherwise.
//   * the u8 Gaussian has ONE route list, gaussian_u8_routes: the stream kernel (conv_sep_stream.hip), the tiled Rgba(u8) kernel (conv_sep_rgba8.hip),
//     the two passes through u16 temp planes (conv_sep_bytes2.hip). [blur, resize(.bilinear) to exactly half] of Rgba(u8) frames asks the same list
//     for its blur + 2:1 form (one launch, the blurred frames never written); everything else is the blur, then resize_frames.
#include "zg_internal.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

namespace zg {

namespace {

struct Shape { // of the frames between two steps: what apply_shape tracks
    uint32_t rows, cols;
    int pixel, space;
    size_t frame_bytes() const { return (size_t)rows * cols * pixel_size(pixel); }
    zg_image at(void *data) const { return zg_image{data, cols, rows, cols, pixel}; }
};

int apply_shape(const zg_step &st, Shape &f) { // what a step does to shape and type; validates the step
    switch (st.kind) {
    case ZG_STEP_GAUSSIAN_BLUR:
        ZG_REQUIRE(st.sigma >= 0, ZG_ERR_INVALID_ARGUMENT, "pipeline: InvalidSigma (%g)", st.sigma);
        return ZG_OK;
    case ZG_STEP_BOX_BLUR: return ZG_OK;
    case ZG_STEP_MEDIAN_BLUR: // the CLI's own limit (src/cli/blur.zig:118-121), which is also the kernels': radius <= 256 (order_stat.hip: k_order_stat to 15, k_order_stat_hist from 16)
        ZG_REQUIRE(st.radius <= 256, ZG_ERR_INVALID_ARGUMENT, "pipeline: median blur radius %u exceeds 256", st.radius);
        return ZG_OK;
    case ZG_STEP_MOTION_BLUR:
        ZG_REQUIRE(st.motion >= ZG_MOTION_LINEAR && st.motion <= ZG_MOTION_RADIAL_SPIN, ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid motion blur kind %d", st.motion);
        return ZG_OK;
    case ZG_STEP_EDGES:
        ZG_REQUIRE(st.edges >= ZG_EDGES_SOBEL && st.edges <= ZG_EDGES_SHEN_CASTAN, ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid edge detector %d", st.edges);
        return ZG_OK;
    case ZG_STEP_RESIZE:
    case ZG_STEP_WARP:
        ZG_REQUIRE(st.method.kind >= ZG_INTERP_NEAREST && st.method.kind <= ZG_INTERP_LANCZOS, ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid interpolation method %d", st.method.kind);
        if (st.kind == ZG_STEP_WARP) ZG_REQUIRE(st.transform >= ZG_TRANSFORM_SIMILARITY && st.transform <= ZG_TRANSFORM_PROJECTIVE, ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid transform %d", st.transform);
        f.rows = st.out_rows;
        f.cols = st.out_cols;
        return ZG_OK;
    case ZG_STEP_CONVERT:
        ZG_REQUIRE(pixel_valid(st.dst_pixel), ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid pixel type %d", st.dst_pixel);
        ZG_REQUIRE(st.dst_space >= ZG_CS_GRAY && st.dst_space <= ZG_CS_XYB, ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid colour space %d", st.dst_space);
        f.pixel = st.dst_pixel;
        f.space = st.dst_space;
        return ZG_OK;
    }
    set_error("pipeline: unknown step kind %d", st.kind);
    return ZG_ERR_INVALID_ARGUMENT;
}

int per_frame(const FrameBatch &b, const std::function<int(const zg_image *, const zg_image *)> &op) {
    zg_image src = *b.src, dst = *b.dst;
    for (uint32_t i = 0; i < b.n; ++i) {
        src.data = (char *)b.src->data + (size_t)i * b.src_frame;
        dst.data = (char *)b.dst->data + (size_t)i * b.dst_frame;
        if (const int rc = op(&src, &dst)) return rc;
    }
    return ZG_OK;
}

// The routes of gaussianBlur(sigma) on u8 frames that take the batch in their grid, in the order they are tried; -1 when none applies (the
// caller goes frame by frame). A destination of exactly half the source asks for blur + 2:1 bilinear, which the first two have a form for.
//   1. try_sep_stream: 3 .. 9 taps while (taps / 2 + 1) x bytes per pixel <= 16, 16-byte rows.
//   2. try_sep_rgba8_batch: Rgba(u8), 3 .. 9 taps, columns a multiple of 4. Both this and route 3 take the 9-tap Rgba(u8) blur that route 1
//      refuses; this one first: 64 x 1080p at sigma 1.2 then a bicubic resize, 0.80 ms against 1.08 ms with route 3 first, through either
//      entry (profiles/batch_one_runner.txt).
//   3. try_sep_bytes2_frames: up to 65 taps through u16 temp planes, a batch only (one frame does better in zg_gaussian_blur, which drops
//      the outer taps that rounded to zero).
// The taps are the integers convolveSeparable derives from gaussianBlur's f32 taps (convolution.zig:303-309), all of them: the batch routes
// do not drop the zero end taps (a known follow-up: DESIGN.md §1, the batch row).
int gaussian_u8_routes(const FrameBatch &b, float sigma, hipStream_t s) {
    int32_t taps[255];
    GaussianTapsI32 t;
    if (const int rc = gaussian_taps_i32(sigma, taps, 255, t)) return rc;
    if (t.n > 255) return -1;
    int rc = try_sep_stream(b, taps, taps, t.n, ZG_BORDER_MIRROR, s);
    if (rc < 0) rc = try_sep_rgba8_batch(b, taps, taps, t.n, ZG_BORDER_MIRROR, s);
    if (rc < 0 && b.n > 1) rc = try_sep_bytes2_frames(b, taps, t.n, taps, t.n, ZG_BORDER_MIRROR, s);
    return rc;
}

int run_blur(const FrameBatch &b, float sigma, hipStream_t s) {
    if (sigma == 0) { ZG_HIP(hipMemcpyAsync(b.dst->data, b.src->data, b.n * b.src_frame, hipMemcpyDeviceToDevice, s)); return ZG_OK; } // image.zig:966
    if (!pixel_is_float(b.src->pixel))
        if (const int rc = gaussian_u8_routes(b, sigma, s); rc >= 0) return rc;
    return per_frame(b, [&](const zg_image *src, const zg_image *dst) { return zg_gaussian_blur(src, dst, sigma, (zg_stream)s); });
}

int run_resize(const FrameBatch &b, const zg_method &method, hipStream_t s) {
    if (const int rc = resize_frames(b, &method, s); rc >= 0) return rc; // one launch over the batch wherever the path is a single kernel
    return per_frame(b, [&](const zg_image *src, const zg_image *dst) { return resize_impl(src, dst, &method, s); });
}

int run_convert(const FrameBatch &b, int src_space, int dst_space, const float *lut, hipStream_t s) {
    // per pixel, and the frames are contiguous: the batch is one tall image
    const uint64_t tall = (uint64_t)b.src->rows * b.n;
    if (tall <= 0x7fffffffu) {
        zg_image src = *b.src, dst = *b.dst;
        src.rows = dst.rows = (uint32_t)tall;
        return convert_impl(&src, src_space, &dst, dst_space, lut, s);
    }
    return per_frame(b, [&](const zg_image *src, const zg_image *dst) { return convert_impl(src, src_space, dst, dst_space, lut, s); });
}

// The CLI's edges step (src/cli/edges.zig:126-135): gray = frame.convert(u8); detector(gray) -> Image(u8); .convert(frame type). The
// detectors take any pixel type and start with that very conversion per pixel (edges.zig:36-45: as(f32, convertColor(u8, px))), so they
// read the frames directly; the edge maps of the whole batch go to one grey scratch plane and come back through ONE conversion launch.
// That shortcut holds for u8 frames in Gray / Rgb / Rgba. Float frames do not: Image(f32).sobel works on the raw floats (edges.zig:36-45 casts, it does
// not scale), where the bridge's frame.convert(u8) maps [0, 1] to [0, 255] first; and frames a CONVERT step left in another colour space (Oklab, Lab, Hsv ...)
// are not RGB at all. Those frames go through the bridge literally: one conversion launch to a grey u8 plane, the detector on that.
int run_edges(const zg_step &st, const FrameBatch &b, int space, hipStream_t s) {
    ScratchBlock grey(s), bridged(s); // released in the reverse order
    const Shape plane{b.src->rows, b.src->cols, ZG_PIXEL_U8, ZG_CS_GRAY};
    if (const int rc = grey.alloc(plane.frame_bytes() * b.n)) return rc;
    const zg_image g0 = plane.at(grey.p);
    zg_image bridge0{};
    FrameBatch in{b.src, &g0, b.n, b.src_frame, plane.frame_bytes()};
    const bool direct = !pixel_is_float(b.src->pixel) && (space == ZG_CS_GRAY || space == ZG_CS_RGB || space == ZG_CS_RGBA);
    if (!direct) {
        if (const int rc = bridged.alloc(plane.frame_bytes() * b.n)) return rc;
        bridge0 = plane.at(bridged.p);
        if (const int rc = run_convert(FrameBatch{b.src, &bridge0, b.n, b.src_frame, plane.frame_bytes()}, space, ZG_CS_GRAY, nullptr, s)) return rc;
        in.src = &bridge0;
        in.src_frame = plane.frame_bytes();
    }
    int rc = st.edges == ZG_EDGES_SOBEL ? sobel_frames(in, s) : -1; // one launch over the batch
    if (rc == -1)
        rc = per_frame(in, [&](const zg_image *src, const zg_image *dst) {
            if (st.edges == ZG_EDGES_SOBEL) return zg_sobel(src, dst, (zg_stream)s);
            if (st.edges == ZG_EDGES_CANNY) return zg_canny(src, dst, st.sigma, st.low, st.high, (zg_stream)s);
            return zg_shen_castan(src, dst, st.sigma, st.window, st.high, st.low, 1, st.use_nms, (zg_stream)s);
        });
    if (rc == ZG_OK) rc = run_convert(FrameBatch{&g0, b.dst, b.n, plane.frame_bytes(), b.dst_frame}, ZG_CS_GRAY, space, nullptr, s);
    return rc;
}

// one step over the batch. Motion blur, box blur and warp carry the frame index in the grid (round 5; they launched once per frame before).
int run_step(const zg_step &st, const FrameBatch &b, int src_space, int dst_space, hipStream_t s) {
    switch (st.kind) {
    case ZG_STEP_GAUSSIAN_BLUR: return run_blur(b, st.sigma, s);
    case ZG_STEP_BOX_BLUR: return box_blur_frames(b, st.radius, s);
    case ZG_STEP_RESIZE: return run_resize(b, st.method, s);
    case ZG_STEP_CONVERT: return run_convert(b, src_space, dst_space, st.srgb_lut, s);
    case ZG_STEP_MEDIAN_BLUR:
        return per_frame(b, [&](const zg_image *src, const zg_image *dst) { return zg_order_statistic_blur(src, dst, st.radius, 0, 0.5, ZG_BORDER_MIRROR, (zg_stream)s); });
    case ZG_STEP_MOTION_BLUR:
        if (st.motion == ZG_MOTION_LINEAR) return motion_linear_frames(b, st.cos_a, st.sin_a, st.distance, s);
        return motion_radial_frames(b, st.center_x, st.center_y, st.strength, st.motion == ZG_MOTION_RADIAL_SPIN, s);
    case ZG_STEP_EDGES: return run_edges(st, b, src_space, s);
    default: { // warp: the same map for every frame, one launch
        const int rc = warp_frames(b, st.transform, st.m, &st.method, s);
        if (rc != -1) return rc; // -1: more frames than one launch takes, frame by frame
        return per_frame(b, [&](const zg_image *src, const zg_image *dst) { return zg_warp(src, dst, st.transform, st.m, &st.method, (zg_stream)s); });
    }
    }
}

// two steps as one fused launch over the batch (b.dst has the second step's shape), or -1
int run_fused_pair(const zg_step &s0, const zg_step &s1, const FrameBatch &b, int src_space, hipStream_t s) {
    if (s0.kind == ZG_STEP_GAUSSIAN_BLUR && s1.kind == ZG_STEP_RESIZE && b.src->pixel == ZG_PIXEL_RGBA_U8 && s0.sigma > 0 && s1.method.kind == ZG_INTERP_BILINEAR &&
        b.src->rows == 2 * b.dst->rows && b.src->cols == 2 * b.dst->cols)
        return gaussian_u8_routes(b, s0.sigma, s);
    if (s0.kind == ZG_STEP_RESIZE && s1.kind == ZG_STEP_CONVERT && src_space == ZG_CS_RGBA && s0.method.kind == ZG_INTERP_BILINEAR)
        return resize_convert_rgba8_frames(b, s1.dst_space, s1.srgb_lut, s);
    return -1;
}

// The recipe over the batch, every argument already checked. Frames go through in groups: two ping-pong scratch blocks hold a group's
// intermediates (a 1024-frame 1080p batch has 8.5 GB of them; nothing is gained by keeping more than a chip-filling group in flight). A block
// takes at most a quarter of the scratch cache (512 MiB by default), so both stay cached from call to call beside whatever else lives there.
int run_steps(const void *src_frames, uint32_t n_frames, const std::vector<Shape> &shape, const zg_step *steps, void *dst_frames, hipStream_t s) {
    const uint32_t n_steps = (uint32_t)shape.size() - 1;
    if (n_steps == 0) {
        ZG_HIP(hipMemcpyAsync(dst_frames, src_frames, (size_t)n_frames * shape[0].frame_bytes(), hipMemcpyDeviceToDevice, s));
        return ZG_OK;
    }
    if (n_steps == 2) { // a recipe that is one fused pair has no intermediates: no scratch and no groups, one launch over the batch
        const zg_image a = shape[0].at((void *)src_frames), b = shape[2].at(dst_frames);
        const int rc = run_fused_pair(steps[0], steps[1], FrameBatch{&a, &b, n_frames, shape[0].frame_bytes(), shape[2].frame_bytes()}, shape[0].space, s);
        if (rc >= 0) return rc;
    }
    size_t widest = 0; // bytes per frame of the largest intermediate
    for (uint32_t i = 1; i < n_steps; ++i) widest = std::max(widest, shape[i].frame_bytes());
    const size_t budget = std::min<size_t>((size_t)1 << 30, scratch_block_budget());
    const uint32_t group = widest ? (uint32_t)std::max<size_t>(1, std::min<size_t>(n_frames, budget / widest)) : n_frames;
    ScratchBlock ping[2]{ScratchBlock(s), ScratchBlock(s)};
    int rc = ZG_OK;
    if (widest) {
        if ((rc = ping[0].alloc((size_t)group * widest))) return rc;
        if (n_steps > 2 && (rc = ping[1].alloc((size_t)group * widest))) return rc;
    }
    for (uint32_t g0 = 0; g0 < n_frames && rc == ZG_OK; g0 += group) {
        const uint32_t gn = std::min(group, n_frames - g0);
        void *cur = (char *)src_frames + (size_t)g0 * shape[0].frame_bytes();
        int flip = 0;
        for (uint32_t i = 0; i < n_steps && rc == ZG_OK;) {
            // steps [i, i + take) from `cur` into the caller's frames when they are the last, into a scratch block otherwise
            auto run = [&](uint32_t take) {
                const uint32_t o = i + take;
                void *next = o == n_steps ? (void *)((char *)dst_frames + (size_t)g0 * shape[o].frame_bytes()) : (void *)ping[flip].p;
                const zg_image a = shape[i].at(cur), b = shape[o].at(next);
                const FrameBatch fb{&a, &b, gn, shape[i].frame_bytes(), shape[o].frame_bytes()};
                const int r = take == 2 ? run_fused_pair(steps[i], steps[i + 1], fb, shape[i].space, s) : run_step(steps[i], fb, shape[i].space, shape[o].space, s);
                if (r < 0) return r; // a pair that does not fuse
                cur = next;
                if (o != n_steps) flip ^= 1;
                i = o;
                return r;
            };
            rc = n_steps > 2 && i + 1 < n_steps ? run(2) : -1; // the step together with its successor (a two-step recipe's pair was tried above), then alone
            if (rc < 0) rc = run(1);
        }
    }
    ping[0].reset(); // the first block first (an array's destructors run from its end): the order of frees decides which block a captured graph reuses
    return rc;
}

// the shapes after every step: validates all steps before anything is enqueued, like the CLI validates its recipe first (pipeline.zig:108-114)
int shapes_of(const Shape &first, const zg_step *steps, uint32_t n_steps, std::vector<Shape> &shape) {
    shape.assign(1, first);
    for (uint32_t i = 0; i < n_steps; ++i) {
        shape.push_back(shape.back());
        if (const int rc = apply_shape(steps[i], shape.back())) return rc;
    }
    return ZG_OK;
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

size_t zg_sizeof_step(void) { return sizeof(zg_step); }

int zg_batch_pipeline_shape(uint32_t rows, uint32_t cols, int pixel, int space, const zg_step *steps, uint32_t n_steps, uint32_t *out_rows, uint32_t *out_cols,
                            int *out_pixel, int *out_space) {
    ZG_REQUIRE(pixel_valid(pixel), ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid pixel type %d", pixel);
    ZG_REQUIRE(n_steps == 0 || steps != nullptr, ZG_ERR_INVALID_ARGUMENT, "pipeline: null steps");
    std::vector<Shape> shape;
    if (const int rc = shapes_of(Shape{rows, cols, pixel, space}, steps, n_steps, shape)) return rc;
    if (out_rows) *out_rows = shape.back().rows;
    if (out_cols) *out_cols = shape.back().cols;
    if (out_pixel) *out_pixel = shape.back().pixel;
    if (out_space) *out_space = shape.back().space;
    return ZG_OK;
}

int zg_batch_pipeline(const void *src_frames, uint32_t n_frames, uint32_t rows, uint32_t cols, int pixel, int space, const zg_step *steps, uint32_t n_steps,
                      void *dst_frames, zg_stream stream) {
    ZG_REQUIRE(pixel_valid(pixel), ZG_ERR_INVALID_ARGUMENT, "pipeline: invalid pixel type %d", pixel);
    ZG_REQUIRE(n_steps == 0 || steps != nullptr, ZG_ERR_INVALID_ARGUMENT, "pipeline: null steps");
    hipStream_t s = as_stream(stream);
    for (uint32_t i = 0; i < n_steps; ++i) // a step with a caller's table would upload it after earlier steps were enqueued: refused up front
        if ((steps[i].srgb_lut || steps[i].method.lanczos_lut) && refuse_under_capture(s, "zg_batch_pipeline with a caller's sRGB or Lanczos table in a step"))
            return ZG_ERR_UNSUPPORTED;
    std::vector<Shape> shape;
    if (const int rc = shapes_of(Shape{rows, cols, pixel, space}, steps, n_steps, shape)) return rc;
    if (n_frames == 0 || rows == 0 || cols == 0) return ZG_OK;
    ZG_REQUIRE(src_frames && dst_frames, ZG_ERR_INVALID_ARGUMENT, "pipeline: null frame pointer");
    for (const Shape &f : shape) ZG_REQUIRE(f.rows > 0 && f.cols > 0, ZG_ERR_INVALID_ARGUMENT, "pipeline: a step produces empty frames");
    return run_steps(src_frames, n_frames, shape, steps, dst_frames, s);
}

int zg_batch_blur_resize(const void *src_frames, uint32_t n_frames, uint32_t rows, uint32_t cols, int pixel, float sigma,
                         void *dst_frames, uint32_t out_rows, uint32_t out_cols, const zg_method *method, zg_stream stream) {
    ZG_REQUIRE(pixel_valid(pixel), ZG_ERR_INVALID_ARGUMENT, "batch: invalid pixel type %d", pixel);
    ZG_REQUIRE(method != nullptr, ZG_ERR_INVALID_ARGUMENT, "batch: null method");
    ZG_REQUIRE(sigma >= 0, ZG_ERR_INVALID_ARGUMENT, "batch: InvalidSigma (%g)", sigma);
    if (n_frames == 0 || rows == 0 || cols == 0 || out_rows == 0 || out_cols == 0) return ZG_OK;
    ZG_REQUIRE(src_frames && dst_frames, ZG_ERR_INVALID_ARGUMENT, "batch: null frame pointer");
    zg_step steps[2] = {};
    steps[0].kind = ZG_STEP_GAUSSIAN_BLUR;
    steps[0].sigma = sigma;
    steps[1].kind = ZG_STEP_RESIZE;
    steps[1].out_rows = out_rows;
    steps[1].out_cols = out_cols;
    steps[1].method = *method;
    std::vector<Shape> shape;
    if (const int rc = shapes_of(Shape{rows, cols, pixel, ZG_CS_RGBA}, steps, 2, shape)) return rc; // the colour space: neither step reads it
    return run_steps(src_frames, n_frames, shape, steps, dst_frames, as_stream(stream));
}

} // extern "C"

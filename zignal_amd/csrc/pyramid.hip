// pyramid.hip — ImagePyramid.build's host side (reference src/image/pyramid.zig:31-102): the per-level arithmetic, one level, and the
// whole build over forked streams. The kernels are elsewhere: conv_sep_bytes2.hip (try_pyramid_level_u8, try_pyramid_levels_u8: they
// share their row pass with the two-pass u8 blur) and pyramid_tile.hip (try_pyramid_tiles_u8).
#include "zg_internal.h"
#include "zg_hostmath.h"

#include <cmath>
#include <map>
#include <vector>

namespace zg {

int resize_impl_bilinear_u8(const zg_image *src, const zg_image *dst, hipStream_t s) {
    const zg_method bilinear{ZG_INTERP_BILINEAR, 0.0f, 0.0f, nullptr};
    return zg_resize(src, dst, &bilinear, (zg_stream)s);
}

namespace {

struct LevelStreams {
    hipStream_t s[3] = {nullptr, nullptr, nullptr};
};
// The helper streams the levels fork over: per thread (a stream can sit in one capture at a time, so two threads recording pyramids must not
// share them) and per device, created the first time a build on that device wants to fork, destroyed when the thread ends. A stream that
// cannot be created leaves its lane out (the build then forks over fewer lanes, or not at all): forking is an optimisation.
struct LevelStreamPool {
    std::map<int, LevelStreams> by_device;
    ~LevelStreamPool() {
        for (auto &kv : by_device)
            for (hipStream_t st : kv.second.s)
                if (st) (void)hipStreamDestroy(st);
    }
};
LevelStreams &level_streams() {
    static thread_local LevelStreamPool pool;
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto it = pool.by_device.find(dev);
    if (it == pool.by_device.end()) {
        it = pool.by_device.emplace(dev, LevelStreams{}).first;
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed; // creating a stream is an "unsafe" call while a capture is in progress
        const bool swapped = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
        for (hipStream_t &st : it->second.s)
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); st = nullptr; }
        if (swapped) (void)hipThreadExchangeStreamCaptureMode(&mode);
    }
    return it->second;
}

} // namespace
} // namespace zg

using namespace zg;

extern "C" {

// ImagePyramid.build's per-level arithmetic (src/image/pyramid.zig:57-80). `scale` is pow(scale_factor, level) as the
// CALLER's maths library computes it (a Zig host passes std.math.pow's value); zg_pyramid_scale is the library's own.
float zg_pyramid_scale(float scale_factor, uint32_t level) { return hostmath::pow_f32(scale_factor, (float)level); }

int zg_pyramid_level(uint32_t rows, uint32_t cols, float scale, float blur_sigma, uint32_t *out_rows, uint32_t *out_cols, float *out_sigma) {
    ZG_REQUIRE(out_rows && out_cols && out_sigma, ZG_ERR_INVALID_ARGUMENT, "pyramid level: null output");
    ZG_REQUIRE(scale > 0, ZG_ERR_INVALID_ARGUMENT, "pyramid level: scale must be positive");
    uint32_t nr = (uint32_t)std::trunc((float)rows / scale), nc = (uint32_t)std::trunc((float)cols / scale);
    *out_rows = nr < 1 ? 1 : nr;
    *out_cols = nc < 1 ? 1 : nc;
    *out_sigma = blur_sigma * std::sqrt(scale * scale - 1.0f);
    return ZG_OK;
}

// One level of ImagePyramid.build (pyramid.zig:76-92) in a single call: blur the ORIGINAL with `sigma` when sigma > 0.5
// (library scratch holds the blurred copy), then bilinear resize into `level`. `sigma` is zg_pyramid_level's output.
int zg_pyramid_build_level(const zg_image *source, const zg_image *level, float sigma, zg_stream stream) {
    int rc;
    if ((rc = check_image(source, "source")) || (rc = check_image(level, "level"))) return rc;
    ZG_REQUIRE(source->pixel == level->pixel, ZG_ERR_INVALID_ARGUMENT, "pyramid level: pixel types differ");
    const zg_method bilinear{ZG_INTERP_BILINEAR, 0.0f, 0.0f, nullptr};
    if (!(sigma > 0.5f) || source->rows == 0 || source->cols == 0) return zg_resize(source, level, &bilinear, stream);
    hipStream_t s = as_stream(stream);
    if (source->pixel == ZG_PIXEL_U8 && sigma > 0) { // Image(u8), what ORB builds its pyramid on: the column pass evaluated where the resize looks (conv_sep_bytes2.hip)
        int32_t itaps[65];
        GaussianTapsI32 t;
        if (gaussian_taps_i32(sigma, itaps, 65, t) == ZG_OK && t.n <= 65) {
            const int rcf = try_pyramid_level_u8(source, level, itaps + t.z, t.n - 2 * t.z, s);
            if (rcf >= 0) return rcf;
        }
    }
    ScratchBlock blurred(s);
    if ((rc = blurred.alloc((size_t)source->rows * source->cols * pixel_size(source->pixel)))) return rc;
    const zg_image tmp{blurred.p, source->cols, source->rows, source->cols, source->pixel};
    if ((rc = zg_gaussian_blur(source, &tmp, sigma, stream))) return rc;
    return zg_resize(&tmp, level, &bilinear, stream);
}

// ImagePyramid.build (pyramid.zig:31-102) as one device operation: every level is made from the ORIGINAL (blur with its own sigma, then
// bilinear resize), so the levels are independent of each other — they are enqueued on a few internal streams forked from `stream`
// and joined back into it (events; no host synchronisation, and the fork / join is what stream capture expects, so the whole build
// records into a graph). levels[i] / sigmas[i] are pyramid level i + 1: shapes from zg_pyramid_level, memory from the caller.
int zg_pyramid_build(const zg_image *source, const zg_image *levels, const float *sigmas, uint32_t n_levels, zg_stream stream) {
    ZG_REQUIRE(source && (n_levels == 0 || (levels && sigmas)), ZG_ERR_INVALID_ARGUMENT, "pyramid build: null argument");
    if (n_levels == 0) return ZG_OK;
    hipStream_t main = as_stream(stream);
    // Forking pays when the device is the bottleneck — a graph replay: 445 us on one stream, 351 us on four for ORB's default pyramid of
    // a 4096^2 plane — and costs when the host is (eager launches: 508 us on one stream, 661 us on four: every cross-stream hand-off
    // is host work). So the levels fork under stream capture and stay on `stream` otherwise.
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(main, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
    int want = capturing == hipStreamCaptureStatusActive ? 4 : 1;
    if (n_levels < (uint32_t)want) want = (int)n_levels;
    hipStream_t lanes[4] = {main, nullptr, nullptr, nullptr};
    int n_lanes = 1;
    if (want > 1) { // the pool is only touched (and its streams only created) by a build that forks
        const LevelStreams &pool = level_streams();
        for (int i = 1; i < want && pool.s[i - 1]; ++i) { lanes[i] = pool.s[i - 1]; n_lanes = i + 1; }
    }
    hipEvent_t fork = nullptr, join[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = ZG_OK;
    auto hip = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == ZG_OK) rc = hip_fail(e, what, __FILE__, __LINE__);
    };
    if (n_lanes > 1) {
        hip(hipEventCreateWithFlags(&fork, hipEventDisableTiming), "hipEventCreateWithFlags");
        if (rc == ZG_OK) hip(hipEventRecord(fork, main), "hipEventRecord");
        for (int l = 1; l < n_lanes && rc == ZG_OK; ++l) hip(hipStreamWaitEvent(lanes[l], fork, 0), "hipStreamWaitEvent");
    }
    // Image(u8): the long-tap levels as one batch on the last lane (three launches + the resizes of the dense levels), the rest level by level
    std::vector<uint8_t> handled(n_levels, 0);
    if (rc == ZG_OK && n_levels <= 64 && check_image(source, "source") == ZG_OK) {
        bool all_ok = true;
        for (uint32_t i = 0; i < n_levels; ++i) all_ok = all_ok && check_image(&levels[i], "level") == ZG_OK && levels[i].pixel == source->pixel;
        if (all_ok) {
            // round 6: every level whose taps fit (<= 35, each <= 255) as one tile kernel with no plane in between (pyramid_tile.hip); what it leaves goes on as before
            const int rct = try_pyramid_tiles_u8(source, levels, sigmas, n_levels, handled.data(), lanes[n_lanes - 1]);
            if (rct > 0) rc = rct;
        }
        if (all_ok && rc == ZG_OK) {
            if (n_lanes >= 3) { // two independent batches on two lanes: levels reduced by 2 and more (fused column pass), and the others (dense + resize)
                const int rcf = try_pyramid_levels_u8(source, levels, sigmas, n_levels, handled.data(), 0, lanes[n_lanes - 1]);
                const int rcd = try_pyramid_levels_u8(source, levels, sigmas, n_levels, handled.data(), 1, lanes[n_lanes - 2]);
                if (rcf > 0) rc = rcf; else if (rcd > 0) rc = rcd;
            } else {
                const int rcb = try_pyramid_levels_u8(source, levels, sigmas, n_levels, handled.data(), 2, lanes[n_lanes - 1]);
                if (rcb > 0) rc = rcb;
            }
        }
    }
    // the largest levels (the longest kernels) first, dealt round the lanes
    uint32_t dealt = 0;
    for (uint32_t i = 0; i < n_levels && rc == ZG_OK; ++i) {
        if (handled[i]) continue;
        rc = zg_pyramid_build_level(source, &levels[i], sigmas[i], (zg_stream)lanes[dealt++ % (uint32_t)n_lanes]);
    }
    for (int l = 1; l < n_lanes; ++l) { // always joined, also after a failure: a forked stream must not be left inside a capture
        if (hipEventCreateWithFlags(&join[l], hipEventDisableTiming) == hipSuccess && hipEventRecord(join[l], lanes[l]) == hipSuccess)
            hip(hipStreamWaitEvent(main, join[l], 0), "hipStreamWaitEvent");
        else
            hip(hipGetLastError(), "pyramid build: join");
    }
    if (fork) (void)hipEventDestroy(fork);
    for (hipEvent_t e : join)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

} // extern "C"

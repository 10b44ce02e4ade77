//! zignal_hip_metrics.zig — the image-metrics module of the shim: Image(T).psnr, ssim and meanPixelError (reference
//! src/image/metrics.zig) through libzignal_hip.so's entry points (include/zignal_hip_metrics.h). Like the other files of the shim it
//! has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub const ZgMetricResult = extern struct { sum: f64 = 0, count: u64 = 0, value: f64 = 0, serial_terms: u64 = 0 };
    pub const ZgMetricOptions = extern struct { ssim_window: ?[*]const f64 = null, ssim_map: ?[*]f64 = null };
    pub extern fn zg_sum_f64_chunk() u32;
    pub extern fn zg_ssim_window_host(w: *[121]f64) c_int;
    pub extern fn zg_psnr_from_mse(mse: f64, max_value: f64) f64;
    pub extern fn zg_exp_f64_host(x: f64) f64;
    pub extern fn zg_log10_f64_host(x: f64) f64;
    pub extern fn zg_sum_f64_sequential(values: ?[*]const f64, n: u64, chunk_log2: u32, result: *ZgMetricResult, stream: ?*anyopaque) c_int;
    pub extern fn zg_psnr(a: *const hip.c.ZgImage, b: *const hip.c.ZgImage, opt: ?*const ZgMetricOptions, result: *ZgMetricResult, stream: ?*anyopaque) c_int;
    pub extern fn zg_mean_pixel_error(a: *const hip.c.ZgImage, b: *const hip.c.ZgImage, opt: ?*const ZgMetricOptions, result: *ZgMetricResult, stream: ?*anyopaque) c_int;
    pub extern fn zg_ssim(a: *const hip.c.ZgImage, b: *const hip.c.ZgImage, opt: ?*const ZgMetricOptions, result: *ZgMetricResult, stream: ?*anyopaque) c_int;
    pub extern fn zg_psnr_host(a: *const hip.c.ZgImage, b: *const hip.c.ZgImage, opt: ?*const ZgMetricOptions, value: *f64, result: ?*ZgMetricResult) c_int;
    pub extern fn zg_mean_pixel_error_host(a: *const hip.c.ZgImage, b: *const hip.c.ZgImage, opt: ?*const ZgMetricOptions, value: *f64, result: ?*ZgMetricResult) c_int;
    pub extern fn zg_ssim_host(a: *const hip.c.ZgImage, b: *const hip.c.ZgImage, opt: ?*const ZgMetricOptions, value: *f64, result: ?*ZgMetricResult) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgMetricResult) == 32);
    std.debug.assert(@sizeOf(c.ZgMetricOptions) == 16);
}

/// ZG_PIXEL_* of a pixel type the library measures: u8, f32, Rgb / Rgba of u8 and of f32.
fn pixelOf(comptime T: type) c_int {
    return switch (T) {
        u8 => 0,
        f32 => 1,
        zignal.Rgb(u8) => 2,
        zignal.Rgba(u8) => 3,
        zignal.Rgb(f32) => 4,
        zignal.Rgba(f32) => 5,
        else => @compileError("metrics on the device: unsupported pixel type " ++ @typeName(T)),
    };
}

fn desc(comptime T: type, img: zignal.Image(T)) hip.c.ZgImage {
    return .{ .data = @ptrCast(img.data.ptr), .stride = img.stride, .rows = img.rows, .cols = img.cols, .pixel = pixelOf(T) };
}

fn maxValue(comptime T: type) f64 {
    return switch (T) {
        u8, zignal.Rgb(u8), zignal.Rgba(u8) => 255.0,
        else => 1.0,
    };
}

/// generateSsimWindow (metrics.zig:230-249) evaluated by this compiler, so that the device sees Zig's own weights.
const ssim_window: [121]f64 = blk: {
    @setEvalBranchQuota(10000);
    var w: [121]f64 = undefined;
    var sum: f64 = 0.0;
    for (0..11) |dy| {
        for (0..11) |dx| {
            const y: f64 = @as(f64, @floatFromInt(dy)) - 5.0;
            const x: f64 = @as(f64, @floatFromInt(dx)) - 5.0;
            const g = @exp(-(x * x + y * y) / (2.0 * 1.5 * 1.5));
            w[dy * 11 + dx] = g;
            sum += g;
        }
    }
    for (&w) |*v| v.* /= sum;
    break :blk w;
};

/// Drop-in for Image(T).psnr on host images (metrics.zig:10-54): the mse comes from the device, the logarithms are Zig's.
pub fn psnr(comptime T: type, image_a: zignal.Image(T), image_b: zignal.Image(T)) !f64 {
    if (image_a.rows != image_b.rows or image_a.cols != image_b.cols) return error.DimensionMismatch;
    var value: f64 = 0;
    var res: c.ZgMetricResult = .{};
    try hip.check(c.zg_psnr_host(&desc(T, image_a), &desc(T, image_b), null, &value, &res));
    if (res.value == 0.0) return std.math.inf(f64);
    return 20.0 * std.math.log10(maxValue(T)) - 10.0 * std.math.log10(res.value);
}

/// Drop-in for Image(T).meanPixelError on host images (metrics.zig:114-166).
pub fn meanPixelError(comptime T: type, image_a: zignal.Image(T), image_b: zignal.Image(T)) !f64 {
    if (image_a.rows != image_b.rows or image_a.cols != image_b.cols) return error.DimensionMismatch;
    var value: f64 = 0;
    try hip.check(c.zg_mean_pixel_error_host(&desc(T, image_a), &desc(T, image_b), null, &value, null));
    return value;
}

/// Drop-in for Image(T).ssim on host images (metrics.zig:56-112), with this compiler's window.
pub fn ssim(comptime T: type, image_a: zignal.Image(T), image_b: zignal.Image(T)) !f64 {
    if (image_a.rows != image_b.rows or image_a.cols != image_b.cols) return error.DimensionMismatch;
    if (image_a.rows < 11 or image_a.cols < 11) return error.ImageTooSmall;
    var value: f64 = 0;
    const opt: c.ZgMetricOptions = .{ .ssim_window = &ssim_window };
    try hip.check(c.zg_ssim_host(&desc(T, image_a), &desc(T, image_b), &opt, &value, null));
    return value;
}

/// The device forms: asynchronous on `stream`, capturable into a graph; the images' data, opts.ssim_map and `result` are device memory
/// from zg_malloc. result.value is the mse for `.psnr` and the method's value for the other two.
pub const Metric = enum { psnr, mean_pixel_error, ssim };
pub fn metricInto(metric: Metric, a: hip.c.ZgImage, b: hip.c.ZgImage, map: ?[*]f64, result: *c.ZgMetricResult, stream: ?*anyopaque) !void {
    const opt: c.ZgMetricOptions = .{ .ssim_window = &ssim_window, .ssim_map = map };
    try hip.check(switch (metric) {
        .psnr => c.zg_psnr(&a, &b, &opt, result, stream),
        .mean_pixel_error => c.zg_mean_pixel_error(&a, &b, &opt, result, stream),
        .ssim => c.zg_ssim(&a, &b, &opt, result, stream),
    });
}

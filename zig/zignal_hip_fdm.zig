//! zignal_hip_fdm.zig — the feature-distribution-matching module of the shim: FeatureDistributionMatching(T) (reference src/fdm.zig)
//! through libzignal_hip.so's entry points (include/zignal_hip_fdm.h). The device takes its statistics from exact integer moments, not
//! from CovarianceStats' Welford recurrence: a byte can differ from the reference's where its value before @round is within about 1e-12
//! of a tie. A caller who needs the reference's bytes runs CovarianceStats itself and goes through targetFromStats / transformFromStats
//! and zg_fdm_apply. Like the other files of the shim it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub const ZgFdmMoments = extern struct {
        n: u64 = 0,
        sum: [3]u64 = @splat(0),
        prod: [6]u64 = @splat(0),
        lum_sum: u64 = 0,
        lum_sq: u64 = 0,
        not_gray: u32 = 0,
        pixel: i32 = 0,
    };
    pub const ZgFdmTarget = extern struct {
        mean: [3]f64 = @splat(0),
        u: [9]f64 = @splat(0),
        s: [3]f64 = @splat(0),
        is_gray: i32 = 0,
        status: i32 = 0,
        pixel: i32 = 0,
        reserved: i32 = 0,
    };
    pub const ZgFdmTransform = extern struct {
        route: i32 = 0,
        status: i32 = 0,
        w: [9]f64 = @splat(0),
        bias: [3]f64 = @splat(0),
        scale: f64 = 1,
        offset: f64 = 0,
    };
    pub extern fn zg_fdm_sizeof_moments() usize;
    pub extern fn zg_fdm_sizeof_target() usize;
    pub extern fn zg_fdm_sizeof_transform() usize;
    pub extern fn zg_fdm_lane_run() u32;
    pub extern fn zg_fdm_frames_per_launch() u32;
    pub extern fn zg_fdm_compute_moments(img: *const hip.c.ZgImage, moments_dev: *ZgFdmMoments, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_compute_moments_frames(frames: ?[*]const hip.c.ZgImage, n: u32, moments_dev: ?[*]ZgFdmMoments, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_target_from_moments(moments_dev: *const ZgFdmMoments, target_dev: *ZgFdmTarget, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_transform_from_moments(moments_dev: *const ZgFdmMoments, pixel: c_int, target_dev: *const ZgFdmTarget, transform_dev: *ZgFdmTransform, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_transform_from_moments_frames(moments_dev: ?[*]const ZgFdmMoments, n: u32, target_dev: ?*const ZgFdmTarget, transforms_dev: ?[*]ZgFdmTransform, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_target_host(pixel: c_int, mean: *const [3]f64, cov: *const [9]f64, is_gray: c_int, out: *ZgFdmTarget) c_int;
    pub extern fn zg_fdm_transform_host(pixel: c_int, target: *const ZgFdmTarget, mean: *const [3]f64, cov: *const [9]f64, out: *ZgFdmTransform) c_int;
    pub extern fn zg_fdm_stats_from_moments_host(moments: *const ZgFdmMoments, luminance: c_int, mean: *[3]f64, cov: *[9]f64) c_int;
    pub extern fn zg_fdm_apply(img: *const hip.c.ZgImage, transform_dev: *const ZgFdmTransform, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_apply_frames(frames: ?[*]const hip.c.ZgImage, n: u32, transforms_dev: ?[*]const ZgFdmTransform, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_match(src: *const hip.c.ZgImage, target: *const hip.c.ZgImage, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_match_frames(frames: ?[*]const hip.c.ZgImage, n: u32, target: ?*const hip.c.ZgImage, prepared_dev: ?*const ZgFdmTarget, stream: ?*anyopaque) c_int;
    pub extern fn zg_fdm_match_host(src: *const hip.c.ZgImage, target: *const hip.c.ZgImage) c_int;
    pub extern fn zg_fdm_match_frames_host(frames: ?[*]const hip.c.ZgImage, n: u32, target: *const hip.c.ZgImage) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgFdmMoments) == 104);
    std.debug.assert(@sizeOf(c.ZgFdmTarget) == 136);
    std.debug.assert(@sizeOf(c.ZgFdmTransform) == 120);
}

fn pixelOf(comptime T: type) c_int {
    return switch (T) {
        u8 => 0,
        zignal.Rgb(u8) => 2,
        zignal.Rgba(u8) => 3,
        else => @compileError("feature distribution matching takes u8, Rgb(u8) and Rgba(u8), got " ++ @typeName(T)),
    };
}

fn desc(comptime T: type, img: zignal.Image(T)) hip.c.ZgImage {
    return .{ .data = @ptrCast(img.data.ptr), .stride = img.stride, .rows = img.rows, .cols = img.cols, .pixel = pixelOf(T) };
}

/// Drop-in for FeatureDistributionMatching(T) on host images: the same state machine, the work on the device.
pub fn FeatureDistributionMatching(comptime T: type) type {
    return struct {
        const Self = @This();
        target_image: ?zignal.Image(T) = null,
        source_image: ?zignal.Image(T) = null,

        pub fn init() Self {
            return .{};
        }
        pub fn setTarget(self: *Self, target_image: zignal.Image(T)) !void {
            self.target_image = target_image;
        }
        pub fn setSource(self: *Self, source_image: zignal.Image(T)) !void {
            self.source_image = source_image;
        }
        pub fn update(self: *Self) !void {
            const target = self.target_image orelse return error.NoTargetSet;
            const source = self.source_image orelse return error.NoSourceSet;
            try hip.check(c.zg_fdm_match_host(&desc(T, source), &desc(T, target)));
        }
        pub fn match(self: *Self, source_image: zignal.Image(T), target_image: zignal.Image(T)) !void {
            try self.setTarget(target_image);
            try self.setSource(source_image);
            try self.update();
        }
        /// every frame against the target set before, in one chain
        pub fn updateFrames(self: *Self, allocator: std.mem.Allocator, frames: []const zignal.Image(T)) !void {
            const target = self.target_image orelse return error.NoTargetSet;
            const descs = try allocator.alloc(hip.c.ZgImage, frames.len);
            defer allocator.free(descs);
            for (frames, descs) |f, *d| d.* = desc(T, f);
            try hip.check(c.zg_fdm_match_frames_host(descs.ptr, @intCast(frames.len), &desc(T, target)));
        }
    };
}

/// setTarget and update between the caller's own statistics (CovarianceStats' mean and covariance, row-major) and the pixels: host
/// arithmetic, the reference's bit for bit. Upload the transform and run zg_fdm_apply for the reference's bytes.
pub fn targetFromStats(comptime T: type, mean: [3]f64, cov: [9]f64, is_gray: bool) !c.ZgFdmTarget {
    var out: c.ZgFdmTarget = .{};
    try hip.check(c.zg_fdm_target_host(pixelOf(T), &mean, &cov, @intFromBool(is_gray), &out));
    return out;
}
pub fn transformFromStats(comptime T: type, target: c.ZgFdmTarget, mean: [3]f64, cov: [9]f64) !c.ZgFdmTransform {
    var out: c.ZgFdmTransform = .{};
    try hip.check(c.zg_fdm_transform_host(pixelOf(T), &target, &mean, &cov, &out));
    return out;
}

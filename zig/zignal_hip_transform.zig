//! zignal_hip_transform.zig — the geometry-fitting module of the shim: SimilarityTransform.find, AffineTransform.find and
//! ProjectiveTransform.find (reference src/geometry/transforms.zig) through libzignal_hip.so's entry points
//! (include/zignal_hip_transform.h). The host forms run the reference's arithmetic on the CPU bit for bit, except AffineTransform.find on
//! 86 or more points, where the reference's own value depends on its build's vector width and the library keeps the scalar chain. Like the
//! other files of the shim it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub const ZgTransformFit = extern struct {
        kind: i32 = 0,
        status: i32 = 0,
        n_points: u32 = 0,
        svd_converged: u32 = 0,
        m64: [9]f64 = @splat(0),
        m32: [9]f32 = @splat(0),
        reserved: u32 = 0,
    };
    pub extern fn zg_transform_sizeof_fit() usize;
    pub extern fn zg_transform_chunk() u32;
    pub extern fn zg_transform_fit_points(kind: c_int, scalar: c_int, from: ?*const anyopaque, to: ?*const anyopaque, capacity: u32, count: ?*const u32, out: *ZgTransformFit, stream: ?*anyopaque) c_int;
    pub extern fn zg_transform_fit_matches(kind: c_int, scalar: c_int, query_kps: ?*const anyopaque, n_query: u32, train_kps: ?*const anyopaque, n_train: u32, matches: ?*const anyopaque, capacity: u32, count: ?*const u32, train_to_query: c_int, out: *ZgTransformFit, stream: ?*anyopaque) c_int;
    pub extern fn zg_transform_fit_points_host(kind: c_int, scalar: c_int, from: ?*const anyopaque, to: ?*const anyopaque, capacity: u32, count: ?*const u32, out: *ZgTransformFit) c_int;
    pub extern fn zg_transform_fit_matches_host(kind: c_int, scalar: c_int, query_kps: ?*const anyopaque, n_query: u32, train_kps: ?*const anyopaque, n_train: u32, matches: ?*const anyopaque, capacity: u32, count: ?*const u32, train_to_query: c_int, out: *ZgTransformFit) c_int;
    pub extern fn zg_transform_project_points(fit: *const ZgTransformFit, scalar: c_int, in: ?*const anyopaque, out: ?*anyopaque, n: u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_transform_project_points_host(fit: *const ZgTransformFit, scalar: c_int, in: ?*const anyopaque, out: ?*anyopaque, n: u32) c_int;
    pub extern fn zg_transform_invert(fit: *const ZgTransformFit, scalar: c_int, out: *ZgTransformFit, stream: ?*anyopaque) c_int;
    pub extern fn zg_transform_invert_host(fit: *const ZgTransformFit, scalar: c_int, out: *ZgTransformFit) c_int;
    pub extern fn zg_warp_fitted(src: *const hip.c.ZgImage, dst: *const hip.c.ZgImage, fit_dev: *const ZgTransformFit, method: *const hip.c.ZgMethod, stream: ?*anyopaque) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgTransformFit) == 128);
}

pub const Kind = enum(c_int) { similarity = 0, affine = 1, projective = 2 };
pub const FitError = error{ NotConverged, RankDeficient, BadCount, BadInput };

fn scalarOf(comptime T: type) c_int {
    return switch (T) {
        f32 => 0,
        f64 => 1,
        else => @compileError("a fit runs in f32 or f64, got " ++ @typeName(T)),
    };
}

fn checkStatus(status: i32) FitError!void {
    return switch (status) {
        0 => {},
        1 => error.NotConverged,
        2 => error.RankDeficient,
        3 => error.BadCount,
        else => error.BadInput,
    };
}

/// find for `kind` on host points (Point(2, T) is two T): the record, or the reference's error.
pub fn fit(comptime T: type, kind: Kind, from_points: []const zignal.Point(2, T), to_points: []const zignal.Point(2, T)) !c.ZgTransformFit {
    std.debug.assert(from_points.len == to_points.len);
    var out: c.ZgTransformFit = .{};
    try hip.check(c.zg_transform_fit_points_host(@intFromEnum(kind), scalarOf(T), from_points.ptr, to_points.ptr, @intCast(from_points.len), null, &out));
    try checkStatus(out.status);
    return out;
}

fn coefficients(comptime T: type, record: c.ZgTransformFit) [9]T {
    var m: [9]T = undefined;
    for (0..9) |i| m[i] = if (T == f32) record.m32[i] else record.m64[i];
    return m;
}

/// Drop-ins for the three init functions: the reference's types, filled from the record.
pub fn similarity(comptime T: type, from_points: []const zignal.Point(2, T), to_points: []const zignal.Point(2, T)) !zignal.SimilarityTransform(T) {
    const m = coefficients(T, try fit(T, .similarity, from_points, to_points));
    return .{ .matrix = .init(.{ .{ m[0], m[1] }, .{ m[2], m[3] } }), .bias = .init(.{ .{m[4]}, .{m[5]} }) };
}
pub fn affine(comptime T: type, from_points: []const zignal.Point(2, T), to_points: []const zignal.Point(2, T)) !zignal.AffineTransform(T) {
    const m = coefficients(T, try fit(T, .affine, from_points, to_points));
    return .{ .matrix = .init(.{ .{ m[0], m[1] }, .{ m[2], m[3] } }), .bias = .init(.{ .{m[4]}, .{m[5]} }) };
}
pub fn projective(comptime T: type, from_points: []const zignal.Point(2, T), to_points: []const zignal.Point(2, T)) !zignal.ProjectiveTransform(T) {
    const m = coefficients(T, try fit(T, .projective, from_points, to_points));
    return .{ .matrix = .init(.{ .{ m[0], m[1], m[2] }, .{ m[3], m[4], m[5] }, .{ m[6], m[7], m[8] } }) };
}

//! zignal_hip_tracer.zig — the Tracer module of the shim: Tracer.trace (reference src/features/Tracer.zig) through libzignal_hip.so's
//! zg_trace_paths* entry points, and the builder from paths to Canvas line commands (include/zignal_hip_tracer.h). Like the other files
//! of the shim it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");
const canvas = @import("zignal_hip_canvas.zig");

pub const c = struct {
    pub const ZgTracerOptions = extern struct { min_path_length: u32 = 5, simplification_epsilon: f32 = 1.0 }; // Tracer.zig:20-25
    pub extern fn zg_trace_scratch_bytes(rows: u32, cols: u32) usize;
    pub extern fn zg_trace_paths(edges: *const hip.c.ZgImage, opt: ?*const ZgTracerOptions, points: ?[*]f32, point_capacity: u32, path_offsets: [*]u32, path_capacity: u32, counts: *[4]u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_trace_paths_host(edges: *const hip.c.ZgImage, opt: ?*const ZgTracerOptions, points: ?[*]f32, point_capacity: u32, path_offsets: ?[*]u32, path_capacity: u32, counts: *[4]u32) c_int;
    pub extern fn zg_canvas_cmds_from_paths(points: ?[*]const f32, path_offsets: [*]const u32, counts: *const [4]u32, capacity: u32, color: *const [4]u8, width: u32, mode: c_int, cmds_out: ?[*]canvas.c.ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgTracerOptions) == 8);
}

const Point = zignal.Point(2, f32);
pub const Path = std.ArrayList(Point);
pub const PathList = std.ArrayList(Path);

fn desc(img: zignal.Image(u8)) hip.c.ZgImage {
    return .{ .data = @ptrCast(img.data.ptr), .stride = img.stride, .rows = img.rows, .cols = img.cols, .pixel = 0 };
}

/// Drop-in for Tracer.trace on a host edge map (Tracer.zig:46-80): the same paths in the same order with the same f32 bits. Two
/// synchronous calls: the counts first, then the lists. The caller owns the returned memory, as with the reference.
pub fn trace(tracer: zignal.Tracer, edges: zignal.Image(u8)) !PathList {
    const gpa = tracer.allocator;
    const o: c.ZgTracerOptions = .{ .min_path_length = @intCast(@min(tracer.min_path_length, std.math.maxInt(u32))), .simplification_epsilon = tracer.simplification_epsilon };
    var counts: [4]u32 = .{ 0, 0, 0, 0 };
    const d = desc(edges);
    try hip.check(c.zg_trace_paths_host(&d, &o, null, 0, null, 0, &counts));
    const points = try gpa.alloc(f32, 2 * @as(usize, counts[1]));
    defer gpa.free(points);
    const offsets = try gpa.alloc(u32, @as(usize, counts[0]) + 1);
    defer gpa.free(offsets);
    try hip.check(c.zg_trace_paths_host(&d, &o, if (points.len > 0) points.ptr else null, counts[1], offsets.ptr, counts[0], &counts));
    var paths: PathList = .empty;
    errdefer {
        for (paths.items) |*p| p.deinit(gpa);
        paths.deinit(gpa);
    }
    for (0..counts[2]) |i| {
        var path: Path = try .initCapacity(gpa, offsets[i + 1] - offsets[i]);
        for (offsets[i]..offsets[i + 1]) |j| path.appendAssumeCapacity(.init(.{ points[2 * j], points[2 * j + 1] }));
        try paths.append(gpa, path);
    }
    return paths;
}

/// The device form: asynchronous on `stream`, capturable into a graph; edges.data, points (point_capacity x, y pairs), path_offsets
/// (path_capacity + 1 words) and counts (four words) are device memory from zg_malloc.
pub fn traceInto(edges: hip.c.ZgImage, opts: c.ZgTracerOptions, points: ?[*]f32, point_capacity: u32, path_offsets: [*]u32, path_capacity: u32, counts: *[4]u32, stream: ?*anyopaque) !void {
    try hip.check(c.zg_trace_paths(&edges, &opts, points, point_capacity, path_offsets, path_capacity, counts, stream));
}

/// One ZG_DRAW_LINE per consecutive pair of points of every written path, built on the device (zg_canvas_cmds_from_paths).
pub fn cmdsFromPaths(points: ?[*]const f32, path_offsets: [*]const u32, counts: *const [4]u32, capacity: u32, color: [4]u8, width: u32, mode: c_int, cmds_out: ?[*]canvas.c.ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) !void {
    try hip.check(c.zg_canvas_cmds_from_paths(points, path_offsets, counts, capacity, &color, width, mode, cmds_out, count_out, stream));
}

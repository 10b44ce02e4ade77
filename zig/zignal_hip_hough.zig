//! zignal_hip_hough.zig — the Hough module of the shim: HoughTransform.init / compute / findLines (reference src/image/hough.zig)
//! through libzignal_hip.so's zg_hough_* entry points (include/zignal_hip_hough.h). The tables handed to the library are the ones
//! zignal's own HoughTransform.init made with Zig's @cos and @sin, so nothing of the library's restatement of them is on this path.
//! Like the other files of the shim it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub const ZgHoughLine = extern struct { angle: f32, radius: f32, score: u32, p1: [2]f32, p2: [2]f32 }; // hough.zig:13-25
    pub extern fn zg_hough_lds_max_size() u32;
    pub extern fn zg_hough_pixel_chunk() u32;
    pub extern fn zg_hough_tables_host(size: u32, cos_table: [*]i32, sin_table: [*]i32) c_int;
    pub extern fn zg_hough_create(size: u32, out: *?*anyopaque) c_int;
    pub extern fn zg_hough_create_with_tables(size: u32, cos_table: [*]const i32, sin_table: [*]const i32, out: *?*anyopaque) c_int;
    pub extern fn zg_hough_destroy(h: ?*anyopaque) c_int;
    pub extern fn zg_hough_size(h: ?*anyopaque) u32;
    pub extern fn zg_hough_compute(h: ?*anyopaque, edges: *const hip.c.ZgImage, l: u32, t: u32, r: u32, b: u32, accumulator: [*]u32, acc_stride: usize, stream: ?*anyopaque) c_int;
    pub extern fn zg_hough_find_lines(h: ?*anyopaque, accumulator: [*]const u32, acc_stride: usize, threshold: u32, threshold_device: ?*const u32, angle_nms_thresh: f32, radius_nms_thresh: f32, max_candidates: u32, lines: ?[*]ZgHoughLine, capacity: u32, counts: [*]u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_hough_compute_host(h: ?*anyopaque, edges: *const hip.c.ZgImage, l: u32, t: u32, r: u32, b: u32, accumulator: [*]u32, acc_stride: usize) c_int;
    pub extern fn zg_hough_find_lines_host(h: ?*anyopaque, accumulator: [*]const u32, acc_stride: usize, threshold: u32, angle_nms_thresh: f32, radius_nms_thresh: f32, max_candidates: u32, lines: ?[*]ZgHoughLine, capacity: u32, counts: [*]u32) c_int;
};

pub const max_size: u32 = 32768; // ZG_HOUGH_MAX_SIZE
pub const max_candidates_limit: u32 = 1 << 20; // ZG_HOUGH_MAX_CANDIDATES

comptime {
    std.debug.assert(@sizeOf(c.ZgHoughLine) == 28);
}

const Image = zignal.Image;
const Rectangle = zignal.Rectangle;
const Point = zignal.Point;

/// Drop-in for zignal.HoughTransform: same fields of Line, same calls, the work on the device.
pub const HoughTransform = struct {
    pub const Line = zignal.HoughTransform.Line;

    size: u32,
    even_size: u32,
    handle: ?*anyopaque,

    const Self = @This();

    /// hough.zig:38-66. zignal's init makes the tables (and checks the size); they are uploaded once, synchronously.
    pub fn init(allocator: std.mem.Allocator, size: u32) !Self {
        var own = try zignal.HoughTransform.init(allocator, size);
        defer own.deinit();
        var handle: ?*anyopaque = null;
        try hip.check(c.zg_hough_create_with_tables(size, own.cos_table.ptr, own.sin_table.ptr, &handle));
        return .{ .size = size, .even_size = own.even_size, .handle = handle };
    }

    pub fn deinit(self: *Self) void {
        _ = c.zg_hough_destroy(self.handle);
        self.handle = null;
    }

    fn desc(img: Image(u8)) hip.c.ZgImage {
        return .{ .data = @ptrCast(img.data.ptr), .stride = img.stride, .rows = img.rows, .cols = img.cols, .pixel = 0 }; // ZG_PIXEL_U8
    }

    /// hough.zig:75-139 on host images: the votes are added to `accumulator`.
    pub fn compute(self: Self, edges: Image(u8), box: Rectangle(u32), accumulator: Image(u32)) !void {
        if (accumulator.rows != self.size or accumulator.cols != self.size) return error.DimensionMismatch;
        try hip.check(c.zg_hough_compute_host(self.handle, &desc(edges), box.l, box.t, box.r, box.b, accumulator.data.ptr, accumulator.stride));
    }

    fn lineFrom(l: c.ZgHoughLine) Line {
        return .{ .angle = l.angle, .radius = l.radius, .score = l.score, .p1 = .init(.{ l.p1[0], l.p1[1] }), .p2 = .init(.{ l.p2[0], l.p2[1] }) };
    }

    /// hough.zig:142-204 on a host accumulator of size x size. Asked again with more room when the candidates or the lines outnumber
    /// the first guess, so the list is the reference's whatever its length (up to max_candidates_limit candidates).
    pub fn findLines(self: Self, allocator: std.mem.Allocator, accumulator: Image(u32), threshold: u32, angle_nms_thresh: f32, radius_nms_thresh: f32) ![]Line {
        if (accumulator.rows != self.size or accumulator.cols != self.size) return error.DimensionMismatch;
        var max_candidates: u32 = 4096;
        var capacity: u32 = 256;
        while (true) {
            const raw = try allocator.alloc(c.ZgHoughLine, capacity);
            defer allocator.free(raw);
            var counts = [2]u32{ 0, 0 };
            try hip.check(c.zg_hough_find_lines_host(self.handle, accumulator.data.ptr, accumulator.stride, threshold, angle_nms_thresh, radius_nms_thresh, max_candidates, raw.ptr, capacity, &counts));
            if (counts[0] > max_candidates_limit) return error.Unsupported;
            if (counts[0] > max_candidates) {
                max_candidates = counts[0];
                continue;
            }
            if (counts[1] > capacity) {
                capacity = counts[1];
                continue;
            }
            const out = try allocator.alloc(Line, counts[1]);
            for (out, raw[0..counts[1]]) |*o, l| o.* = lineFrom(l);
            return out;
        }
    }

    /// The device forms: asynchronous on `stream`, capturable into a graph; every pointer is device memory from zg_malloc.
    pub fn computeInto(self: Self, edges: hip.c.ZgImage, box: Rectangle(u32), accumulator: [*]u32, acc_stride: usize, stream: ?*anyopaque) !void {
        try hip.check(c.zg_hough_compute(self.handle, &edges, box.l, box.t, box.r, box.b, accumulator, acc_stride, stream));
    }

    pub fn findLinesInto(self: Self, accumulator: [*]const u32, acc_stride: usize, threshold: u32, threshold_device: ?*const u32, angle_nms_thresh: f32, radius_nms_thresh: f32, max_candidates: u32, lines: ?[*]c.ZgHoughLine, capacity: u32, counts: [*]u32, stream: ?*anyopaque) !void {
        try hip.check(c.zg_hough_find_lines(self.handle, accumulator, acc_stride, threshold, threshold_device, angle_nms_thresh, radius_nms_thresh, max_candidates, lines, capacity, counts, stream));
    }
};

//! zignal_hip_canvas.zig — the Canvas module of the shim: Canvas(T)'s lines, rectangles, circles, arcs, polygons, Bézier curves and spline polygons (reference
//! src/canvas/Canvas.zig) through libzignal_hip.so's zg_canvas_* entry points (include/zignal_hip_canvas.h). Like the other files of
//! the shim it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub const ZgDrawCmd = extern struct { kind: i32, mode: i32 = 0, width: u32 = 1, color: [4]u8, p: [4]f32 = .{ 0, 0, 0, 0 }, first_vertex: u32 = 0, n_vertices: u32 = 0 };
    pub extern fn zg_sizeof_draw_cmd() usize;
    pub extern fn zg_canvas_tile() u32;
    pub extern fn zg_canvas_draw(img: *const hip.c.ZgImage, cmds: ?[*]const ZgDrawCmd, n: u32, count_device: ?*const u32, vertices: ?[*]const f32, n_vertices: u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_canvas_draw_arcs(img: *const hip.c.ZgImage, cmds: ?[*]const ZgDrawCmd, n: u32, count_device: ?*const u32, vertices: ?[*]const f32, n_vertices: u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_canvas_draw_host(img: *const hip.c.ZgImage, cmds: ?[*]const ZgDrawCmd, n: u32, vertices: ?[*]const f32, n_vertices: u32) c_int;
    pub extern fn zg_canvas_cmds_from_hough_lines(lines: ?*const anyopaque, counts: *const u32, capacity: u32, color: *const [4]u8, width: u32, mode: c_int, cmds_out: ?[*]ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_canvas_cmds_from_keypoints(keypoints: ?*const anyopaque, count: *const u32, capacity: u32, radius: f32, color: *const [4]u8, width: u32, mode: c_int, cmds_out: ?[*]ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgDrawCmd) == 40);
}

pub const Kind = enum(i32) { line = 0, rectangle = 1, fill_rectangle = 2, circle = 3, fill_circle = 4, polygon = 5, fill_polygon = 6, arc = 16, fill_arc = 17, quad_bezier = 18, cubic_bezier = 19, spline_polygon = 20, fill_spline_polygon = 21 };
/// ZG_CANVAS_MAX_CURVE_POINTS: the points a filled spline polygon may tessellate into
pub const max_curve_points: u32 = 512;
pub const DrawMode = zignal.DrawMode;
const Rgba = zignal.Rgba(u8);
const Point = zignal.Point(2, f32);
const Rectangle = zignal.Rectangle(f32);

fn pixelOf(comptime T: type) c_int {
    return switch (T) {
        u8 => 0,
        zignal.Rgb(u8) => 2,
        zignal.Rgba(u8) => 3,
        else => @compileError("Canvas on the device: unsupported pixel type " ++ @typeName(T)),
    };
}

/// Canvas(T) over a host Image(T): the draw methods append to a command list, flush() executes it in list order through
/// zg_canvas_draw_host (which sees the list and takes the kernel that knows arcs only when it holds one) and empties it. The result equals the reference's Canvas(T) making the same calls, byte for byte.
pub fn Canvas(comptime T: type) type {
    return struct {
        image: zignal.Image(T),
        allocator: std.mem.Allocator,
        cmds: std.ArrayList(c.ZgDrawCmd) = .empty,
        vertices: std.ArrayList(f32) = .empty,

        const Self = @This();

        /// zg_draw_cmd carries no size field: a library built from another header must not be handed arrays of this file's ZgDrawCmd
        pub fn init(allocator: std.mem.Allocator, image: zignal.Image(T)) !Self {
            if (c.zg_sizeof_draw_cmd() != @sizeOf(c.ZgDrawCmd)) return error.AbiMismatch;
            return .{ .image = image, .allocator = allocator };
        }
        pub fn deinit(self: *Self) void {
            self.cmds.deinit(self.allocator);
            self.vertices.deinit(self.allocator);
        }

        fn add(self: *Self, kind: Kind, mode: DrawMode, width: u32, color: Rgba, p: [4]f32) !void {
            try self.cmds.append(self.allocator, .{ .kind = @intFromEnum(kind), .mode = if (mode == .soft) 1 else 0, .width = width, .color = .{ color.r, color.g, color.b, color.a }, .p = p });
        }
        fn addPolygon(self: *Self, kind: Kind, polygon: []const Point, mode: DrawMode, width: u32, color: Rgba) !void {
            try self.addPoints(kind, polygon, mode, width, color, 0);
        }
        fn addPoints(self: *Self, kind: Kind, polygon: []const Point, mode: DrawMode, width: u32, color: Rgba, p0: f32) !void {
            const first: u32 = @intCast(self.vertices.items.len / 2);
            for (polygon) |pt| try self.vertices.appendSlice(self.allocator, &.{ pt.x(), pt.y() });
            try self.add(kind, mode, width, color, .{ p0, 0, 0, 0 });
            self.cmds.items[self.cmds.items.len - 1].first_vertex = first;
            self.cmds.items[self.cmds.items.len - 1].n_vertices = @intCast(polygon.len);
        }
        pub fn drawLine(self: *Self, p1: Point, p2: Point, color: Rgba, width: u32, mode: DrawMode) !void {
            try self.add(.line, mode, width, color, .{ p1.x(), p1.y(), p2.x(), p2.y() });
        }
        pub fn drawRectangle(self: *Self, rect: Rectangle, color: Rgba, width: u32, mode: DrawMode) !void {
            try self.add(.rectangle, mode, width, color, .{ rect.l, rect.t, rect.r, rect.b });
        }
        pub fn fillRectangle(self: *Self, rect: Rectangle, color: Rgba, mode: DrawMode) !void {
            try self.add(.fill_rectangle, mode, 1, color, .{ rect.l, rect.t, rect.r, rect.b });
        }
        pub fn drawCircle(self: *Self, center: Point, radius: f32, color: Rgba, width: u32, mode: DrawMode) !void {
            try self.add(.circle, mode, width, color, .{ center.x(), center.y(), radius, 0 });
        }
        pub fn fillCircle(self: *Self, center: Point, radius: f32, color: Rgba, mode: DrawMode) !void {
            try self.add(.fill_circle, mode, 1, color, .{ center.x(), center.y(), radius, 0 });
        }
        /// The two angles travel as one entry of the vertex array; any finite angle, normalised as the reference's ArcRange does.
        pub fn drawArc(self: *Self, center: Point, radius: f32, start_angle: f32, end_angle: f32, color: Rgba, width: u32, mode: DrawMode) !void {
            try self.addArc(.arc, center, radius, start_angle, end_angle, mode, width, color);
        }
        pub fn fillArc(self: *Self, center: Point, radius: f32, start_angle: f32, end_angle: f32, color: Rgba, mode: DrawMode) !void {
            try self.addArc(.fill_arc, center, radius, start_angle, end_angle, mode, 1, color);
        }
        fn addArc(self: *Self, kind: Kind, center: Point, radius: f32, start_angle: f32, end_angle: f32, mode: DrawMode, width: u32, color: Rgba) !void {
            const first: u32 = @intCast(self.vertices.items.len / 2);
            try self.vertices.appendSlice(self.allocator, &.{ start_angle, end_angle });
            try self.add(kind, mode, width, color, .{ center.x(), center.y(), radius, 0 });
            self.cmds.items[self.cmds.items.len - 1].first_vertex = first;
            self.cmds.items[self.cmds.items.len - 1].n_vertices = 1;
        }
        pub fn drawPolygon(self: *Self, polygon: []const Point, color: Rgba, width: u32, mode: DrawMode) !void {
            try self.addPolygon(.polygon, polygon, mode, width, color);
        }
        pub fn fillPolygon(self: *Self, polygon: []const Point, color: Rgba, mode: DrawMode) !void {
            try self.addPolygon(.fill_polygon, polygon, mode, 1, color);
        }
        pub fn drawQuadraticBezier(self: *Self, p0: Point, p1: Point, p2: Point, color: Rgba, width: u32, mode: DrawMode) !void {
            try self.addPoints(.quad_bezier, &.{ p0, p1, p2 }, mode, width, color, 0);
        }
        pub fn drawCubicBezier(self: *Self, p0: Point, p1: Point, p2: Point, p3: Point, color: Rgba, width: u32, mode: DrawMode) !void {
            try self.addPoints(.cubic_bezier, &.{ p0, p1, p2, p3 }, mode, width, color, 0);
        }
        pub fn drawSplinePolygon(self: *Self, polygon: []const Point, color: Rgba, width: u32, tension: f32, mode: DrawMode) !void {
            try self.addPoints(.spline_polygon, polygon, mode, width, color, tension);
        }
        /// At most max_curve_points points once tessellated: past that flush() fails and draws nothing.
        pub fn fillSplinePolygon(self: *Self, polygon: []const Point, color: Rgba, tension: f32, mode: DrawMode) !void {
            try self.addPoints(.fill_spline_polygon, polygon, mode, 1, color, tension);
        }
        pub fn flush(self: *Self) !void {
            defer self.cmds.clearRetainingCapacity();
            defer self.vertices.clearRetainingCapacity();
            if (self.cmds.items.len == 0) return;
            const d: hip.c.ZgImage = .{ .data = @ptrCast(self.image.data.ptr), .stride = self.image.stride, .rows = self.image.rows, .cols = self.image.cols, .pixel = pixelOf(T) };
            const nv: u32 = @intCast(self.vertices.items.len / 2);
            try hip.check(c.zg_canvas_draw_host(&d, self.cmds.items.ptr, @intCast(self.cmds.items.len), if (nv != 0) self.vertices.items.ptr else null, nv));
        }
    };
}

/// The device form: asynchronous on `stream`, capturable into a graph; image.data, cmds, count_device and vertices are device memory
/// from zg_malloc. count_device null draws all n commands.
pub fn drawInto(image: hip.c.ZgImage, cmds: [*]const c.ZgDrawCmd, n: u32, count_device: ?*const u32, vertices: ?[*]const f32, n_vertices: u32, stream: ?*anyopaque) !void {
    if (c.zg_sizeof_draw_cmd() != @sizeOf(c.ZgDrawCmd)) return error.AbiMismatch;
    try hip.check(c.zg_canvas_draw(&image, cmds, n, count_device, vertices, n_vertices, stream));
}

/// drawInto for a list that may hold .arc or .fill_arc commands (zg_canvas_draw_arcs; drawInto skips them): the caller who built the
/// device list knows whether it may.
pub fn drawArcsInto(image: hip.c.ZgImage, cmds: [*]const c.ZgDrawCmd, n: u32, count_device: ?*const u32, vertices: ?[*]const f32, n_vertices: u32, stream: ?*anyopaque) !void {
    if (c.zg_sizeof_draw_cmd() != @sizeOf(c.ZgDrawCmd)) return error.AbiMismatch;
    try hip.check(c.zg_canvas_draw_arcs(&image, cmds, n, count_device, vertices, n_vertices, stream));
}

/// One line command per line of zg_hough_find_lines' device list; counts is that call's two device words.
pub fn cmdsFromHoughLines(lines: ?*const anyopaque, counts: *const u32, capacity: u32, color: Rgba, width: u32, mode: DrawMode, cmds_out: ?[*]c.ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) !void {
    const col = [4]u8{ color.r, color.g, color.b, color.a };
    try hip.check(c.zg_canvas_cmds_from_hough_lines(lines, counts, capacity, &col, width, if (mode == .soft) 1 else 0, cmds_out, count_out, stream));
}

/// One circle outline of `radius` at each keypoint of a detector's device list; count is its device count word.
pub fn cmdsFromKeypoints(keypoints: ?*const anyopaque, count: *const u32, capacity: u32, radius: f32, color: Rgba, width: u32, mode: DrawMode, cmds_out: ?[*]c.ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) !void {
    const col = [4]u8{ color.r, color.g, color.b, color.a };
    try hip.check(c.zg_canvas_cmds_from_keypoints(keypoints, count, capacity, radius, &col, width, if (mode == .soft) 1 else 0, cmds_out, count_out, stream));
}

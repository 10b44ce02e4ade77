//! zignal_hip_flood.zig — the flood-fill module of the shim: Image(T).floodFill (reference src/image/flood_fill.zig) through
//! libzignal_hip.so's zg_flood_fill* entry points (include/zignal_hip_flood.h). Like the other files of the shim it has not been
//! compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub const ZgFloodFillOptions = extern struct { threshold: f64 = 0, connectivity: c_int = 4, mode: c_int = 0 }; // flood_fill.zig:5-26
    pub extern fn zg_flood_fill_tile() u32;
    pub extern fn zg_flood_fill_bound_host(pixel: c_int, threshold: f64, bound: *f64) c_int;
    pub extern fn zg_flood_fill(img: *const hip.c.ZgImage, row: u32, col: u32, seed_device: ?[*]const u32, fill_value: *const anyopaque, opt: ?*const ZgFloodFillOptions, filled_count_device: ?*u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_flood_fill_host(img: *const hip.c.ZgImage, row: u32, col: u32, fill_value: *const anyopaque, opt: ?*const ZgFloodFillOptions, filled_count: ?*u32) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgFloodFillOptions) == 16);
}

pub const FloodFillOptions = zignal.FloodFillOptions;

fn options(o: FloodFillOptions) c.ZgFloodFillOptions {
    return .{ .threshold = o.threshold, .connectivity = @intFromEnum(o.connectivity), .mode = switch (o.mode) {
        .seed => 0,
        .neighbor => 1,
    } };
}

/// ZG_PIXEL_* of a pixel type the library fills: u8, f32, Rgb / Rgba of u8 and of f32.
fn pixelOf(comptime T: type) c_int {
    return switch (T) {
        u8 => 0,
        f32 => 1,
        zignal.Rgb(u8) => 2,
        zignal.Rgba(u8) => 3,
        zignal.Rgb(f32) => 4,
        zignal.Rgba(f32) => 5,
        else => @compileError("floodFill on the device: unsupported pixel type " ++ @typeName(T)),
    };
}

fn desc(comptime T: type, img: zignal.Image(T)) hip.c.ZgImage {
    return .{ .data = @ptrCast(img.data.ptr), .stride = img.stride, .rows = img.rows, .cols = img.cols, .pixel = pixelOf(T) };
}

/// Drop-in for Image(T).floodFill on a host image (flood_fill.zig:59-131); returns the number of filled pixels. A seed outside the
/// image is error.OutOfBounds, as in the reference.
pub fn floodFill(comptime T: type, image: zignal.Image(T), start_row: u32, start_col: u32, fill_value: T, opts: FloodFillOptions) !u32 {
    if (start_row >= image.rows or start_col >= image.cols) return error.OutOfBounds;
    var filled: u32 = 0;
    const o = options(opts);
    try hip.check(c.zg_flood_fill_host(&desc(T, image), start_row, start_col, @ptrCast(&fill_value), &o, &filled));
    return filled;
}

/// The device form: asynchronous on `stream`, capturable into a graph; image.data, seed_device (two words: row, col) and
/// filled_count_device are device memory from zg_malloc.
pub fn floodFillInto(image: hip.c.ZgImage, start_row: u32, start_col: u32, seed_device: ?[*]const u32, fill_value: *const anyopaque, opts: FloodFillOptions, filled_count_device: ?*u32, stream: ?*anyopaque) !void {
    const o = options(opts);
    try hip.check(c.zg_flood_fill(&image, start_row, start_col, seed_device, fill_value, &o, filled_count_device, stream));
}

/// The constant the kernels compare with (zg_flood_fill_bound_host): host arithmetic.
pub fn bound(pixel: c_int, threshold: f64) !f64 {
    var b: f64 = 0;
    try hip.check(c.zg_flood_fill_bound_host(pixel, threshold, &b));
    return b;
}

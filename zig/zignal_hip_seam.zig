//! zignal_hip_seam.zig — the seam-carving module of the shim: the reference's seam_carve example (examples/src/seam_carving.zig) through
//! libzignal_hip.so's zg_seam_* entry points (include/zignal_hip_seam.h). Like the other files of the shim it has not been compiled
//! where the library is built (no Zig toolchain), so it stays thin: the four functions keep the example's arguments and return an
//! error union where the example returns void.
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub extern fn zg_seam_band_rows() u32;
    pub extern fn zg_seam_strip_cols() u32;
    pub extern fn zg_seam_energy(edges: *const hip.c.ZgImage, energy: [*]u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_seam_find(energy: [*]const u32, rows: u32, cols: u32, seam: [*]u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_seam_remove(src: *const hip.c.ZgImage, seam: [*]const u32, dst: *const hip.c.ZgImage, stream: ?*anyopaque) c_int;
    pub extern fn zg_seam_carve(src: *const hip.c.ZgImage, dst: *const hip.c.ZgImage, n: u32, axis: c_int, energy_source: ?*const hip.c.ZgImage, seams_device: ?[*]u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_seam_energy_host(edges: *const hip.c.ZgImage, energy: [*]u32) c_int;
    pub extern fn zg_seam_find_host(energy: [*]const u32, rows: u32, cols: u32, seam: [*]u32) c_int;
    pub extern fn zg_seam_remove_host(src: *const hip.c.ZgImage, seam: [*]const u32, dst: *const hip.c.ZgImage) c_int;
    pub extern fn zg_seam_carve_host(src: *const hip.c.ZgImage, dst: *const hip.c.ZgImage, n: u32, axis: c_int, energy_source: ?*const hip.c.ZgImage, seams: ?[*]u32) c_int;
};

pub const Axis = enum(c_int) { vertical = 0, horizontal = 1 };

/// ZG_PIXEL_* of a pixel type the library carves: u8, f32, Rgb / Rgba of u8 and of f32.
fn pixelOf(comptime T: type) c_int {
    return switch (T) {
        u8 => 0,
        f32 => 1,
        zignal.Rgb(u8) => 2,
        zignal.Rgba(u8) => 3,
        zignal.Rgb(f32) => 4,
        zignal.Rgba(f32) => 5,
        else => @compileError("seam carving on the device: unsupported pixel type " ++ @typeName(T)),
    };
}

fn desc(comptime T: type, img: zignal.Image(T)) hip.c.ZgImage {
    return .{ .data = @ptrCast(img.data.ptr), .stride = img.stride, .rows = img.rows, .cols = img.cols, .pixel = pixelOf(T) };
}

/// The u32 words the library wrote at the front of a []usize, widened in place from the back.
fn widen(seam: []usize) void {
    const words: [*]const u32 = @ptrCast(seam.ptr);
    var i = seam.len;
    while (i > 0) {
        i -= 1;
        seam[i] = words[i];
    }
}

/// computeEnergy (:22-45). energy is packed (stride == cols), as the example's is.
pub fn computeEnergy(edges: zignal.Image(u8), energy: *zignal.Image(u32)) !void {
    if (edges.rows != energy.rows or edges.cols != energy.cols or energy.stride != energy.cols) return error.DimensionMismatch;
    try hip.check(c.zg_seam_energy_host(&desc(u8, edges), energy.data.ptr));
}

/// computeSeam (:47-74).
pub fn computeSeam(energy: zignal.Image(u32), seam: []usize) !void {
    if (energy.rows != seam.len or energy.stride != energy.cols) return error.DimensionMismatch;
    try hip.check(c.zg_seam_find_host(energy.data.ptr, energy.rows, energy.cols, @ptrCast(seam.ptr)));
    widen(seam);
}

/// removeSeam (:76-102): in place as in the example, through a copy of the pixels (the library's form is out of place).
pub fn removeSeam(comptime T: type, image: *zignal.Image(T), seam: []const usize) !void {
    if (image.rows != seam.len or image.cols == 0) return error.DimensionMismatch;
    const gpa = std.heap.page_allocator;
    const words = try gpa.alloc(u32, seam.len);
    defer gpa.free(words);
    for (seam, words) |s, *w| w.* = @intCast(@min(s, std.math.maxInt(u32)));
    var copy = try zignal.Image(T).init(gpa, image.rows, image.cols);
    defer copy.deinit(gpa);
    image.copy(copy);
    const size = image.rows * image.cols;
    image.cols -= 1;
    image.stride = image.cols;
    image.data = image.data[0..(size - image.rows)];
    try hip.check(c.zg_seam_remove_host(&desc(T, copy), words.ptr, &desc(T, image.*)));
}

/// n iterations of the example's seam_carve (:104-144) on a host image; `seams`, when given, is n * rows entries (n * cols for the
/// horizontal axis, which is the library's own definition). The result is a new image from `gpa`.
pub fn seamCarve(comptime T: type, gpa: std.mem.Allocator, image: zignal.Image(T), n: u32, axis: Axis, seams: ?[]usize) !zignal.Image(T) {
    const rows = if (axis == .horizontal) image.rows -| n else image.rows;
    const cols = if (axis == .horizontal) image.cols else image.cols -| n;
    var out = try zignal.Image(T).init(gpa, rows, cols);
    errdefer out.deinit(gpa);
    const words: ?[*]u32 = if (seams) |s| @ptrCast(s.ptr) else null;
    try hip.check(c.zg_seam_carve_host(&desc(T, image), &desc(T, out), n, @intFromEnum(axis), null, words));
    if (seams) |s| widen(s);
    return out;
}

/// The device form: asynchronous on `stream`, capturable into a graph; the images' data and seams_device are device memory.
pub fn seamCarveInto(src: hip.c.ZgImage, dst: hip.c.ZgImage, n: u32, axis: Axis, seams_device: ?[*]u32, stream: ?*anyopaque) !void {
    try hip.check(c.zg_seam_carve(&src, &dst, n, @intFromEnum(axis), null, seams_device, stream));
}

//! zignal_hip_qr.zig — the QR detector module of the shim: reference src/qrcode/detector.zig:57-641 through libzignal_hip.so's
//! zg_qr_detect* entry points, up to the sampled module grids that the reference hands to decoder.decodeModules, and the builder from
//! their corners to Canvas line commands (include/zignal_hip_qr.h). Decoding the grids stays with the reference's own decoder. Like the
//! other files of the shim it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");
const canvas = @import("zignal_hip_canvas.zig");

pub const max_modules = 177 * 177;
pub const Binarize = enum(c_int) { adaptive = 0, otsu = 1, binary = 2 };

pub const c = struct {
    pub const ZgQrFinder = extern struct { x: f32, y: f32, module_size: f32, hits: f32 }; // detector.zig:170-175
    pub const ZgQrFourth = extern struct { x: f32, y: f32, is_alignment: u32 }; // :410-413
    pub const ZgQrDetection = extern struct {
        finders: [64]ZgQrFinder,
        finder_count: u32,
        merged_count: u32,
        triple_found: u32,
        triple: [3]ZgQrFinder,
        version_estimate: u32,
        version_count: u32,
        versions: [8]u8,
        fourth_count: u32,
        fourths: [5]ZgQrFourth,
        grids_total: u32,
        grids_written: u32,
        modules_written: u32,
    };
    pub const ZgQrGrid = extern struct {
        version: u32,
        dim: u32,
        fourth_index: u32,
        modules_offset: u32,
        version_hint: i32,
        corners: [8]f32,
        reserved: u32,
        transform: [9]f64,
    };
    pub extern fn zg_qr_sizeof_detection() usize;
    pub extern fn zg_qr_sizeof_grid() usize;
    pub extern fn zg_qr_scratch_bytes(rows: u32, cols: u32) usize;
    pub extern fn zg_qr_detect(src: *const hip.c.ZgImage, binarize: c_int, detection: *ZgQrDetection, grids: ?[*]ZgQrGrid, grid_capacity: u32, modules: ?[*]u8, module_capacity: u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_qr_detect_host(src: *const hip.c.ZgImage, binarize: c_int, detection: *ZgQrDetection, grids: ?[*]ZgQrGrid, grid_capacity: u32, modules: ?[*]u8, module_capacity: u32) c_int;
    pub extern fn zg_canvas_cmds_from_qr(grids: ?[*]const ZgQrGrid, detection: *const ZgQrDetection, capacity: u32, color: *const [4]u8, width: u32, mode: c_int, cmds_out: ?[*]canvas.c.ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgQrDetection) == 1176);
    std.debug.assert(@sizeOf(c.ZgQrGrid) == 128);
}

/// The grids of one binarisation of a host Image(u8), in the reference's order of trial: what detectAndDecode (detector.zig:86-156)
/// hands to decoder.decodeModules one after another. `modules` holds every grid's dim * dim bytes at its modules_offset. The caller
/// owns both slices. Walking them in order and stopping at the first grid that decodeModules accepts reproduces the reference.
pub const Grids = struct { detection: c.ZgQrDetection, grids: []c.ZgQrGrid, modules: []u8 };

pub fn detectPass(gpa: std.mem.Allocator, image: zignal.Image(u8), binarize: Binarize) !Grids {
    const d: hip.c.ZgImage = .{ .data = @ptrCast(image.data.ptr), .stride = image.stride, .rows = image.rows, .cols = image.cols, .pixel = 0 };
    var det: c.ZgQrDetection = undefined;
    try hip.check(c.zg_qr_detect_host(&d, @intFromEnum(binarize), &det, null, 0, null, 0));
    const n = det.grids_total;
    const grids = try gpa.alloc(c.ZgQrGrid, n);
    errdefer gpa.free(grids);
    const modules = try gpa.alloc(u8, @as(usize, n) * max_modules);
    errdefer gpa.free(modules);
    try hip.check(c.zg_qr_detect_host(&d, @intFromEnum(binarize), &det, if (n > 0) grids.ptr else null, n, if (n > 0) modules.ptr else null, n * max_modules));
    return .{ .detection = det, .grids = grids[0..det.grids_written], .modules = modules };
}

/// The device form: asynchronous on `stream`, capturable into a graph; src.data, detection, grids and modules are device memory.
pub fn detectInto(src: hip.c.ZgImage, binarize: Binarize, detection: *c.ZgQrDetection, grids: ?[*]c.ZgQrGrid, grid_capacity: u32, modules: ?[*]u8, module_capacity: u32, stream: ?*anyopaque) !void {
    try hip.check(c.zg_qr_detect(&src, @intFromEnum(binarize), detection, grids, grid_capacity, modules, module_capacity, stream));
}

/// Four ZG_DRAW_LINE commands per written grid, outlining its corners, built on the device (zg_canvas_cmds_from_qr).
pub fn cmdsFromQr(grids: ?[*]const c.ZgQrGrid, detection: *const c.ZgQrDetection, capacity: u32, color: [4]u8, width: u32, mode: c_int, cmds_out: ?[*]canvas.c.ZgDrawCmd, count_out: *u32, stream: ?*anyopaque) !void {
    try hip.check(c.zg_canvas_cmds_from_qr(grids, detection, capacity, &color, width, mode, cmds_out, count_out, stream));
}

//! zignal_hip_quantize.zig — the quantisation module of the shim: the colour histogram, median cut and lookup table of the reference's
//! src/image/quantize.zig, the dither modes of src/image/dither.zig and mapImageToPalette (src/codecs/gif.zig:875-920) through
//! libzignal_hip.so's entry points (include/zignal_hip_quantize.h). Like the other files of the shim it has not been compiled where the
//! library is built (no Zig toolchain). The GIF container and its LZW, sixel output and Mode.auto's heuristic stay with the reference.
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const histogram_cells: usize = 32768; // ZG_HISTOGRAM_CELLS
pub const histogram_untouched: u32 = 0xFFFFFFFF; // ZG_HISTOGRAM_UNTOUCHED

pub const c = struct {
    pub extern fn zg_color_histogram(img: *const hip.c.ZgImage, counts_device: [*]u32, first_device: [*]u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_median_cut_from_histogram_host(counts: [*]const u32, first: [*]const u32, max_colors: u32, capacity: u32, palette_rgb: [*]u8, n: *u32) c_int;
    pub extern fn zg_median_cut(img_device: *const hip.c.ZgImage, max_colors: u32, capacity: u32, palette_rgb: [*]u8, n: *u32) c_int;
    pub extern fn zg_build_palette(img_device: ?*const hip.c.ZgImage, mode: c_int, max_colors: u32, palette_rgb: [*]u8, n: *u32) c_int;
    pub extern fn zg_palette_lut(palette_device: [*]const u8, n: u32, lut_device: [*]u8, stream: ?*anyopaque) c_int;
    pub extern fn zg_palette_lut_host(palette: [*]const u8, n: u32, lut: [*]u8) c_int;
    pub extern fn zg_dither_geometry(band_rows: ?*u32, phase_cols: ?*u32, rows_per_launch: ?*u32) void;
    pub extern fn zg_dither(img: *const hip.c.ZgImage, palette_device: [*]const u8, n: u32, lut_device: [*]const u8, mode: c_int, stream: ?*anyopaque) c_int;
    pub extern fn zg_dither_frames(img: *const hip.c.ZgImage, n_frames: u32, frame_bytes: usize, palette_device: [*]const u8, n: u32, lut_device: [*]const u8, mode: c_int, stream: ?*anyopaque) c_int;
    pub extern fn zg_palette_map(src: *const hip.c.ZgImage, indices: *const hip.c.ZgImage, palette_device: [*]const u8, n: u32, use_dither: c_int, transparent_index: c_int, stream: ?*anyopaque) c_int;
};

pub const Rgb = zignal.Rgb(u8);

comptime {
    std.debug.assert(@sizeOf(Rgb) == 3); // a palette crosses the boundary as n x 3 bytes
}

/// dither.Mode's ordinal (dither.zig:18-30): the declaration order is the library's ZG_DITHER_*.
pub fn ditherMode(mode: anytype) c_int {
    return @intFromEnum(mode);
}

/// PaletteMode's ordinal and max_colors (quantize.zig:476-498).
fn paletteMode(mode: anytype) struct { c_int, u32 } {
    return switch (mode) {
        .fixed_6x7x6 => .{ 0, 256 },
        .fixed_vga16 => .{ 1, 256 },
        .fixed_web216 => .{ 2, 256 },
        .adaptive => |opts| .{ 3, opts.max_colors },
    };
}

/// medianCut (quantize.zig:175-412) from the histogram zg_color_histogram leaves (host copies of its two arrays). Host arithmetic.
pub fn medianCutFromHistogram(counts: *const [histogram_cells]u32, first: *const [histogram_cells]u32, palette: []Rgb, max_colors: u16) !usize {
    var n: u32 = 0;
    hip.check(c.zg_median_cut_from_histogram_host(counts, first, max_colors, @intCast(@min(palette.len, 256)), @ptrCast(palette.ptr), &n)) catch |e| {
        return if (e == error.InvalidArgument) error.NoPaletteColors else e;
    };
    return n;
}

/// medianCut of a device image (u8, Rgb(u8) or Rgba(u8)): synchronises once, not capturable.
pub fn medianCut(image_device: hip.c.ZgImage, palette: []Rgb, max_colors: u16) !usize {
    var n: u32 = 0;
    hip.check(c.zg_median_cut(&image_device, max_colors, @intCast(@min(palette.len, 256)), @ptrCast(palette.ptr), &n)) catch |e| {
        return if (e == error.InvalidArgument) error.NoPaletteColors else e;
    };
    return n;
}

/// buildPalette (quantize.zig:502-527); image_device may be null for the fixed modes.
pub fn buildPalette(image_device: ?*const hip.c.ZgImage, mode: anytype, palette: *[256]Rgb) !usize {
    var n: u32 = 0;
    const m = paletteMode(mode);
    try hip.check(c.zg_build_palette(image_device, m[0], m[1], @ptrCast(palette), &n));
    return n;
}

/// ColorLookupTable.init (quantize.zig:66-159) on the host: table[r5][g5][b5] as 32768 bytes.
pub fn paletteLut(palette: []const Rgb, table: *[32][32][32]u8) !void {
    try hip.check(c.zg_palette_lut_host(@ptrCast(palette.ptr), @intCast(palette.len), @ptrCast(table)));
}

/// The device forms: asynchronous on `stream`, capturable into a graph; every pointer is device memory from zg_malloc.
pub fn colorHistogramInto(image: hip.c.ZgImage, counts_device: [*]u32, first_device: [*]u32, stream: ?*anyopaque) !void {
    try hip.check(c.zg_color_histogram(&image, counts_device, first_device, stream));
}

pub fn paletteLutInto(palette_device: [*]const u8, n: u32, lut_device: [*]u8, stream: ?*anyopaque) !void {
    try hip.check(c.zg_palette_lut(palette_device, n, lut_device, stream));
}

/// dither.apply (dither.zig:34-41) in place on an Rgb(u8) device image.
pub fn ditherInto(image: hip.c.ZgImage, palette_device: [*]const u8, n: u32, lut_device: [*]const u8, mode: anytype, stream: ?*anyopaque) !void {
    try hip.check(c.zg_dither(&image, palette_device, n, lut_device, ditherMode(mode), stream));
}

/// The same over n_frames frames frame_bytes apart: one workgroup per frame.
pub fn ditherFramesInto(image: hip.c.ZgImage, n_frames: u32, frame_bytes: usize, palette_device: [*]const u8, n: u32, lut_device: [*]const u8, mode: anytype, stream: ?*anyopaque) !void {
    try hip.check(c.zg_dither_frames(&image, n_frames, frame_bytes, palette_device, n, lut_device, ditherMode(mode), stream));
}

/// mapImageToPalette (gif.zig:875-920): `indices` is a u8 device image of src's rows and cols.
pub fn mapImageToPaletteInto(src: hip.c.ZgImage, indices: hip.c.ZgImage, palette_device: [*]const u8, n: u32, use_dither: bool, transparent_index: ?u8, stream: ?*anyopaque) !void {
    try hip.check(c.zg_palette_map(&src, &indices, palette_device, n, @intFromBool(use_dither), if (transparent_index) |t| t else -1, stream));
}

/// (band rows, phase columns, rows per launch) of the error-diffusion kernel.
pub fn ditherGeometry() [3]u32 {
    var g: [3]u32 = .{ 0, 0, 0 };
    c.zg_dither_geometry(&g[0], &g[1], &g[2]);
    return g;
}

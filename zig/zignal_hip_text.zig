//! zignal_hip_text.zig — the text module of the shim: Canvas(T).drawText with the caller's BitmapFont (reference src/canvas/Canvas.zig:1476-1658,
//! src/font/BitmapFont.zig) through libzignal_hip.so's zg_canvas_draw_text* entry points (include/zignal_hip_text.h). Like the other files of
//! the shim it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const c = struct {
    pub const ZgGlyph = extern struct { codepoint: u32, bitmap_offset: u32, width: u8, height: u8, x_offset: i16, y_offset: i16, device_width: i16 };
    pub const ZgFont = extern struct { data: ?[*]const u8 = null, glyphs: ?[*]const ZgGlyph = null, data_len: u32 = 0, n_glyphs: u32 = 0, char_width: u8 = 0, char_height: u8 = 0, first_char: u8 = 0, last_char: u8 = 0, reserved: u32 = 0 };
    pub const ZgTextCmd = extern struct { x: f32, y: f32, scale: f32 = 1, mode: i32 = 0, color: [4]u8, first_codepoint: u32 = 0, n_codepoints: u32 = 0 };
    pub extern fn zg_sizeof_font() usize;
    pub extern fn zg_sizeof_glyph() usize;
    pub extern fn zg_sizeof_text_cmd() usize;
    pub extern fn zg_font_check(host_font: ?*const ZgFont) c_int;
    pub extern fn zg_font_upload(host_font: ?*const ZgFont, device_font: ?*ZgFont) c_int;
    pub extern fn zg_font_free(device_font: ?*ZgFont) c_int;
    pub extern fn zg_text_bounds_host(host_font: ?*const ZgFont, codepoints: ?[*]const u32, n: u32, scale: f32, out_ltrb: *[4]f32) c_int;
    pub extern fn zg_canvas_draw_text(img: *const hip.c.ZgImage, font: ?*const ZgFont, cmds: ?[*]const ZgTextCmd, n: u32, count_device: ?*const u32, codepoints: ?[*]const u32, n_codepoints: u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_canvas_draw_text_host(img: *const hip.c.ZgImage, host_font: ?*const ZgFont, cmds: ?[*]const ZgTextCmd, n: u32, codepoints: ?[*]const u32, n_codepoints: u32) c_int;
};

comptime {
    std.debug.assert(@sizeOf(c.ZgGlyph) == 16 and @sizeOf(c.ZgFont) == 32 and @sizeOf(c.ZgTextCmd) == 28);
}

/// ZG_TEXT_MAX_SCALE, ZG_TEXT_MAX_CODEPOINTS (of one command), ZG_TEXT_MAX_COMMANDS and ZG_TEXT_MAX_TOTAL (of one call)
pub const max_scale: f32 = 64.0;
pub const max_codepoints: u32 = 65536;
pub const max_commands: u32 = 65536;
pub const max_total: u32 = 16777216;
pub const DrawMode = zignal.DrawMode;
const Rgba = zignal.Rgba(u8);
const Point = zignal.Point(2, f32);
const Rectangle = zignal.Rectangle(f32);

fn abiChecked() !void {
    if (c.zg_sizeof_font() != @sizeOf(c.ZgFont) or c.zg_sizeof_glyph() != @sizeOf(c.ZgGlyph) or c.zg_sizeof_text_cmd() != @sizeOf(c.ZgTextCmd)) return error.AbiMismatch;
}

fn pixelOf(comptime T: type) c_int {
    return switch (T) {
        u8 => 0,
        zignal.Rgb(u8) => 2,
        zignal.Rgba(u8) => 3,
        else => @compileError("drawText on the device: unsupported pixel type " ++ @typeName(T)),
    };
}

/// A BitmapFont over the caller's tables (the library ships no glyphs), in the reference's two forms. The slices must outlive the font.
pub const BitmapFont = struct {
    font: c.ZgFont,

    /// glyph cp is char_height rows of (char_width + 7) / 8 bytes at (cp - first_char) times that, bits LSB first
    pub fn initFixed(char_width: u8, char_height: u8, first_char: u8, last_char: u8, data: []const u8) !BitmapFont {
        try abiChecked();
        const f: c.ZgFont = .{ .data = data.ptr, .data_len = @intCast(data.len), .char_width = char_width, .char_height = char_height, .first_char = first_char, .last_char = last_char };
        try hip.check(c.zg_font_check(&f));
        return .{ .font = f };
    }
    /// glyphs sorted by codepoint, every codepoint once; a codepoint the table lacks advances by char_width
    pub fn initGlyphs(char_width: u8, char_height: u8, glyphs: []const c.ZgGlyph, data: []const u8) !BitmapFont {
        try abiChecked();
        const f: c.ZgFont = .{ .data = data.ptr, .glyphs = glyphs.ptr, .data_len = @intCast(data.len), .n_glyphs = @intCast(glyphs.len), .char_width = char_width, .char_height = char_height };
        try hip.check(c.zg_font_check(&f));
        return .{ .font = f };
    }
    /// getTextBounds over codepoints
    pub fn textBounds(self: BitmapFont, codepoints: []const u32, scale: f32) !Rectangle {
        var ltrb: [4]f32 = undefined;
        try hip.check(c.zg_text_bounds_host(&self.font, codepoints.ptr, @intCast(codepoints.len), scale, &ltrb));
        return .{ .l = ltrb[0], .t = ltrb[1], .r = ltrb[2], .b = ltrb[3] };
    }
    /// The font with its tables on the current device, for drawTextInto; release it with freeDevice.
    pub fn upload(self: BitmapFont) !c.ZgFont {
        var device: c.ZgFont = .{};
        try hip.check(c.zg_font_upload(&self.font, &device));
        return device;
    }
    pub fn freeDevice(device: *c.ZgFont) void {
        _ = c.zg_font_free(device);
    }
};

/// drawText calls over a host Image(T): drawText appends to a list (the text decoded from UTF-8), flush() executes it in order through
/// zg_canvas_draw_text_host and empties it. One font per TextCanvas; draw other commands through zignal_hip_canvas.zig's Canvas and flush
/// the two in the order the calls are to take effect. The result equals the reference's Canvas(T).drawText making the same calls, byte for byte.
pub fn TextCanvas(comptime T: type) type {
    return struct {
        image: zignal.Image(T),
        allocator: std.mem.Allocator,
        font: BitmapFont,
        cmds: std.ArrayList(c.ZgTextCmd) = .empty,
        codepoints: std.ArrayList(u32) = .empty,

        const Self = @This();

        pub fn init(allocator: std.mem.Allocator, image: zignal.Image(T), font: BitmapFont) !Self {
            try abiChecked();
            return .{ .image = image, .allocator = allocator, .font = font };
        }
        pub fn deinit(self: *Self) void {
            self.cmds.deinit(self.allocator);
            self.codepoints.deinit(self.allocator);
        }
        pub fn drawText(self: *Self, text: []const u8, position: Point, color: Rgba, scale: f32, mode: DrawMode) !void {
            const first: u32 = @intCast(self.codepoints.items.len);
            var it = std.unicode.Utf8Iterator{ .bytes = text, .i = 0 };
            while (it.nextCodepoint()) |cp| try self.codepoints.append(self.allocator, cp);
            try self.cmds.append(self.allocator, .{ .x = position.x(), .y = position.y(), .scale = scale, .mode = if (mode == .soft) 1 else 0, .color = .{ color.r, color.g, color.b, color.a }, .first_codepoint = first, .n_codepoints = @as(u32, @intCast(self.codepoints.items.len)) - first });
        }
        pub fn flush(self: *Self) !void {
            defer self.cmds.clearRetainingCapacity();
            defer self.codepoints.clearRetainingCapacity();
            if (self.cmds.items.len == 0) return;
            const d: hip.c.ZgImage = .{ .data = @ptrCast(self.image.data.ptr), .stride = self.image.stride, .rows = self.image.rows, .cols = self.image.cols, .pixel = pixelOf(T) };
            const n: u32 = @intCast(self.codepoints.items.len);
            try hip.check(c.zg_canvas_draw_text_host(&d, &self.font.font, self.cmds.items.ptr, @intCast(self.cmds.items.len), if (n != 0) self.codepoints.items.ptr else null, n));
        }
    };
}

/// The device form: asynchronous on `stream`, capturable into a graph; image.data, the font's tables (BitmapFont.upload), cmds,
/// count_device and codepoints are device memory. count_device null draws all n commands.
pub fn drawTextInto(image: hip.c.ZgImage, device_font: *const c.ZgFont, cmds: [*]const c.ZgTextCmd, n: u32, count_device: ?*const u32, codepoints: ?[*]const u32, n_codepoints: u32, stream: ?*anyopaque) !void {
    try abiChecked();
    try hip.check(c.zg_canvas_draw_text(&image, device_font, cmds, n, count_device, codepoints, n_codepoints, stream));
}

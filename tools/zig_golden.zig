//! zig_golden.zig — golden vectors for the transcendental boundary of zignal's image hot path, made by REAL Zig.
//!
//! The MI355X library and its CPU oracle restate Zig's std maths (musl's expf / sinf / cosf / cbrtf, Go's Pow) from the published
//! algorithms, because no Zig toolchain exists where they are built (DESIGN.md §4: "parity unpinned against Zig at the last ulp").
//! This program is the other half of that sentence: run it once with the toolchain the reference pins
//! (build.zig.zon: minimum_zig_version 0.17.0-dev.1441+d5181a9c9) and the pytest beside it turns "unpinned" into "pinned":
//!
//!     zig run -O ReleaseFast --dep zignal -Mroot=tools/zig_golden.zig -Mzignal=<zignal checkout>/src/root.zig > tests/golden/zig_golden.json
//!     python -m pytest tests/test_zig_golden.py -q          # skipped while the file is absent
//!
//! (The zignal module is what the `matcher` and `hough` sections call; every other section is std only.)
//!
//! (ReleaseFast is what the reference's own CI and examples build with; Debug must give the same bits — none of this is fast-math.)
//! Std only but for the matcher section: every expression below is the reference's own, restated with its file:line, so the numbers are those zignal computes
//! with this compiler — the same @exp, @sin, @cos, std.math.pow and std.math.cbrt calls on the same operands in the same order.
//! Every f32 travels as the u32 of its bit pattern; sweeps carry their inputs, so the checker never has to re-derive them.
//!
//! Sections of the JSON object:
//!   gamma_to_linear         256 x gammaToLinear(f32, i / 255)                  src/color.zig:1252-1258 (+ :365-373 for the / 255)
//!   lanczos3_lut_comptime   1025 x lanczosKernel(i / (1024 / 3), 3) at comptime  src/image/interpolation.zig:245-267 (the table the library takes in zg_method.lanczos_lut)
//!   lanczos3_lut_runtime    the same expression at run time (compiler-rt's sinf; shows whether comptime and run-time @sin agree)
//!   gaussian_taps           gaussianBlur's normalised taps for a sigma sweep   src/image.zig:973-990
//!   lanczos_plane_weights   resizePlaneLanczosU8's six weights per destination column, 4096 -> 1500 and 640 -> 1000   src/image/channel_ops.zig:446-466
//!   oklab_17 / lab_17       Rgb(u8) on the 17^3 lattice {0, 16, ..., 240, 255}^3 -> Oklab(f32) / Lab(f32)   src/color.zig:1261-1272, 1289-1310, 1381-1400
//!   orb                     ORB's orientation weight table at comptime (961), atan2 in degrees on a sweep [y, x, degrees], cos / sin of
//!                           degrees on a sweep [degrees, cos, sin]             src/features/orb.zig:340-357, 424-425, 432-433
//!   matcher                 BruteForceMatcher.match / knnMatch / radiusMatch of the zignal module itself on clustered descriptors with
//!                           tied distances; each case carries its inputs [query bytes, train bytes] and parameters. Pins what a
//!                           restatement cannot: that std.mem.sort keeps equal distances in train order   src/features/matcher.zig:44-212
//!   hough                   HoughTransform of the zignal module itself: the cos / sin tables of init for sizes with and without a quarter
//!                           point (the entries that rest on the last bit of Zig's f64 @cos / @sin), then compute and findLines on
//!                           random edges, inputs included; the all-zero accumulator pins std.mem.sort's order of equal scores   src/image/hough.zig:38-257
//!   flood_fill              Image(T).floodFill of the zignal module itself on patchy frames of u8, f32, Rgb(u8) and Rgba(f32) past 64 pixels
//!                           in both directions: every case carries its pixels as bytes, the seed, the options (the threshold as f64
//!                           bits, the exact square root of a sum of squares and the f64 below it among them), the fill value and the
//!                           filled image   src/image/flood_fill.zig:28-131
//!   metrics                 generateSsimWindow's 121 f64 weights at comptime and at run time (u64 bit patterns), @exp of an f64 at the
//!                           window's 20 distinct arguments and std.math.log10 of an f64 on a sweep of mse-like values, as [input
//!                           bits, output bits]: what zg_ssim_window_host and zg_psnr_from_mse restate   src/image/metrics.zig:53, 230-249
//!   exp / sin / cos / cbrt / pow24 / pow_third / pow_inv24   [input, output] pairs over the argument ranges the path uses
const std = @import("std");
const builtin = @import("builtin");
const zignal = @import("zignal"); // the matcher, hough, flood_fill and quantize sections alone

fn bits(x: f32) u32 {
    return @bitCast(x);
}

// ---- src/color.zig:84-89, 74-81 -----------------------------------------------------------------------------------------
const srgb_gamma_threshold = 0.04045;
const srgb_gamma_offset = 0.055;
const srgb_gamma_scale = 1.055;
const srgb_linear_slope = 12.92;
const srgb_gamma_exponent = 2.4;
const d65_x = 95.047;
const d65_y = 100.000;
const d65_z = 108.883;
const lab_epsilon = 0.008856;
const lab_kappa_div_116 = 7.787;
const lab_delta = 16.0 / 116.0;
const pow = std.math.pow;

/// src/color.zig:1252-1258
fn gammaToLinear(comptime T: type, c: T) T {
    return if (c > srgb_gamma_threshold)
        pow(T, (c + srgb_gamma_offset) / srgb_gamma_scale, srgb_gamma_exponent)
    else
        c / srgb_linear_slope;
}

const Xyz = struct { x: f32, y: f32, z: f32 };

/// src/color.zig:365-373 (Rgb(u8).as(f32): @as(U, self.r) / 255) then :1261-1272
fn rgbToXyz(r8: u8, g8: u8, b8: u8) Xyz {
    const T = f32;
    const r = gammaToLinear(T, @as(T, @floatFromInt(r8)) / 255);
    const g = gammaToLinear(T, @as(T, @floatFromInt(g8)) / 255);
    const b = gammaToLinear(T, @as(T, @floatFromInt(b8)) / 255);
    return .{
        .x = (r * 0.4124 + g * 0.3576 + b * 0.1805) * 100,
        .y = (r * 0.2126 + g * 0.7152 + b * 0.0722) * 100,
        .z = (r * 0.0193 + g * 0.1192 + b * 0.9505) * 100,
    };
}

/// src/color.zig:1381-1400
fn xyzToOklab(xyz: Xyz) [3]f32 {
    const x = xyz.x / 100.0;
    const y = xyz.y / 100.0;
    const z = xyz.z / 100.0;
    const l_linear = 0.8189330101 * x + 0.3618667424 * y - 0.1288597137 * z;
    const m_linear = 0.0329845436 * x + 0.9293118715 * y + 0.0361456387 * z;
    const s_linear = 0.0482003018 * x + 0.2643662691 * y + 0.6338517070 * z;
    const l_dash = std.math.cbrt(l_linear);
    const m_dash = std.math.cbrt(m_linear);
    const s_dash = std.math.cbrt(s_linear);
    return .{
        0.2104542553 * l_dash + 0.7936177850 * m_dash - 0.0040720468 * s_dash,
        1.9779984951 * l_dash - 2.4285922050 * m_dash + 0.4505937099 * s_dash,
        0.0259040371 * l_dash + 0.7827717662 * m_dash - 0.8086757660 * s_dash,
    };
}

/// src/color.zig:1289-1291
fn labForward(comptime T: type, t: T) T {
    return if (t > lab_epsilon) pow(T, t, 1.0 / 3.0) else lab_kappa_div_116 * t + lab_delta;
}

/// src/color.zig:1294-1310
fn xyzToLab(xyz: Xyz) [3]f32 {
    const T = f32;
    const fx = labForward(T, xyz.x / d65_x);
    const fy = labForward(T, xyz.y / d65_y);
    const fz = labForward(T, xyz.z / d65_z);
    return .{ @max(0, 116.0 * fy - 16.0), 500.0 * (fx - fy), 200.0 * (fy - fz) };
}

/// src/image/interpolation.zig:245-252
fn lanczosKernel(x: f32, a: f32) f32 {
    if (x == 0) return 1;
    if (@abs(x) >= a) return 0;
    const pi_x = std.math.pi * x;
    const pi_x_over_a = pi_x / a;
    return (a * @sin(pi_x) * @sin(pi_x_over_a)) / (pi_x * pi_x);
}

/// src/image/interpolation.zig:255-267, verbatim: evaluated by the COMPILER
const lanczos3_lut: [1025]f32 = blk: {
    const size = 1024;
    const max_dist: f32 = 3.0;
    const step = size / max_dist;
    @setEvalBranchQuota(40000);
    var vals: [size + 1]f32 = undefined;
    for (0..1025) |i| {
        const x = @as(f32, @floatFromInt(i)) / step;
        vals[i] = lanczosKernel(x, 3.0);
    }
    break :blk vals;
};

/// src/image/channel_ops.zig:446-454
fn lanczosPlaneKernel(x: f32) f32 {
    if (x == 0) return 1.0;
    const a = 3.0;
    if (@abs(x) >= a) return 0.0;
    const pi_x = std.math.pi * x;
    return (a * @sin(pi_x) * @sin(pi_x / a)) / (pi_x * pi_x);
}

// A run-time value the optimiser cannot fold: the sweeps and tables below must be computed by the generated code, not by the compiler.
fn runtime(x: f32) f32 {
    var v = x;
    std.mem.doNotOptimizeAway(&v);
    return v;
}

const Lcg = struct {
    s: u32,
    fn next(self: *Lcg) u32 {
        self.s = self.s *% 1664525 +% 1013904223;
        return self.s;
    }
    /// uniform in [lo, hi): a 24-bit fraction, one multiply and one add in f32
    fn uniform(self: *Lcg, lo: f32, hi: f32) f32 {
        const u = @as(f32, @floatFromInt(self.next() >> 8)) * (1.0 / 16777216.0);
        return lo + u * (hi - lo);
    }
};

fn sweep(w: anytype, comptime name: []const u8, comptime f: fn (f32) f32, seed: u32, lo: f32, hi: f32, n: usize, last: bool) !void {
    var rng = Lcg{ .s = seed };
    try w.print("  \"{s}\": [", .{name});
    for (0..n) |i| {
        const x = runtime(rng.uniform(lo, hi));
        try w.print("{s}[{d},{d}]", .{ if (i == 0) "" else ",", bits(x), bits(f(x)) });
    }
    try w.print("]{s}\n", .{if (last) "" else ","});
}

fn fExp(x: f32) f32 {
    return @exp(x);
}
fn fSin(x: f32) f32 {
    return @sin(x);
}
fn fCos(x: f32) f32 {
    return @cos(x);
}
fn fCbrt(x: f32) f32 {
    return std.math.cbrt(x);
}
fn fPow24(x: f32) f32 {
    return pow(f32, x, srgb_gamma_exponent);
}
fn fPowThird(x: f32) f32 {
    return pow(f32, x, 1.0 / 3.0);
}
fn fPowInv24(x: f32) f32 {
    return pow(f32, x, 1.0 / srgb_gamma_exponent);
}

/// src/features/orb.zig:340-357: exp(-d^2 / (225 / 2)) inside d^2 <= 225, at comptime
const orb_weights: [31 * 31]f32 = blk: {
    @setEvalBranchQuota(100_000);
    var vals: [31 * 31]f32 = @splat(0);
    const radius_sq: f32 = 225.0;
    const denom: f32 = radius_sq / 2.0;
    for (0..31) |v| {
        for (0..31) |u| {
            const dy: i32 = @as(i32, @intCast(v)) - 15;
            const dx: i32 = @as(i32, @intCast(u)) - 15;
            const dist_sq: f32 = @floatFromInt(dx * dx + dy * dy);
            if (dist_sq <= radius_sq) vals[v * 31 + u] = @exp(-dist_sq / denom);
        }
    }
    break :blk vals;
};

// ---- matcher: the reference's own BruteForceMatcher on inputs made here --------------------------------------------------------
fn flipBits(d: *zignal.BinaryDescriptor, rng: *Lcg, n: u32) void {
    for (0..n) |_| {
        const b = rng.next() >> 24; // a bit may be hit twice: the distances that result are what the section records
        d.bits[b / 8] ^= @as(u8, 1) << @as(u3, @intCast(b % 8));
    }
}

/// Random train descriptors, a tenth of them copies or near copies of an earlier one; queries that are train entries with
/// 0 .. 90 bits flipped, or random, a tenth of them copies of an earlier query: ties at every distance the tests look at.
fn clusteredDescriptors(rng: *Lcg, query: []zignal.BinaryDescriptor, train: []zignal.BinaryDescriptor) void {
    const flips = [_]u32{ 0, 3, 10, 30, 60, 64, 65, 90 };
    for (train, 0..) |*t, i| {
        for (&t.bits) |*b| b.* = @intCast(rng.next() >> 24);
        if (i > 0 and rng.next() % 10 == 0) {
            t.* = train[rng.next() % i];
            if (rng.next() % 2 == 1) flipBits(t, rng, rng.next() % 39 + 1);
        }
    }
    for (query, 0..) |*q, i| {
        for (&q.bits) |*b| b.* = @intCast(rng.next() >> 24);
        if (rng.next() % 5 != 0) {
            q.* = train[rng.next() % train.len];
            flipBits(q, rng, flips[rng.next() % flips.len]);
        }
        if (i > 0 and rng.next() % 10 == 0) q.* = query[rng.next() % i];
    }
}

fn printDescriptors(w: anytype, ds: []const zignal.BinaryDescriptor) !void {
    try w.print("[", .{});
    for (ds, 0..) |d, i| {
        for (d.bits, 0..) |b, j| try w.print("{s}{d}", .{ if (i == 0 and j == 0) "" else ",", b });
    }
    try w.print("]", .{});
}

fn printMatches(w: anytype, ms: anytype) !void {
    try w.print("[", .{});
    for (ms, 0..) |m, i| try w.print("{s}[{d},{d},{d}]", .{ if (i == 0) "" else ",", m.query_idx, m.train_idx, bits(m.distance) });
    try w.print("]", .{});
}

fn printRows(w: anytype, allocator: std.mem.Allocator, rows: anytype) !void {
    try w.print("[", .{});
    for (rows, 0..) |row, i| {
        if (i != 0) try w.print(",", .{});
        try printMatches(w, row);
        allocator.free(row);
    }
    allocator.free(rows);
    try w.print("]", .{});
}

fn matcherSection(w: anytype, allocator: std.mem.Allocator) !void {
    const shapes = [_][2]usize{ .{ 1, 1 }, .{ 5, 1 }, .{ 9, 40 }, .{ 65, 129 }, .{ 40, 300 } };
    const ratios = [_]f32{ 0.8, 0.5, 1.0, 2.0, 0.0, std.math.inf(f32), std.math.nan(f32), -1.0 };
    const max_distances = [_]u32{ 0, 64, 256, std.math.maxInt(u32) };
    const radii = [_]f32{ -1.0, 0.0, 40.0, 64.5, 300.0, std.math.nan(f32) };
    try w.print("  \"matcher\": [", .{});
    for (shapes, 0..) |shape, si| {
        var rng = Lcg{ .s = 40 + @as(u32, @intCast(si)) };
        const query = try allocator.alloc(zignal.BinaryDescriptor, shape[0]);
        defer allocator.free(query);
        const train = try allocator.alloc(zignal.BinaryDescriptor, shape[1]);
        defer allocator.free(train);
        clusteredDescriptors(&rng, query, train);
        try w.print("{s}\n   {{\"nq\": {d}, \"nt\": {d}, \"query\": ", .{ if (si == 0) "" else ",", shape[0], shape[1] });
        try printDescriptors(w, query);
        try w.print(", \"train\": ", .{});
        try printDescriptors(w, train);
        try w.print(", \"match\": [", .{});
        var first = true;
        for ([_]bool{ false, true }) |cross| for (max_distances) |md| for (ratios) |ratio| {
            const m = zignal.BruteForceMatcher{ .cross_check = cross, .max_distance = md, .ratio_threshold = runtime(ratio) };
            const got = try m.match(allocator, query, train);
            defer allocator.free(got);
            try w.print("{s}{{\"cross_check\": {d}, \"max_distance\": {d}, \"ratio_bits\": {d}, \"matches\": ", .{ if (first) "" else ",", @intFromBool(cross), md, bits(ratio) });
            try printMatches(w, got);
            try w.print("}}", .{});
            first = false;
        };
        try w.print("], \"knn\": [", .{});
        first = true;
        for ([_]usize{ 1, 2, 3, shape[1], shape[1] + 5 }) |k| for (max_distances) |md| {
            const m = zignal.BruteForceMatcher{ .max_distance = md };
            try w.print("{s}{{\"k\": {d}, \"max_distance\": {d}, \"rows\": ", .{ if (first) "" else ",", k, md });
            try printRows(w, allocator, try m.knnMatch(allocator, query, train, k));
            try w.print("}}", .{});
            first = false;
        };
        try w.print("], \"radius\": [", .{});
        for (radii, 0..) |r, ri| {
            const m = zignal.BruteForceMatcher{};
            try w.print("{s}{{\"max_dist_bits\": {d}, \"rows\": ", .{ if (ri == 0) "" else ",", bits(r) });
            try printRows(w, allocator, try m.radiusMatch(allocator, query, train, runtime(r)));
            try w.print("}}", .{});
        }
        try w.print("]}}", .{});
    }
    try w.print("\n  ],\n", .{});
}

// ---- hough: the reference's own HoughTransform on inputs made here -------------------------------------------------------------
fn printLines(w: anytype, lines: []const zignal.HoughTransform.Line) !void {
    try w.print("[", .{});
    for (lines, 0..) |l, i| try w.print("{s}[{d},{d},{d},{d},{d},{d},{d}]", .{ if (i == 0) "" else ",", bits(l.angle), bits(l.radius), l.score, bits(l.p1.x()), bits(l.p1.y()), bits(l.p2.x()), bits(l.p2.y()) });
    try w.print("]", .{});
}

/// The tables of init for sizes with and without a quarter point (the only entries the last bit of @cos / @sin can move), then
/// compute and findLines on random edges with three values, a box past the image's edge, and the all-zero tie-order accumulator.
fn houghSection(w: anytype, allocator: std.mem.Allocator) !void {
    const table_sizes = [_]u32{ 2, 3, 4, 5, 8, 9, 63, 64, 97, 126, 128, 130, 220, 250, 256, 300, 512, 1024, 2048 };
    try w.print("  \"hough\": {{\"tables\": [", .{});
    for (table_sizes, 0..) |size, si| {
        var h = try zignal.HoughTransform.init(allocator, size);
        defer h.deinit();
        try w.print("{s}\n   {{\"size\": {d}, \"cos\": [", .{ if (si == 0) "" else ",", size });
        for (h.cos_table, 0..) |v, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", v });
        try w.print("], \"sin\": [", .{});
        for (h.sin_table, 0..) |v, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", v });
        try w.print("]}}", .{});
    }
    try w.print("\n  ], \"cases\": [", .{});
    // size, image rows, image cols, box l, box t, one edge pixel in `sparsity`
    const shapes = [_][6]u32{ .{ 2, 2, 2, 0, 0, 2 }, .{ 5, 5, 5, 0, 0, 2 }, .{ 9, 9, 9, 0, 0, 0 }, .{ 63, 70, 66, 2, 3, 8 }, .{ 64, 64, 64, 0, 0, 16 }, .{ 97, 110, 120, 20, 30, 24 } };
    const nms = [_][2]f32{ .{ 10.0, 5.0 }, .{ 5.0, 5.0 }, .{ std.math.nan(f32), 5.0 }, .{ -1.0, -1.0 }, .{ std.math.inf(f32), std.math.inf(f32) }, .{ 180.0, 1.5 } };
    for (shapes, 0..) |shape, si| {
        var rng = Lcg{ .s = 60 + @as(u32, @intCast(si)) };
        const size = shape[0];
        var edges: zignal.Image(u8) = try .init(allocator, shape[1], shape[2]);
        defer edges.deinit(allocator);
        const values = [_]u8{ 1, 128, 255 };
        for (edges.data) |*e| e.* = if (shape[5] != 0 and rng.next() % shape[5] == 0) values[rng.next() % 3] else 0; // sparsity 0: no edge at all, the tie-order case
        var h = try zignal.HoughTransform.init(allocator, size);
        defer h.deinit();
        var acc: zignal.Image(u32) = try .init(allocator, size, size);
        defer acc.deinit(allocator);
        acc.fill(0);
        h.compute(edges, .{ .l = shape[3], .t = shape[4], .r = shape[3] + size, .b = shape[4] + size }, acc);
        try w.print("{s}\n   {{\"size\": {d}, \"rows\": {d}, \"cols\": {d}, \"box\": [{d},{d},{d},{d}], \"edges\": [", .{ if (si == 0) "" else ",", size, shape[1], shape[2], shape[3], shape[4], shape[3] + size, shape[4] + size });
        for (edges.data, 0..) |e, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", e });
        try w.print("], \"accumulator\": [", .{});
        var max: u32 = 0;
        for (acc.data, 0..) |v, i| {
            try w.print("{s}{d}", .{ if (i == 0) "" else ",", v });
            max = @max(max, v);
        }
        try w.print("], \"finds\": [", .{});
        var first = true;
        for ([_]u32{ 0, @max(1, max / 2), max + 1 }) |threshold| for (nms) |pair| {
            const lines = try h.findLines(allocator, acc, threshold, runtime(pair[0]), runtime(pair[1]));
            defer allocator.free(lines);
            try w.print("{s}{{\"threshold\": {d}, \"angle_bits\": {d}, \"radius_bits\": {d}, \"lines\": ", .{ if (first) "" else ",", threshold, bits(pair[0]), bits(pair[1]) });
            try printLines(w, lines);
            try w.print("}}", .{});
            first = false;
        };
        try w.print("]}}", .{});
    }
    try w.print("\n  ]}},\n", .{});
}

// ---- flood_fill: the reference's own Image(T).floodFill on inputs made here --------------------------------------------------------
fn printBytes(w: anytype, bytes: []const u8) !void {
    try w.print("[", .{});
    for (bytes, 0..) |b, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", b });
    try w.print("]", .{});
}

fn floodValue(comptime T: type, v: u32) T {
    return switch (T) {
        u8 => @intCast(100 + v),
        f32 => 0.25 * @as(f32, @floatFromInt(v)),
        zignal.Rgb(u8) => .{ .r = @intCast(100 + v), .g = 7, .b = @intCast(50 + (v & 1)) },
        zignal.Rgba(f32) => .{ .r = 0.5, .g = 0.125 * @as(f32, @floatFromInt(v)), .b = 0.75, .a = 0.25 * @as(f32, @floatFromInt(v & 1)) },
        else => unreachable,
    };
}

/// One pixel type: patches three pixels wide of four levels with a tenth of the pixels redrawn, every threshold with both modes and
/// both connectivities from a seed next to the corner of the first 64 x 64 tile.
fn floodCases(comptime T: type, comptime name: []const u8, w: anytype, allocator: std.mem.Allocator, seed: u32, thresholds: []const f64, fill_value: T, first: *bool) !void {
    const rows: u32 = 73;
    const cols: u32 = 133;
    var rng = Lcg{ .s = seed };
    var src: zignal.Image(T) = try .init(allocator, rows, cols);
    defer src.deinit(allocator);
    var coarse: [(rows / 3 + 1) * (cols / 3 + 1)]u32 = undefined;
    for (&coarse) |*v| v.* = rng.next() % 4;
    for (0..rows) |r| for (0..cols) |c| {
        src.at(r, c).* = floodValue(T, if (rng.next() % 10 == 0) rng.next() % 4 else coarse[(r / 3) * (cols / 3 + 1) + c / 3]);
    };
    try w.print("{s}\n   {{\"pixel\": \"{s}\", \"rows\": {d}, \"cols\": {d}, \"data\": ", .{ if (first.*) "" else ",", name, rows, cols });
    first.* = false;
    try printBytes(w, std.mem.sliceAsBytes(src.data));
    try w.print(", \"fill\": ", .{});
    try printBytes(w, std.mem.asBytes(&fill_value)[0..@sizeOf(T)]);
    try w.print(", \"fills\": [", .{});
    var first_fill = true;
    for (thresholds) |threshold| for ([_]zignal.FloodFillOptions.ThresholdMode{ .seed, .neighbor }, 0..) |mode, mi| for ([_]zignal.FloodFillOptions.Connectivity{ .four, .eight }) |connectivity| {
        var img = try src.dupe(allocator);
        defer img.deinit(allocator);
        try img.floodFill(allocator, 63, 64, fill_value, .{ .threshold = threshold, .connectivity = connectivity, .mode = mode });
        try w.print("{s}\n    {{\"row\": 63, \"col\": 64, \"threshold_bits\": {d}, \"connectivity\": {d}, \"mode\": {d}, \"out\": ", .{ if (first_fill) "" else ",", @as(u64, @bitCast(threshold)), @intFromEnum(connectivity), mi });
        try printBytes(w, std.mem.sliceAsBytes(img.data));
        try w.print("}}", .{});
        first_fill = false;
    };
    try w.print("]}}", .{});
}

fn floodSection(w: anytype, allocator: std.mem.Allocator) !void {
    try w.print("  \"flood_fill\": [", .{});
    var first = true;
    const nan = std.math.nan(f64);
    const inf = std.math.inf(f64);
    const root2 = @sqrt(@as(f64, 2.0)); // Rgb(u8): r differs by 1 and b by 1
    const step = @sqrt(@as(f64, 0.125 * 0.125 + 0.25 * 0.25)); // Rgba(f32): g differs by 0.125 and a by 0.25
    try floodCases(u8, "u8", w, allocator, 81, &.{ 0.0, 1.0, 1.5, -0.0, -1.0, nan, inf }, 7, &first);
    try floodCases(f32, "f32", w, allocator, 82, &.{ 0.0, 0.25, std.math.nextAfter(f64, 0.25, 0.0), inf }, -3.5, &first);
    try floodCases(zignal.Rgb(u8), "rgb_u8", w, allocator, 83, &.{ 0.0, root2, std.math.nextAfter(f64, root2, 0.0), 2.0, nan }, .{ .r = 1, .g = 2, .b = 3 }, &first);
    try floodCases(zignal.Rgba(f32), "rgba_f32", w, allocator, 84, &.{ 0.0, step, std.math.nextAfter(f64, step, 0.0), inf }, .{ .r = -1, .g = -2, .b = -3, .a = -4 }, &first);
    try w.print("\n  ],\n", .{});
}

// ---- quantize: the reference's own medianCut and error diffusion on inputs made here ------------------------------------------------
/// Frames with few distinct values per channel: every sort of medianCut meets long runs of equal keys, which is where the order that
/// std.sort.heap (unstable) leaves shows in the palette. Then both diffusion modes on noise against the two-grey palette.
fn quantizeSection(w: anytype, allocator: std.mem.Allocator) !void {
    const Rgb = zignal.Rgb(u8);
    const levels = [_]u8{ 0, 8, 64, 72, 200, 248 };
    try w.print("  \"quantize\": {{\"median_cut\": [", .{});
    var first = true;
    for ([_]u32{ 101, 102, 103 }, [_]u32{ 48, 31, 64 }, [_]u32{ 48, 77, 64 }, [_]bool{ true, true, false }) |seed, rows, cols, few| {
        var rng = Lcg{ .s = seed };
        var img: zignal.Image(Rgb) = try .init(allocator, rows, cols);
        defer img.deinit(allocator);
        for (img.data) |*p| {
            p.* = if (few)
                Rgb{ .r = levels[(rng.next() >> 16) % 6], .g = levels[(rng.next() >> 16) % 6], .b = levels[(rng.next() >> 16) % 6] }
            else
                Rgb{ .r = @intCast(rng.next() >> 24), .g = @intCast(rng.next() >> 24), .b = @intCast(rng.next() >> 24) };
        }
        try w.print("{s}\n   {{\"rows\": {d}, \"cols\": {d}, \"data\": ", .{ if (first) "" else ",", rows, cols });
        first = false;
        try printBytes(w, std.mem.sliceAsBytes(img.data));
        try w.print(", \"palettes\": [", .{});
        for ([_]u16{ 2, 5, 16, 64, 256 }, 0..) |max_colors, i| {
            var palette: [256]Rgb = undefined;
            const n = try zignal.quantize.medianCut(Rgb, allocator, img, &palette, max_colors);
            try w.print("{s}{{\"max_colors\": {d}, \"palette\": ", .{ if (i == 0) "" else ", ", max_colors });
            try printBytes(w, std.mem.sliceAsBytes(palette[0..n]));
            try w.print("}}", .{});
        }
        try w.print("]}}", .{});
    }
    try w.print("\n  ], \"dither\": [", .{});
    const greys = [_]Rgb{ .{ .r = 64, .g = 64, .b = 64 }, .{ .r = 192, .g = 192, .b = 192 } };
    const lut: zignal.quantize.ColorLookupTable = .init(&greys);
    first = true;
    for ([_]zignal.dither.Mode{ .floyd_steinberg, .atkinson, .ordered }) |mode| {
        var rng = Lcg{ .s = 104 };
        var img: zignal.Image(Rgb) = try .init(allocator, 37, 53);
        defer img.deinit(allocator);
        for (img.data) |*p| p.* = .{ .r = @intCast(rng.next() >> 24), .g = @intCast(rng.next() >> 24), .b = @intCast(rng.next() >> 24) };
        try w.print("{s}\n   {{\"mode\": {d}, \"rows\": 37, \"cols\": 53, \"data\": ", .{ if (first) "" else ",", @intFromEnum(mode) });
        first = false;
        try printBytes(w, std.mem.sliceAsBytes(img.data));
        zignal.dither.apply(img, &greys, lut, mode);
        try w.print(", \"out\": ", .{});
        try printBytes(w, std.mem.sliceAsBytes(img.data));
        try w.print("}}", .{});
    }
    try w.print("\n  ]}},\n", .{});
}

// ---- metrics: the host arithmetic of psnr and ssim in f64 -----------------------------------------------------------------------------
fn runtime64(x: f64) f64 {
    var v = x;
    std.mem.doNotOptimizeAway(&v);
    return v;
}

/// src/image/metrics.zig:230-249; `at_runtime` keeps the compiler from folding the exponentials
fn ssimWindow(at_runtime: bool) [121]f64 {
    const sigma: f64 = 1.5;
    var window: [121]f64 = undefined;
    var sum: f64 = 0.0;
    for (0..11) |dy| {
        for (0..11) |dx| {
            const y: f64 = @as(f64, @floatFromInt(dy)) - 5.0;
            const x: f64 = @as(f64, @floatFromInt(dx)) - 5.0;
            const arg = -(x * x + y * y) / (2.0 * sigma * sigma);
            const gauss = @exp(if (at_runtime) runtime64(arg) else arg);
            window[dy * 11 + dx] = gauss;
            sum += gauss;
        }
    }
    for (&window) |*v| v.* /= sum;
    return window;
}

const ssim_window_comptime = blk: {
    @setEvalBranchQuota(20000);
    break :blk ssimWindow(false);
};

fn metricsSection(w: anytype) !void {
    try w.print("  \"metrics\": {{\"ssim_window_comptime\": [", .{});
    for (ssim_window_comptime, 0..) |v, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", @as(u64, @bitCast(v)) });
    try w.print("], \"ssim_window_runtime\": [", .{});
    for (ssimWindow(true), 0..) |v, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", @as(u64, @bitCast(v)) });
    try w.print("], \"exp\": [", .{});
    var first = true;
    for (0..6) |yi| for (yi..6) |xi| {
        const x: f64 = @floatFromInt(xi);
        const y: f64 = @floatFromInt(yi);
        const arg = runtime64(-(x * x + y * y) / (2.0 * 1.5 * 1.5));
        try w.print("{s}[{d},{d}]", .{ if (first) "" else ",", @as(u64, @bitCast(arg)), @as(u64, @bitCast(@exp(arg))) });
        first = false;
    };
    try w.print("], \"log10\": [", .{});
    var rng = Lcg{ .s = 91 };
    for (0..4096) |i| {
        // mse-like values from 1e-12 to 65025, the component maxima, and values around 1
        const u = @as(f64, @floatFromInt(rng.next() >> 8)) / 16777216.0;
        const x = runtime64(switch (i % 4) {
            0 => 65025.0 * u,
            1 => std.math.pow(f64, 10.0, -12.0 + 17.0 * u),
            2 => 0.5 + 1.5 * u,
            else => if (i == 3) 255.0 else if (i == 7) 1.0 else 255.0 * u,
        });
        try w.print("{s}[{d},{d}]", .{ if (i == 0) "" else ",", @as(u64, @bitCast(x)), @as(u64, @bitCast(std.math.log10(x))) });
    }
    try w.print("]}},\n", .{});
}

pub fn main(init: std.process.Init) !void {
    var buffer: [1 << 16]u8 = undefined;
    var stdout = std.Io.File.stdout().writer(init.io, &buffer);
    const w = &stdout.interface;

    try w.print("{{\n  \"zig_version\": \"{s}\",\n  \"optimize\": \"{s}\",\n", .{ builtin.zig_version_string, @tagName(builtin.mode) });

    try w.print("  \"gamma_to_linear\": [", .{});
    for (0..256) |i| {
        const c = runtime(@as(f32, @floatFromInt(i))) / 255;
        try w.print("{s}{d}", .{ if (i == 0) "" else ",", bits(gammaToLinear(f32, c)) });
    }
    try w.print("],\n  \"lanczos3_lut_comptime\": [", .{});
    for (lanczos3_lut, 0..) |v, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", bits(v) });
    try w.print("],\n  \"lanczos3_lut_runtime\": [", .{});
    {
        const step = runtime(1024.0) / runtime(3.0);
        for (0..1025) |i| {
            const x = runtime(@as(f32, @floatFromInt(i))) / step;
            try w.print("{s}{d}", .{ if (i == 0) "" else ",", bits(lanczosKernel(x, 3.0)) });
        }
    }

    // src/image.zig:973-990
    try w.print("],\n  \"gaussian_taps\": {{", .{});
    const sigmas = [_]f32{ 0.3, 0.5, 0.6, 0.75, 1.0, 1.2, 1.4, 1.6, 2.0, 2.5, 3.0, 4.0, 5.5 };
    for (sigmas, 0..) |sigma_c, si| {
        const sigma = runtime(sigma_c);
        const radius: usize = @ceil(3.0 * sigma); // as the reference writes it (src/image.zig:973)
        const kernel_size = 2 * radius + 1;
        var kernel: [64]f32 = undefined;
        var sum: f32 = 0;
        for (0..kernel_size) |i| {
            const x = @as(f32, @floatFromInt(i)) - @as(f32, @floatFromInt(radius));
            kernel[i] = @exp(-(x * x) / (2.0 * sigma * sigma));
            sum += kernel[i];
        }
        for (kernel[0..kernel_size]) |*k| k.* /= sum;
        try w.print("{s}\"{d}\": [", .{ if (si == 0) "" else ", ", bits(sigma) });
        for (kernel[0..kernel_size], 0..) |k, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", bits(k) });
        try w.print("]", .{});
    }

    // src/image/channel_ops.zig:456-466: x_ratio in f32, src_x_f = (c + 0.5) * x_ratio - 0.5, fx = src_x_f - floor, weight k = kernel((k - 2) - fx)
    try w.print("}},\n  \"lanczos_plane_weights\": {{", .{});
    const geometries = [_][2]u32{ .{ 4096, 1500 }, .{ 640, 1000 } };
    for (geometries, 0..) |g, gi| {
        const ratio = runtime(@as(f32, @floatFromInt(g[0]))) / @as(f32, @floatFromInt(g[1]));
        try w.print("{s}\"{d}x{d}\": [", .{ if (gi == 0) "" else ", ", g[0], g[1] });
        for (0..g[1]) |c| {
            const src_x_f = (@as(f32, @floatFromInt(c)) + 0.5) * ratio - 0.5;
            const fx = src_x_f - @floor(src_x_f);
            for (0..6) |k| {
                const wk = lanczosPlaneKernel(@as(f32, @floatFromInt(@as(isize, @intCast(k)) - 2)) - fx);
                try w.print("{s}{d}", .{ if (c == 0 and k == 0) "" else ",", bits(wk) });
            }
        }
        try w.print("]", .{});
    }

    try w.print("}},\n  \"oklab_17\": [", .{});
    for (0..17) |ri| for (0..17) |gi| for (0..17) |bi| {
        const r: u8 = @intCast(@min(ri * 16, 255));
        const g: u8 = @intCast(@min(gi * 16, 255));
        const b: u8 = @intCast(@min(bi * 16, 255));
        const lab = xyzToOklab(rgbToXyz(r, g, b));
        try w.print("{s}{d},{d},{d}", .{ if (ri + gi + bi == 0) "" else ",", bits(lab[0]), bits(lab[1]), bits(lab[2]) });
    };
    try w.print("],\n  \"lab_17\": [", .{});
    for (0..17) |ri| for (0..17) |gi| for (0..17) |bi| {
        const r: u8 = @intCast(@min(ri * 16, 255));
        const g: u8 = @intCast(@min(gi * 16, 255));
        const b: u8 = @intCast(@min(bi * 16, 255));
        const lab = xyzToLab(rgbToXyz(r, g, b));
        try w.print("{s}{d},{d},{d}", .{ if (ri + gi + bi == 0) "" else ",", bits(lab[0]), bits(lab[1]), bits(lab[2]) });
    };
    try w.print("],\n", .{});

    // the argument ranges the path uses: Gaussian tap exponents; rotation angles and pi * x of the Lanczos kernels; LMS values;
    // (c + 0.055) / 1.055 of gammaToLinear; t of labForward; c of linearToGamma
    try sweep(w, "exp", fExp, 11, -90.0, 0.0, 4096, false);
    try sweep(w, "sin", fSin, 12, -12.0, 12.0, 4096, false);
    try sweep(w, "cos", fCos, 13, -12.0, 12.0, 4096, false);
    try sweep(w, "cbrt", fCbrt, 14, 0.0, 1.2, 4096, false);
    try sweep(w, "pow24", fPow24, 15, 0.0404, 1.0, 4096, false);
    try sweep(w, "pow_third", fPowThird, 16, 0.008856, 1.1, 4096, false);
    try sweep(w, "pow_inv24", fPowInv24, 17, 0.0031308, 1.0, 4096, false);

    // src/features/matcher.zig:44-212 through the zignal module
    try matcherSection(w, init.gpa);

    // src/image/hough.zig:38-257 through the zignal module
    try houghSection(w, init.gpa);

    // src/image/flood_fill.zig:28-131 through the zignal module
    try floodSection(w, init.gpa);

    // src/image/metrics.zig:53, 230-249
    try metricsSection(w);

    // src/image/quantize.zig:175-412 and src/image/dither.zig:34-331 through the zignal module
    try quantizeSection(w, init.gpa);

    // src/features/orb.zig:340-357 (the table), :424-425 (radiansToDegrees(atan2(m01 / m00, m10 / m00)): centroid offsets lie within the
    // 15-pixel patch), :432-433 (@cos / @sin of degreesToRadians(angle), angle in [-180, 180])
    try w.print("  \"orb\": {{\"weights\": [", .{});
    for (orb_weights, 0..) |v, i| try w.print("{s}{d}", .{ if (i == 0) "" else ",", bits(v) });
    try w.print("], \"atan2_degrees\": [", .{});
    {
        var rng = Lcg{ .s = 18 };
        for (0..4096) |i| {
            const y = runtime(rng.uniform(-15.0, 15.0));
            const x = runtime(rng.uniform(-15.0, 15.0));
            const deg = std.math.radiansToDegrees(std.math.atan2(y, x));
            try w.print("{s}[{d},{d},{d}]", .{ if (i == 0) "" else ",", bits(y), bits(x), bits(deg) });
        }
    }
    try w.print("], \"cos_sin_of_degrees\": [", .{});
    {
        var rng = Lcg{ .s = 19 };
        for (0..4096) |i| {
            const a = runtime(rng.uniform(-180.0, 180.0));
            const c = @cos(std.math.degreesToRadians(a));
            const sn = @sin(std.math.degreesToRadians(a));
            try w.print("{s}[{d},{d},{d}]", .{ if (i == 0) "" else ",", bits(a), bits(c), bits(sn) });
        }
    }
    try w.print("]}}\n", .{});
    try w.print("}}\n", .{});
    try w.flush();
}

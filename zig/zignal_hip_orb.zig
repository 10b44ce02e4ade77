//! zignal_hip_orb.zig — the ORB module of the shim: Orb.detect / compute / detectAndCompute (reference src/features/orb.zig) through
//! libzignal_hip.so's zg_orb_* entry points (include/zignal_hip_orb.h). Sits beside zignal_hip.zig and builds on its Image,
//! DeviceImage, KeyPoint and error mapping. Like that file it has not been compiled where the library is built (no Zig toolchain).
const std = @import("std");
const zignal = @import("zignal");
const hip = @import("zignal_hip.zig");

pub const KeyPoint = hip.KeyPoint;

pub const c = struct {
    pub const ZgBinaryDescriptor = extern struct { bits: [32]u8 }; // BinaryDescriptor.zig:10
    pub const ZgOrbParams = extern struct { n_features: u32, scale_factor: f32, n_levels: u32, edge_threshold: u32, first_level: u32, wta_k: u32, fast_threshold: u32, score_type: i32, orientation_weights: ?[*]const f32 }; // orb.zig:87-109
    pub extern fn zg_orb_default_params(params: *ZgOrbParams) void;
    pub extern fn zg_orb_features_per_level(params: *const ZgOrbParams, out: [*]u32) c_int;
    pub extern fn zg_orb_adaptive_threshold(params: *const ZgOrbParams, level: u32) c_int;
    pub extern fn zg_orb_detect_and_compute(src: *const hip.c.ZgImage, params: *const ZgOrbParams, keypoints: ?[*]hip.c.ZgKeypoint, descriptors: ?[*]ZgBinaryDescriptor, capacity: u32, count: *u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_orb_compute(src: *const hip.c.ZgImage, params: *const ZgOrbParams, keypoints: ?[*]const hip.c.ZgKeypoint, n: u32, descriptors: ?[*]ZgBinaryDescriptor, stream: ?*anyopaque) c_int;
    pub extern fn zg_orb_detect_and_compute_host(src: *const hip.c.ZgImage, params: *const ZgOrbParams, keypoints: ?[*]hip.c.ZgKeypoint, descriptors: ?[*]ZgBinaryDescriptor, capacity: u32, count: *u32) c_int;
    pub extern fn zg_orb_compute_host(src: *const hip.c.ZgImage, params: *const ZgOrbParams, keypoints: ?[*]const hip.c.ZgKeypoint, n: u32, descriptors: ?[*]ZgBinaryDescriptor) c_int;
};

// ---- features: ORB (reference src/features/orb.zig, BinaryDescriptor.zig) --------------------------------------------

/// BinaryDescriptor (src/features/BinaryDescriptor.zig:10) laid out as zg_binary_descriptor.
pub const BinaryDescriptor = c.ZgBinaryDescriptor;
comptime {
    std.debug.assert(@sizeOf(BinaryDescriptor) == 32);
}

/// Orb (src/features/orb.zig:87-109): same fields, same defaults; detect / compute / detectAndCompute return the reference's
/// arrays, order included. orientation_weights: null for the library's table, or this program's own 31 x 31 table (orb.zig:340-357).
pub const Orb = struct {
    n_features: usize = 500,
    scale_factor: f32 = 1.2,
    n_levels: u8 = 8,
    edge_threshold: u8 = 15,
    first_level: u8 = 0,
    wta_k: u8 = 2,
    fast_threshold: u8 = 20,
    score_type: ScoreType = .fast_score,
    orientation_weights: ?*const [31 * 31]f32 = null,

    pub const ScoreType = enum(i32) { harris_score = 0, fast_score = 1 };
    pub const Features = struct { keypoints: []KeyPoint, descriptors: []BinaryDescriptor };

    fn params(self: Orb) c.ZgOrbParams {
        return .{
            .n_features = @intCast(@min(self.n_features, std.math.maxInt(u32))),
            .scale_factor = self.scale_factor,
            .n_levels = self.n_levels,
            .edge_threshold = self.edge_threshold,
            .first_level = self.first_level,
            .wta_k = self.wta_k,
            .fast_threshold = self.fast_threshold,
            .score_type = @intFromEnum(self.score_type),
            .orientation_weights = if (self.orientation_weights) |w| w else null,
        };
    }

    /// orb.zig:279-334
    pub fn featuresPerLevel(self: Orb, allocator: std.mem.Allocator) ![]u32 {
        const out = try allocator.alloc(u32, self.n_levels);
        errdefer allocator.free(out);
        const p = self.params();
        try hip.check(c.zg_orb_features_per_level(&p, out.ptr));
        return out;
    }

    /// orb.zig:511-517
    pub fn adaptiveThreshold(self: Orb, level: u32) !u8 {
        const p = self.params();
        const rc = c.zg_orb_adaptive_threshold(&p, level);
        if (rc < 0) try hip.check(-rc);
        return @intCast(rc);
    }

    /// orb.zig:250-276 on a host image: the count is asked first.
    pub fn detectAndCompute(self: Orb, allocator: std.mem.Allocator, image: zignal.Image(u8)) !Features {
        const d = hip.Image(u8).desc(image);
        const p = self.params();
        var n: u32 = 0;
        try hip.check(c.zg_orb_detect_and_compute_host(&d, &p, null, null, 0, &n));
        const kps = try allocator.alloc(KeyPoint, n);
        errdefer allocator.free(kps);
        const des = try allocator.alloc(BinaryDescriptor, n);
        errdefer allocator.free(des);
        var m: u32 = 0;
        if (n > 0) try hip.check(c.zg_orb_detect_and_compute_host(&d, &p, kps.ptr, des.ptr, n, &m));
        return .{ .keypoints = kps, .descriptors = des };
    }

    /// orb.zig:119-130
    pub fn detect(self: Orb, allocator: std.mem.Allocator, image: zignal.Image(u8)) ![]KeyPoint {
        const d = hip.Image(u8).desc(image);
        const p = self.params();
        var n: u32 = 0;
        try hip.check(c.zg_orb_detect_and_compute_host(&d, &p, null, null, 0, &n));
        const kps = try allocator.alloc(KeyPoint, n);
        errdefer allocator.free(kps);
        var m: u32 = 0;
        if (n > 0) try hip.check(c.zg_orb_detect_and_compute_host(&d, &p, kps.ptr, null, n, &m));
        return kps;
    }

    /// orb.zig:133-144
    pub fn compute(self: Orb, allocator: std.mem.Allocator, image: zignal.Image(u8), keypoints: []const KeyPoint) ![]BinaryDescriptor {
        const d = hip.Image(u8).desc(image);
        const p = self.params();
        const des = try allocator.alloc(BinaryDescriptor, keypoints.len);
        errdefer allocator.free(des);
        if (keypoints.len > 0) try hip.check(c.zg_orb_compute_host(&d, &p, keypoints.ptr, @intCast(keypoints.len), des.ptr));
        return des;
    }

    /// The device form: zg_orb_detect_and_compute on the image's stream into device memory from zg_malloc (at most `capacity`
    /// entries are written, *count receives the full length; descriptors may be null). Asynchronous, capturable into a graph.
    pub fn detectAndComputeInto(self: Orb, image: hip.DeviceImage(u8), keypoints: ?[*]KeyPoint, descriptors: ?[*]BinaryDescriptor, capacity: u32, count: *u32) !void {
        const p = self.params();
        try hip.check(c.zg_orb_detect_and_compute(&image.desc(), &p, keypoints, descriptors, capacity, count, image.stream));
    }

    /// Orb.compute for keypoints already on the device.
    pub fn computeInto(self: Orb, image: hip.DeviceImage(u8), keypoints: [*]const KeyPoint, n: u32, descriptors: [*]BinaryDescriptor) !void {
        const p = self.params();
        try hip.check(c.zg_orb_compute(&image.desc(), &p, keypoints, n, descriptors, image.stream));
    }
};

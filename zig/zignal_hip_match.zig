//! zignal_hip_match.zig — the matcher module of the shim: BruteForceMatcher.match / knnMatch / radiusMatch and MatchStats.compute
//! (reference src/features/matcher.zig) through libzignal_hip.so's zg_match_* entry points (include/zignal_hip_match.h). Sits beside
//! zignal_hip_orb.zig and takes its BinaryDescriptor. Like that file it has not been compiled where the library is built (no Zig
//! toolchain).
const std = @import("std");
const hip = @import("zignal_hip.zig");
const orb = @import("zignal_hip_orb.zig");

pub const BinaryDescriptor = orb.BinaryDescriptor;

pub const c = struct {
    pub const ZgMatch = extern struct { query_idx: u32, train_idx: u32, distance: f32 }; // matcher.zig:10-19, 32-bit indices
    pub const ZgDescriptorSet = extern struct { data: ?[*]const BinaryDescriptor, capacity: u32, count: ?*const u32 };
    pub const ZgMatcherParams = extern struct { cross_check: i32, max_distance: u32, ratio_threshold: f32 }; // matcher.zig:33-41
    pub const ZgMatchStatistics = extern struct { total_matches: usize, mean_distance: f32, min_distance: f32, max_distance: f32 };
    pub extern fn zg_matcher_default_params(params: *ZgMatcherParams) void;
    pub extern fn zg_match_train_chunk() u32;
    pub extern fn zg_match_descriptors(query: *const ZgDescriptorSet, train: *const ZgDescriptorSet, params: *const ZgMatcherParams, matches: ?[*]ZgMatch, capacity: u32, count: *u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_match_knn(query: *const ZgDescriptorSet, train: *const ZgDescriptorSet, params: *const ZgMatcherParams, k: u32, matches: ?[*]ZgMatch, row_counts: ?[*]u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_match_radius(query: *const ZgDescriptorSet, train: *const ZgDescriptorSet, max_dist: f32, matches: ?[*]ZgMatch, capacity: u32, row_counts: ?[*]u32, count: *u32, stream: ?*anyopaque) c_int;
    pub extern fn zg_match_descriptors_host(query: *const ZgDescriptorSet, train: *const ZgDescriptorSet, params: *const ZgMatcherParams, matches: ?[*]ZgMatch, capacity: u32, count: *u32) c_int;
    pub extern fn zg_match_knn_host(query: *const ZgDescriptorSet, train: *const ZgDescriptorSet, params: *const ZgMatcherParams, k: u32, matches: ?[*]ZgMatch, row_counts: ?[*]u32) c_int;
    pub extern fn zg_match_radius_host(query: *const ZgDescriptorSet, train: *const ZgDescriptorSet, max_dist: f32, matches: ?[*]ZgMatch, capacity: u32, row_counts: ?[*]u32, count: *u32) c_int;
    pub extern fn zg_match_stats(matches: ?[*]const ZgMatch, n: usize, out: *ZgMatchStatistics) c_int;
};

// ---- features: BruteForceMatcher (reference src/features/matcher.zig) ----------------------------------------------------

/// Match (matcher.zig:10-19) with usize indices, as the reference's.
pub const Match = struct {
    query_idx: usize,
    train_idx: usize,
    distance: f32,

    fn from(m: c.ZgMatch) Match {
        return .{ .query_idx = m.query_idx, .train_idx = m.train_idx, .distance = m.distance };
    }
};
comptime {
    std.debug.assert(@sizeOf(c.ZgMatch) == 12);
}

fn hostSet(descriptors: []const BinaryDescriptor) !c.ZgDescriptorSet {
    if (descriptors.len > std.math.maxInt(u32)) return error.Unsupported;
    return .{ .data = if (descriptors.len > 0) descriptors.ptr else null, .capacity = @intCast(descriptors.len), .count = null };
}

/// A descriptor array in device memory and, optionally, the device word that holds how many of them count: what
/// Orb.detectAndComputeInto wrote, as it is.
pub const DeviceDescriptors = struct {
    data: ?[*]const BinaryDescriptor,
    capacity: u32,
    count: ?*const u32 = null,

    fn set(self: DeviceDescriptors) c.ZgDescriptorSet {
        return .{ .data = self.data, .capacity = self.capacity, .count = self.count };
    }
};

/// BruteForceMatcher (matcher.zig:33-41): same fields, same defaults; match / knnMatch / radiusMatch return the reference's
/// lists, order included.
pub const BruteForceMatcher = struct {
    cross_check: bool = false,
    max_distance: u32 = 64,
    ratio_threshold: f32 = 0.8,

    fn params(self: BruteForceMatcher) c.ZgMatcherParams {
        return .{ .cross_check = @intFromBool(self.cross_check), .max_distance = self.max_distance, .ratio_threshold = self.ratio_threshold };
    }

    /// matcher.zig:44-106 on host slices.
    pub fn match(self: BruteForceMatcher, allocator: std.mem.Allocator, query: []const BinaryDescriptor, train: []const BinaryDescriptor) ![]Match {
        const q = try hostSet(query);
        const t = try hostSet(train);
        const p = self.params();
        const raw = try allocator.alloc(c.ZgMatch, query.len);
        defer allocator.free(raw);
        var n: u32 = 0;
        try hip.check(c.zg_match_descriptors_host(&q, &t, &p, if (raw.len > 0) raw.ptr else null, q.capacity, &n));
        const out = try allocator.alloc(Match, n);
        for (out, raw[0..n]) |*o, m| o.* = Match.from(m);
        return out;
    }

    fn rowsFrom(allocator: std.mem.Allocator, raw: []const c.ZgMatch, row_counts: []const u32, pitch: ?usize) ![][]Match {
        const rows = try allocator.alloc([]Match, row_counts.len);
        var filled: usize = 0;
        errdefer {
            for (rows[0..filled]) |r| allocator.free(r);
            allocator.free(rows);
        }
        var at: usize = 0;
        for (row_counts, 0..) |len, i| {
            const first = if (pitch) |k| i * k else at;
            rows[i] = try allocator.alloc(Match, len);
            filled = i + 1;
            for (rows[i], raw[first .. first + len]) |*o, m| o.* = Match.from(m);
            at += len;
        }
        return rows;
    }

    /// matcher.zig:109-162 on host slices.
    pub fn knnMatch(self: BruteForceMatcher, allocator: std.mem.Allocator, query: []const BinaryDescriptor, train: []const BinaryDescriptor, k: usize) ![][]Match {
        if (query.len == 0 or train.len == 0 or k == 0) return try allocator.alloc([]Match, 0);
        const q = try hostSet(query);
        const t = try hostSet(train);
        const p = self.params();
        const kk: u32 = @intCast(@min(k, train.len)); // a row is never longer
        const raw = try allocator.alloc(c.ZgMatch, query.len * kk);
        defer allocator.free(raw);
        const row_counts = try allocator.alloc(u32, query.len);
        defer allocator.free(row_counts);
        try hip.check(c.zg_match_knn_host(&q, &t, &p, kk, raw.ptr, row_counts.ptr));
        return rowsFrom(allocator, raw, row_counts, kk);
    }

    /// matcher.zig:165-212 on host slices: the row lengths are asked first.
    pub fn radiusMatch(self: BruteForceMatcher, allocator: std.mem.Allocator, query: []const BinaryDescriptor, train: []const BinaryDescriptor, max_dist: f32) ![][]Match {
        _ = self;
        if (query.len == 0 or train.len == 0) return try allocator.alloc([]Match, 0);
        const q = try hostSet(query);
        const t = try hostSet(train);
        const row_counts = try allocator.alloc(u32, query.len);
        defer allocator.free(row_counts);
        var n: u32 = 0;
        try hip.check(c.zg_match_radius_host(&q, &t, max_dist, null, 0, row_counts.ptr, &n));
        const raw = try allocator.alloc(c.ZgMatch, n);
        defer allocator.free(raw);
        if (n > 0) try hip.check(c.zg_match_radius_host(&q, &t, max_dist, raw.ptr, n, row_counts.ptr, &n));
        return rowsFrom(allocator, raw, row_counts, null);
    }

    /// The device forms: asynchronous on `stream`, capturable into a graph; every pointer is device memory from zg_malloc.
    pub fn matchInto(self: BruteForceMatcher, query: DeviceDescriptors, train: DeviceDescriptors, matches: ?[*]c.ZgMatch, capacity: u32, count: *u32, stream: ?*anyopaque) !void {
        const p = self.params();
        try hip.check(c.zg_match_descriptors(&query.set(), &train.set(), &p, matches, capacity, count, stream));
    }

    pub fn knnMatchInto(self: BruteForceMatcher, query: DeviceDescriptors, train: DeviceDescriptors, k: u32, matches: ?[*]c.ZgMatch, row_counts: ?[*]u32, stream: ?*anyopaque) !void {
        const p = self.params();
        try hip.check(c.zg_match_knn(&query.set(), &train.set(), &p, k, matches, row_counts, stream));
    }

    pub fn radiusMatchInto(self: BruteForceMatcher, query: DeviceDescriptors, train: DeviceDescriptors, max_dist: f32, matches: ?[*]c.ZgMatch, capacity: u32, row_counts: ?[*]u32, count: *u32, stream: ?*anyopaque) !void {
        _ = self;
        try hip.check(c.zg_match_radius(&query.set(), &train.set(), max_dist, matches, capacity, row_counts, count, stream));
    }
};

/// MatchStats (matcher.zig:237-270) of the library's match records.
pub const MatchStats = struct {
    total_matches: usize,
    mean_distance: f32,
    min_distance: f32,
    max_distance: f32,

    pub fn compute(matches: []const c.ZgMatch) !MatchStats {
        var s: c.ZgMatchStatistics = undefined;
        try hip.check(c.zg_match_stats(if (matches.len > 0) matches.ptr else null, matches.len, &s));
        return .{ .total_matches = s.total_matches, .mean_distance = s.mean_distance, .min_distance = s.min_distance, .max_distance = s.max_distance };
    }
};

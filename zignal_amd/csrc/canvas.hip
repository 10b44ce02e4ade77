// canvas.hip — Canvas(T) (reference src/canvas/Canvas.zig) as one device operation over a list of draw commands:
//   drawLine        :152-487  Bresenham with its horizontal / vertical cases, Xiaolin Wu with its horizontal case, the thick fast line
//                             (fillPolygon of four corners, two fillCircle(.fast)), the thick soft line by distance and its axis-aligned form
//   drawPolygon, drawRectangle :579-601 (drawLine per edge), fillRectangle :608-632, fillPolygon :935-1017
//   drawCircle, fillCircle :636-644, :752-876, :1021-1084 (drawBresenhamCircle, renderRing, fillCircleFast's spans)
//   drawQuadraticBezier, drawCubicBezier :1221-1275, :1360-1455 (tessellated by the lanes into LDS, then drawLine per segment in order)
//   drawSplinePolygon, fillSplinePolygon :1280-1355, :1460-1472 (a cubic per edge; the fill is one fillPolygon over all edges' points)
//   drawArc, fillArc :646-750, :878-927, :1039-1218 (ArcRange; the gated Bresenham circle and ring, the soft outline as lines or one polygon,
//                             fillArcFast's spans, fillArcSoft's coverage) — in k_canvas<PIX, true> only, behind zg_canvas_draw_arcs
// composited with Rgba.blend(.normal) and convertColor exactly as Image.insert does (zg_blend.h).
//
// The device gathers (zg_canvas_tile.h: one workgroup per 16 x 16 pixel tile, one lane per pixel, the pixel in registers, the list's commands
// that reach the tile handed to the lanes in list order): each lane applies every write that reaches its pixel, as often as the reference makes it.
//   k_canvas_prep   one lane per command: checks the command against the contract and writes the pixel box that bounds everything the command
//                   can write (empty for a command that is skipped, draws nothing or lies past the count word)
//   k_canvas        (<PIX, false>: every kind but the arcs, zg_canvas_draw; <PIX, true>: the arcs too, zg_canvas_draw_arcs — the routines are
//                   shared, what knows an arc is compiled into the second only) per tile: tile_gather with a command's box and, for lines and
//                   circles, its shape as the test, and Cv::apply as what a hit does.
//                   A command is expanded into the reference's sequence of internal calls on the fly (a rectangle outline is four lines, a thick
//                   fast line a polygon and two discs ...), so no expanded list and no per-tile list ever exists in memory: the only scratch is the
//                   8 bytes per command of the boxes, a size the host knows without reading the (device-resident) commands.
// What is the same for a whole row of a tile — fillPolygon's sorted intersections, fillCircleFast's row value and span, the axis-aligned thick
// line's coverage — is computed once per (call, row) into LDS by 16 lanes.
// The sequential recurrences are evaluated per pixel without tables (their length depends on commands the host never sees, so a table could
// only be sized for the worst case, n x 64 edges x 32768 steps): the integer Bresenham line has a closed form (tests/canvas_ref.py holds it to
// the literal walk); fillCircleFast's `y += 1` in f32 is replayed a binade at a time (exact inside one); Wu's `intery += gradient` and the
// Bresenham circle are re-walked by each lane up to its own step, after a tile-level test has let through only the tiles near the line or ring.
#include "zg_canvas_tile.h"
// every routine of the canvas kernels is inlined (no calls, so no stack): here the device maths too, which elsewhere is left to the compiler
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "zg_devmath.h"
#pragma clang attribute pop

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace zg {

constexpr int CV_POINTS = ZG_CANVAS_MAX_CURVE_POINTS; // vertices of the largest polygon poly_fill is handed
constexpr int CV_CURVE_BASE = 8; // a Bézier's points sit in s_vx / s_vy from here: below it a thick fast line keeps its four corners
constexpr float CV_TILE_REACH = 11.4f; // from a tile's centre (7.5, 7.5) to its farthest pixel centre, rounded up

// The reference's tessellation constants (:36-48): segment counts are max(min, min(max, trunc(estimated length / pixels per segment)))
constexpr int CV_BEZIER_MAX_SEGMENTS = 200, CV_SPLINE_MAX_SEGMENTS = 50, CV_SPLINE_MIN_SEGMENTS = 4, CV_QUADRATIC_MIN_SEGMENTS = 3;
constexpr float CV_PPS_SOFT = 1.5f, CV_PPS_FAST = 3.0f, CV_PPS_QUADRATIC = 2.0f;

struct CvPoint { float x, y; };
__host__ __device__ __forceinline__ float cv_distance(CvPoint a, CvPoint b) { // Point.distance: sub, dot with itself, @sqrt
    const float dx = a.x - b.x, dy = a.y - b.y;
    return sqrtf(dx * dx + dy * dy);
}
__host__ __device__ __forceinline__ int cv_segments(float estimated_length, float pixels_per_segment, int min_segments, int max_segments) { // :1416
    const float q = truncf(estimated_length / pixels_per_segment); // finite and below 2^21 for coordinates inside the contract
    const int s = q < (float)max_segments ? (int)q : max_segments;
    return s > min_segments ? s : min_segments;
}
__host__ __device__ __forceinline__ float cv_cubic_length(CvPoint p0, CvPoint p1, CvPoint p2, CvPoint p3) { // estimateCubicBezierLength (:1398-1403)
    const float chord = cv_distance(p0, p3);
    const float control_net = cv_distance(p0, p1) + cv_distance(p1, p2) + cv_distance(p2, p3);
    return (chord + control_net) / 2.0f;
}
// calculateSmoothControlPoints (:1460-1472) for the edge from vertex i to vertex i + 1 of the spline polygon v[0 .. n)
__host__ __device__ __forceinline__ void cv_spline_edge(const float *v, uint32_t n, uint32_t i, float tension, CvPoint &p0, CvPoint &cp1, CvPoint &cp2, CvPoint &p1) {
    const uint32_t i1 = (i + 1) % n, i2 = (i + 2) % n;
    const float tension_factor = 1.0f - fmaxf(0.0f, fminf(tension, 1.0f));
    p0 = {v[2 * i], v[2 * i + 1]};
    p1 = {v[2 * i1], v[2 * i1 + 1]};
    const CvPoint p2 = {v[2 * i2], v[2 * i2 + 1]};
    cp1 = {p0.x + (p1.x - p0.x) * tension_factor, p0.y + (p1.y - p0.y) * tension_factor};
    cp2 = {p1.x - (p2.x - p1.x) * tension_factor, p1.y - (p2.y - p1.y) * tension_factor};
}
// fillSplinePolygon's total_points (:1318-1328)
__host__ __device__ __forceinline__ uint32_t cv_spline_fill_points(const float *v, uint32_t n, float tension) {
    uint32_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        CvPoint p0, cp1, cp2, p1;
        cv_spline_edge(v, n, i, tension, p0, cp1, cp2, p1);
        total += (uint32_t)cv_segments(cv_cubic_length(p0, cp1, cp2, p1), CV_PPS_FAST, CV_SPLINE_MIN_SEGMENTS, CV_SPLINE_MAX_SEGMENTS);
    }
    return total;
}

// ArcRange (:679-750). 2 pi and pi are the reference's comptime values rounded to f32.
constexpr float CV_TWO_PI = (float)(2.0 * 3.14159265358979323846), CV_PI = (float)3.14159265358979323846;
constexpr int CV_ARC_MIN_SEGMENTS = 8;
struct CvArc {
    float start, end, span; // normalised: start in [0, 2 pi), end in [start, start + 2 pi]
    bool full, is_long;     // isFull: nothing is gated; isLong: containsCross takes the union of the half-planes
    int segments;           // drawArcSoft (:889-893)
    float step;
};
__device__ __forceinline__ float cv_arc_normalize(float angle) { // normalize (:697-701); @mod on f32 as the compiler lowers it (unpinned)
    float n = angle < 0 ? fmodf(fmodf(angle, CV_TWO_PI) + CV_TWO_PI, CV_TWO_PI) : fmodf(angle, CV_TWO_PI);
    if (n < 0) n += CV_TWO_PI;
    return n;
}
__device__ __forceinline__ CvArc cv_arc_init(float start_angle, float end_angle, float radius) {
    CvArc a;
    a.start = cv_arc_normalize(start_angle);
    a.end = cv_arc_normalize(end_angle);
    if (a.end < a.start) a.end += CV_TWO_PI;
    a.span = a.end - a.start;
    a.full = a.span >= CV_TWO_PI;
    a.is_long = a.span > CV_PI;
    const float pieces = ceilf(a.span * radius / 5.0f); // below 2^17 for a radius inside the contract
    const int s = pieces < (float)CV_BEZIER_MAX_SEGMENTS ? (int)pieces : CV_BEZIER_MAX_SEGMENTS;
    a.segments = s > CV_ARC_MIN_SEGMENTS ? s : CV_ARC_MIN_SEGMENTS;
    a.step = a.span / (float)a.segments;
    return a;
}
__device__ __forceinline__ bool cv_arc_contains(const CvArc &a, float angle) { // contains (:706-712): angle is an atan2, in [-pi, pi]
    const float norm_angle = angle < 0 ? angle + CV_TWO_PI : angle;
    if (norm_angle >= a.start && norm_angle <= a.end) return true;
    const float shifted = norm_angle + CV_TWO_PI;
    return shifted >= a.start && shifted <= a.end;
}
__device__ __forceinline__ bool cv_arc_contains_cross(const CvArc &a, float start_cross, float end_cross) { // containsCross (:745-749)
    const bool s = start_cross <= 0, e = end_cross >= 0;
    return a.is_long ? (s || e) : (s && e);
}
// The sequence v0 = start, v += 1 in f32 (fillArcFast's row walk and its x walk) at its first value whose trunc reaches `target`, with
// the value before it (-1: there is none; the walks start at 0 or above). Adding 1 is exact inside a binade and rounds only where the
// sequence crosses a power of two, so it is replayed a binade at a time (tests/canvas_arcs_ref.py: walk_to). disc_fast replays
// fillCircleFast's row walk the same way in its own loop, left as it is so that the kernel without arcs stays the code it was.
__device__ __forceinline__ void cv_walk_to(float start, int target, float &v, float &pred) {
    v = start; pred = -1.0f;
    for (;;) {
        const int t = (int)v;
        if (t >= target) return;
        if (v < 1.0f) { pred = v; v = v + 1.0f; continue; }
        const float next_pow2 = __uint_as_float(((__float_as_uint(v) >> 23) + 1u) << 23);
        const int exact = (int)ceilf(next_pow2 - v) - 1; // steps that stay below it (the difference is exact)
        const int steps = min(exact, target - t);
        if (steps > 0) { pred = v + (float)(steps - 1); v = v + (float)steps; }
        else { pred = v; v = v + 1.0f; }
    }
}

// 0: inside the contract; 1: outside it; 2: a polygon or spline polygon of more than ZG_CANVAS_MAX_VERTICES vertices; 3: a filled spline
// polygon of more than ZG_CANVAS_MAX_CURVE_POINTS points
__host__ __device__ inline bool cv_coord_ok(float v) { return fabsf(v) <= ZG_CANVAS_MAX_COORD; } // false for NaN and the infinities
__host__ __device__ inline bool cv_takes_vertices(int kind) { return kind == ZG_DRAW_POLYGON || kind == ZG_DRAW_FILL_POLYGON || kind >= ZG_DRAW_QUAD_BEZIER; }
// arcs: the caller draws drawArc and fillArc (zg_canvas_draw_arcs and the host form); to zg_canvas_draw they are no kinds
__host__ __device__ inline bool cv_is_arc(int kind) { return kind == ZG_DRAW_ARC || kind == ZG_DRAW_FILL_ARC; }
__host__ __device__ inline int cv_check(const zg_draw_cmd &c, const float *vertices, uint32_t n_vertices, bool arcs) {
    const bool known = (c.kind >= ZG_DRAW_LINE && c.kind <= ZG_DRAW_FILL_POLYGON) || (c.kind >= ZG_DRAW_QUAD_BEZIER && c.kind <= ZG_DRAW_FILL_SPLINE_POLYGON) ||
                       (arcs && cv_is_arc(c.kind));
    if (!known || (c.mode != ZG_DRAW_FAST && c.mode != ZG_DRAW_SOFT)) return 1;
    if (c.width > ZG_CANVAS_MAX_WIDTH) return 1;
    if (cv_is_arc(c.kind)) { // the angle pair is one vertex: any value, the non-finite ones draw nothing (:659); centre and radius as a circle's
        if (c.n_vertices != 1u || c.first_vertex >= n_vertices) return 1;
        for (int i = 0; i < 3; ++i)
            if (!cv_coord_ok(c.p[i])) return 1;
        return 0;
    }
    if (cv_takes_vertices(c.kind)) {
        if (c.kind == ZG_DRAW_QUAD_BEZIER || c.kind == ZG_DRAW_CUBIC_BEZIER) {
            if (c.n_vertices != (c.kind == ZG_DRAW_QUAD_BEZIER ? 3u : 4u)) return 1;
        } else if (c.n_vertices > ZG_CANVAS_MAX_VERTICES) return 2;
        if (c.first_vertex > n_vertices || c.n_vertices > n_vertices - c.first_vertex) return 1;
        for (uint32_t i = 0; i < c.n_vertices; ++i)
            if (!cv_coord_ok(vertices[2 * (size_t)(c.first_vertex + i)]) || !cv_coord_ok(vertices[2 * (size_t)(c.first_vertex + i) + 1])) return 1;
        if (c.kind == ZG_DRAW_SPLINE_POLYGON || c.kind == ZG_DRAW_FILL_SPLINE_POLYGON) {
            if (!cv_coord_ok(c.p[0])) return 1; // the tension
            if (c.kind == ZG_DRAW_FILL_SPLINE_POLYGON && c.n_vertices >= 3 &&
                cv_spline_fill_points(vertices + 2 * (size_t)c.first_vertex, c.n_vertices, c.p[0]) > ZG_CANVAS_MAX_CURVE_POINTS) return 3;
        }
        return 0;
    }
    const int np = (c.kind == ZG_DRAW_CIRCLE || c.kind == ZG_DRAW_FILL_CIRCLE) ? 3 : 4;
    for (int i = 0; i < np; ++i)
        if (!cv_coord_ok(c.p[i])) return 1;
    return 0;
}

// How far from the segment a drawLine can write: half the width, the roundings of end points and spans, and for a Wu line the drift of
// `intery += gradient` (at most half an ulp per step: steps * largest magnitude * 2^-24, taken twice over).
__device__ inline float cv_line_pad(float x1, float y1, float x2, float y2, uint32_t width, int mode) {
    float pad = 0.5f * (float)width + 3.0f;
    if (mode == ZG_DRAW_SOFT && width == 1) {
        const float extent = fmaxf(fabsf(x2 - x1), fabsf(y2 - y1)) + 2.0f;
        const float largest = fmaxf(fmaxf(fabsf(x1), fabsf(y1)), fmaxf(fabsf(x2), fabsf(y2))) + 2.0f;
        pad += extent * largest * (1.0f / 8388608.0f);
    }
    return pad;
}

// What an arc can write lies within `pad` of its circle (the disc, for a fill): the ring's half width and the roundings; the soft
// outline of width 1 is up to 200 Wu lines between points on the circle, with their drift
__device__ inline float cv_arc_pad(const zg_draw_cmd &c) {
    if (c.kind == ZG_DRAW_FILL_ARC) return 3.0f;
    if (c.mode == ZG_DRAW_SOFT && c.width == 1) return cv_line_pad(c.p[0] - c.p[2], c.p[1] - c.p[2], c.p[0] + c.p[2], c.p[1] + c.p[2], 1, ZG_DRAW_SOFT);
    return 0.5f * (float)c.width + 3.0f;
}

__global__ __launch_bounds__(256) void k_canvas_prep(const zg_draw_cmd *cmds, uint32_t n, const uint32_t *count_device, const float *vertices,
                                                     uint32_t n_vertices, int rows, int cols, ushort4 *boxes, bool arcs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t count = count_device ? min(*count_device, n) : n;
    int4 box = make_int4(0, 0, 0, 0);
    if (i < count && cv_check(cmds[i], vertices, n_vertices, arcs) == 0) {
        const zg_draw_cmd c = cmds[i];
        float x0 = 0, y0 = 0, x1 = 0, y1 = 0, pad = 0;
        bool draws = true;
        switch (c.kind) {
        case ZG_DRAW_LINE:
            x0 = fminf(c.p[0], c.p[2]); x1 = fmaxf(c.p[0], c.p[2]); y0 = fminf(c.p[1], c.p[3]); y1 = fmaxf(c.p[1], c.p[3]);
            pad = cv_line_pad(x0, y0, x1, y1, c.width, c.mode);
            draws = c.width != 0;
            break;
        case ZG_DRAW_RECT:
            x0 = fminf(c.p[0], c.p[2] - 1); x1 = fmaxf(c.p[0], c.p[2] - 1); y0 = fminf(c.p[1], c.p[3] - 1); y1 = fmaxf(c.p[1], c.p[3] - 1);
            pad = cv_line_pad(x0, y0, x1, y1, c.width, c.mode);
            draws = c.width != 0;
            break;
        case ZG_DRAW_FILL_RECT:
            x0 = fminf(c.p[0], c.p[2]); x1 = fmaxf(c.p[0], c.p[2]); y0 = fminf(c.p[1], c.p[3]); y1 = fmaxf(c.p[1], c.p[3]);
            pad = 1.0f;
            break;
        case ZG_DRAW_CIRCLE:
        case ZG_DRAW_FILL_CIRCLE:
            x0 = c.p[0] - c.p[2]; x1 = c.p[0] + c.p[2]; y0 = c.p[1] - c.p[2]; y1 = c.p[1] + c.p[2];
            pad = (c.kind == ZG_DRAW_CIRCLE ? 0.5f * (float)c.width : 0.0f) + 3.0f;
            draws = c.p[2] > 0 && (c.kind == ZG_DRAW_FILL_CIRCLE || c.width != 0);
            break;
        case ZG_DRAW_ARC:
        case ZG_DRAW_FILL_ARC: { // the circle's box
            const float a0 = vertices[2 * (size_t)c.first_vertex], a1 = vertices[2 * (size_t)c.first_vertex + 1];
            x0 = c.p[0] - c.p[2]; x1 = c.p[0] + c.p[2]; y0 = c.p[1] - c.p[2]; y1 = c.p[1] + c.p[2];
            pad = cv_arc_pad(c);
            draws = c.p[2] > 0 && (c.kind == ZG_DRAW_FILL_ARC || c.width != 0) && fabsf(a0) < INFINITY && fabsf(a1) < INFINITY;
            break;
        }
        default: { // the polygons and the curves: a Bézier stays inside the hull of its control points
            const bool outline = c.kind != ZG_DRAW_FILL_POLYGON && c.kind != ZG_DRAW_FILL_SPLINE_POLYGON;
            const bool spline = c.kind == ZG_DRAW_SPLINE_POLYGON || c.kind == ZG_DRAW_FILL_SPLINE_POLYGON;
            draws = outline ? (c.width != 0 && c.n_vertices >= (spline ? 3u : 1u)) : c.n_vertices >= 3;
            if (draws) {
                const float *v = vertices + 2 * (size_t)c.first_vertex;
                x0 = x1 = v[0]; y0 = y1 = v[1];
                for (uint32_t k = 1; k < c.n_vertices; ++k) {
                    x0 = fminf(x0, v[2 * k]); x1 = fmaxf(x1, v[2 * k]); y0 = fminf(y0, v[2 * k + 1]); y1 = fmaxf(y1, v[2 * k + 1]);
                }
                if (spline) { // cp1 lies between two vertices; cp2 = p1 - (p2 - p1) * tf with tf in [0, 1] lies between p1 and 2 p1 - p2
                    for (uint32_t k = 0; k < c.n_vertices; ++k) {
                        const uint32_t k1 = (k + 1) % c.n_vertices, k2 = (k + 2) % c.n_vertices;
                        const float mx = v[2 * k1] - (v[2 * k2] - v[2 * k1]), my = v[2 * k1 + 1] - (v[2 * k2 + 1] - v[2 * k1 + 1]);
                        x0 = fminf(x0, mx); x1 = fmaxf(x1, mx); y0 = fminf(y0, my); y1 = fmaxf(y1, my);
                    }
                }
                pad = outline ? cv_line_pad(x0, y0, x1, y1, c.width, c.mode) : 2.0f;
            }
        }
        }
        if (draws) {
            const float fc = (float)cols, fr = (float)rows;
            box.x = (int)fminf(fmaxf(floorf(x0 - pad), 0.0f), fc);
            box.y = (int)fminf(fmaxf(floorf(y0 - pad), 0.0f), fr);
            box.z = (int)fminf(fmaxf(ceilf(x1 + pad) + 1.0f, 0.0f), fc);
            box.w = (int)fminf(fmaxf(ceilf(y1 + pad) + 1.0f, 0.0f), fr);
            if (box.x >= box.z || box.y >= box.w) box = make_int4(0, 0, 0, 0);
        }
    }
    boxes[i] = make_ushort4((unsigned short)box.x, (unsigned short)box.y, (unsigned short)box.z, (unsigned short)box.w); // 0 .. 32768 each
}

// Is the segment p1-p2 farther than `limit` from (cx, cy)? f32 with margins to spare: the callers' limits carry whole pixels of slack.
__device__ inline bool cv_far_from_segment(float cx, float cy, float p1x, float p1y, float p2x, float p2y, float limit) {
    const float dx = p2x - p1x, dy = p2y - p1y, len2 = dx * dx + dy * dy;
    float t = len2 > 0 ? ((cx - p1x) * dx + (cy - p1y) * dy) / len2 : 0.0f;
    t = fmaxf(0.0f, fminf(t, 1.0f));
    const float qx = cx - (p1x + t * dx), qy = cy - (p1y + t * dy);
    return sqrtf(qx * qx + qy * qy) > limit;
}
// Can the command write into the tile at (tx0, ty0)? Exact "no", generous "yes": for a line the distance from the tile's centre to the
// segment, for a circle to the ring; the other kinds fill most of their boxes. One lane per command asks this while the tile's list is
// made; a line or ring that is part of a larger command (an edge of a rectangle or polygon) is asked again by all lanes when it is drawn.
template <bool ARCS> __device__ inline bool cv_tile_may_touch(const zg_draw_cmd &c, int tx0, int ty0) {
    const float tcx = (float)tx0 + 7.5f, tcy = (float)ty0 + 7.5f;
    if constexpr (ARCS) {
        if (cv_is_arc(c.kind)) { // an arc as its ring, a filled arc as its disc
            const float dx = tcx - c.p[0], dy = tcy - c.p[1], dc = sqrtf(dx * dx + dy * dy), pad = cv_arc_pad(c);
            if (dc - CV_TILE_REACH > c.p[2] + pad) return false;
            // The soft outline of width > 1 is a polygon whose inner edge is chords of the circle of radius r - w / 2: at the cap of 200
            // segments they sag inwards by about r span^2 / 320000, pixels at a radius of tens of thousands, which no fixed pad bounds.
            // So the polygon has no inner "no"; its chords never leave the outer circle, and poly_fill decides the rest per row.
            if (c.kind != ZG_DRAW_ARC || (c.mode == ZG_DRAW_SOFT && c.width > 1)) return true;
            return !(dc + CV_TILE_REACH < c.p[2] - pad);
        }
    }
    if (c.kind == ZG_DRAW_LINE)
        return !cv_far_from_segment(tcx, tcy, c.p[0], c.p[1], c.p[2], c.p[3], cv_line_pad(c.p[0], c.p[1], c.p[2], c.p[3], c.width, c.mode) + CV_TILE_REACH + 0.5f);
    if (c.kind == ZG_DRAW_CIRCLE || c.kind == ZG_DRAW_FILL_CIRCLE) {
        const float dx = tcx - c.p[0], dy = tcy - c.p[1], dc = sqrtf(dx * dx + dy * dy);
        const float half = c.kind == ZG_DRAW_CIRCLE ? 0.5f * (float)c.width : 0.0f;
        if (dc - CV_TILE_REACH > c.p[2] + half + 3.0f) return false;
        return !(c.kind == ZG_DRAW_CIRCLE && dc + CV_TILE_REACH < c.p[2] - half - 3.0f);
    }
    return true;
}

__device__ inline float cv_fpart(float x) { return x - floorf(x); }
__device__ inline float cv_rfpart(float x) { return 1.0f - cv_fpart(x); }
template <int PIX> struct Cv : TilePixel<PIX> {
    using TilePixel<PIX>::col;
    using TilePixel<PIX>::row;
    using TilePixel<PIX>::solid;
    using TilePixel<PIX>::pixel;
    int tx0, ty0, tid;
    float fx, fy, fcols, frows;
    float *s_vx, *s_vy, *s_ix; // polygon vertices [CV_POINTS], [CV_POINTS]; sorted intersections [16][CV_POINTS]
    float *s_row;              // what a disc or an axis-aligned line computes once per tile row or column [16][3]
    int *s_icnt;               // intersections per tile row [16]
    unsigned long long *s_near; // a curve's segments that can reach the tile, one bit each [4]

    __device__ __forceinline__ void point(float x, float y, Rgba8 c) { // setPoint (:518-523)
        if (floorf(x) == fx && floorf(y) == fy) pixel(c);
    }
    __device__ __forceinline__ void span(float x1, float x2, float y, Rgba8 c) { // setHorizontalSpan (:129-145)
        if (y < 0 || y >= frows) return;
        if (x2 < 0 || x1 >= fcols) return;
        const int r = (int)y, start = (int)fmaxf(0.0f, floorf(x1)), end = (int)fminf(fcols - 1, ceilf(x2));
        if (r == row && col >= start && col <= end) solid(c);
    }
    // clampRectToImage (:62-79)
    __device__ __forceinline__ bool clamp_rect(float l, float t, float r, float b, int &left, int &top, int &right, int &bottom) const {
        left = (int)clampf(l, 0.0f, fcols); top = (int)clampf(t, 0.0f, frows);
        right = (int)clampf(r, 0.0f, fcols); bottom = (int)clampf(b, 0.0f, frows);
        return !(left >= right || top >= bottom);
    }
    __device__ __forceinline__ float tile_distance(float cx, float cy) const { // from the tile's centre to (cx, cy)
        const float dx = (float)tx0 + 7.5f - cx, dy = (float)ty0 + 7.5f - cy;
        return sqrtf(dx * dx + dy * dy);
    }

    __device__ __forceinline__ void fill_rect(float l, float t, float r, float b, Rgba8 color, int mode) { // :608-632
        int left, top, right, bottom;
        if (!clamp_rect(l, t, r, b, left, top, right, bottom)) return;
        if (col < left || col >= right || row < top || row >= bottom) return;
        if (mode == ZG_DRAW_FAST) solid(color); else pixel(color);
    }

    // renderRing (:794-822) with ringBoundingBox and ringCoverage (:754-786). ARC: a pixel the ring covers is written only where the arc
    // contains its angle (full arcs excepted); without it, the full circle
    __device__ __forceinline__ void ring(float cx, float cy, float inner, float outer, Rgba8 color, int mode) {
        ring_t<false>(cx, cy, inner, outer, color, mode, CvArc{});
    }
    template <bool ARC> __device__ __forceinline__ void ring_t(float cx, float cy, float inner, float outer, Rgba8 color, int mode, const CvArc &arc) {
        const float dc = tile_distance(cx, cy);
        if (dc - CV_TILE_REACH > outer + 3.0f || (inner > 0 && dc + CV_TILE_REACH < inner - 3.0f)) return; // the tile misses the ring
        const int left = (int)roundf(clampf(cx - outer - 1, 0.0f, fcols)), top = (int)roundf(clampf(cy - outer - 1, 0.0f, frows));
        const int right = (int)roundf(clampf(cx + outer + 1, 0.0f, fcols)), bottom = (int)roundf(clampf(cy + outer + 1, 0.0f, frows));
        if (left >= right || top >= bottom) return;
        if (col < left || col >= right || row < top || row >= bottom) return;
        const float y = fy - cy, x = fx - cx;
        const float dist_sq = x * x + y * y;
        if (mode == ZG_DRAW_SOFT) {
            const float dist = sqrtf(dist_sq);
            if (dist > outer + 0.5f) return;
            if (inner > 0 && dist < inner - 0.5f) return;
            float alpha = 1.0f;
            if (dist > outer - 0.5f) alpha = fminf(alpha, outer + 0.5f - dist);
            if (inner > 0 && dist < inner + 0.5f) alpha = fminf(alpha, dist - (inner - 0.5f));
            const float coverage = clampf(alpha, 0.0f, 1.0f);
            if (coverage <= 0) return;
            if constexpr (ARC) { if (!arc.full && !cv_arc_contains(arc, dev_atan2f(y, x))) return; }
            pixel(fade(color, coverage));
        } else {
            const bool inside_outer = dist_sq <= outer * outer;
            const bool outside_inner = inner <= 0 || dist_sq >= inner * inner;
            if constexpr (ARC) { if (inside_outer && outside_inner && !arc.full && !cv_arc_contains(arc, dev_atan2f(y, x))) return; }
            if (inside_outer && outside_inner) solid(color);
        }
    }

    // drawBresenhamCircle over the full circle (:826-860): f32 state that only ever holds integers. The step (x, y) that can reach this
    // pixel is fixed by the pixel (x = the larger, y = the smaller of its |offsets|); the lane walks to it, then makes the step's eight
    // setPoint calls in their order, so a pixel that two of the offsets name (y == 0, x == y) is written twice.
    // ARC: each of the eight is gated by the arc containing atan2 of its offset. The offsets are negated f32 values, so an offset of 0
    // is +0 or -0, and atan2 tells them apart (atan2(0, -0) = pi, atan2(-0, -0) = -pi): the signs decide which axis points an arc keeps.
    template <bool ARC> __device__ __forceinline__ void circle_bresenham(float center_x, float center_y, float radius, Rgba8 color, const CvArc &arc) {
        const float cx = roundf(center_x), cy = roundf(center_y), r = roundf(radius);
        const float dc = tile_distance(cx, cy);
        if (dc - CV_TILE_REACH > r + 2.0f || dc + CV_TILE_REACH < r - 2.0f) return;
        const float ox = fx - cx, oy = fy - cy;
        const float a = fmaxf(fabsf(ox), fabsf(oy)), b = fminf(fabsf(ox), fabsf(oy));
        float x = r, y = 0, err = 0;
        bool hit = false;
        while (x >= y) {
            if (y > b) break;
            if (y == b && x == a) { hit = true; break; }
            if (err <= 0) { y += 1; err += 2 * y + 1; }
            if (err > 0) { x -= 1; err -= 2 * x + 1; }
        }
        if (!hit) return;
        if constexpr (ARC) {
#pragma unroll 1
            for (int k = 0; k < 8; ++k) { // (x, y) (-x, y) (x, -y) (-x, -y) (y, x) (-y, x) (y, -x) (-y, -x)
                float o0 = k < 4 ? x : y, o1 = k < 4 ? y : x;
                if (k & 1) o0 = -o0;
                if (k & 2) o1 = -o1;
                if (o0 == ox && o1 == oy && (arc.full || cv_arc_contains(arc, dev_atan2f(o1, o0)))) pixel(color);
            }
            return;
        }
        if (x == ox && y == oy) pixel(color);
        if (-x == ox && y == oy) pixel(color);
        if (x == ox && -y == oy) pixel(color);
        if (-x == ox && -y == oy) pixel(color);
        if (y == ox && x == oy) pixel(color);
        if (-y == ox && x == oy) pixel(color);
        if (y == ox && -x == oy) pixel(color);
        if (-y == ox && -x == oy) pixel(color);
    }

    // fillCircleFast (:1067-1084): y starts at top = max(0, cy - radius) and grows by `y += 1` in f32. Adding 1 is exact while y stays inside
    // a binade and rounds only when it crosses a power of two, so the lane replays the walk a binade at a time up to its own row
    // (tests/canvas_ref.py: disc_row_y, held to the literal walk): y is the walk's value in this row, if it has one. The row's y and span
    // ends are the same for the whole row: lanes 0-15 compute them once per (disc, tile row) into LDS. Entered by all lanes together.
    __device__ __forceinline__ void disc_fast(float cx, float cy, float radius, Rgba8 color) {
        if (tile_distance(cx, cy) - CV_TILE_REACH > radius + 3.0f) return;
        if (tid < CV_TILE) {
            const int r = ty0 + tid;
            const float top = fmaxf(0.0f, cy - radius), bottom = fminf(frows - 1, cy + radius);
            float y = top;
            while (y <= bottom) {
                const int t = (int)y;
                if (t >= r) break;
                if (y < 1.0f) { y = y + 1.0f; continue; }
                const float next_pow2 = __uint_as_float(((__float_as_uint(y) >> 23) + 1u) << 23);
                const int exact = (int)ceilf(next_pow2 - y) - 1; // steps that stay below it (the difference is exact)
                const int steps = min(exact, r - t);
                y = steps > 0 ? y + (float)steps : y + 1.0f;
            }
            float x1 = 0.0f, x2 = 0.0f;
            bool has_span = y <= bottom && (int)y == r;
            if (has_span) {
                const float dy = y - cy;
                const float dx = sqrtf(fmaxf(0.0f, radius * radius - dy * dy));
                has_span = dx > 0;
                x1 = cx - dx; x2 = cx + dx;
            }
            s_row[3 * tid] = has_span ? y : -1.0f; // y >= 0 whenever the row has a span
            s_row[3 * tid + 1] = x1;
            s_row[3 * tid + 2] = x2;
        }
        __syncthreads();
        const float y = s_row[3 * (tid >> 4)];
        if (y >= 0) span(s_row[3 * (tid >> 4) + 1], s_row[3 * (tid >> 4) + 2], y, color);
        __syncthreads();
    }

    // fillArcFast (:1088-1146). Rows: the walk of fillCircleFast, its value for each row of the tile found once by lanes 0-15. Within a
    // row the reference visits one sequence of x values, v0 = scan_left, v += 1 in f32 (x and span_end both move along it), and joins
    // consecutive ones that lie in the wedge into spans [v_a, v_b], each stored as pixels floor(v_a) .. ceil(v_b). A value belongs to a
    // span when it is in the wedge and either not past scan_right (the outer loop starts or continues a span there) or reached by the
    // inner loop from the value before it (that one short of scan_right and in the wedge, this one inside the circle). Consecutive values
    // are 1 apart up to a rounding, so the spans' pixels are those of their values, floor(v) .. ceil(v) each: this pixel is stored when a
    // value of a span lies in (col - 1, col + 1), and at most two values do. The stores are plain, so once is as good as twice.
    // (tests/canvas_arcs_ref.py: arc_fill_fast_gather, held to the literal loops.) Entered by all lanes together.
    __device__ __forceinline__ void arc_fill_fast(float cx, float cy, float radius, Rgba8 color, const CvArc &arc) {
        if (arc.span <= 0) return;
        if (tile_distance(cx, cy) - CV_TILE_REACH > radius + 3.0f) return;
        const float top = fmaxf(0.0f, cy - radius), bottom = fminf(frows - 1, cy + radius);
        if (tid < CV_TILE) {
            float y, before;
            cv_walk_to(top, ty0 + tid, y, before);
            s_row[tid] = (y <= bottom && (int)y == ty0 + tid) ? y : -1.0f;
        }
        __syncthreads();
        const float y = s_row[tid >> 4];
        __syncthreads();
        if (!(y >= 0)) return;
        const float cos_s = dev_cosf(arc.start), sin_s = dev_sinf(arc.start), cos_e = dev_cosf(arc.end), sin_e = dev_sinf(arc.end); // startVector, endVector
        const float cx_sin_s = cx * sin_s, cx_sin_e = cx * sin_e;
        const float left = fmaxf(0.0f, cx - radius), right = fminf(fcols - 1, cx + radius);
        const float radius_sq = radius * radius;
        const float dy = y - cy, dx_max_sq = radius_sq - dy * dy;
        if (dx_max_sq <= 0) return;
        const float dx_max = sqrtf(dx_max_sq);
        const float scan_left = fmaxf(left, cx - dx_max), scan_right = fminf(right, cx + dx_max);
        const float start_const = -cx_sin_s - dy * cos_s, end_const = -cx_sin_e - dy * cos_e;
        float v, before;
        cv_walk_to(scan_left, col - 1, v, before);
        bool stored = false;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (v > fx - 1 && v < fx + 1 && cv_arc_contains_cross(arc, v * sin_s + start_const, v * sin_e + end_const)) {
                bool in_span = v <= scan_right;
                if (!in_span && before >= 0 && before < scan_right) {
                    const float dnx = v - cx;
                    in_span = !(dnx * dnx + dy * dy > radius_sq) && cv_arc_contains_cross(arc, before * sin_s + start_const, before * sin_e + end_const);
                }
                stored = stored || in_span;
            }
            before = v; v = v + 1.0f;
        }
        if (stored) solid(color);
    }

    // fillArcSoft (:1179-1218) with calculateArcCoverage (:1149-1176)
    __device__ __forceinline__ void arc_fill_soft(float cx, float cy, float radius, Rgba8 color, const CvArc &arc) {
        if (tile_distance(cx, cy) - CV_TILE_REACH > radius + 3.0f) return;
        const int left = (int)roundf(clampf(cx - radius - 1, 0.0f, fcols)), top = (int)roundf(clampf(cy - radius - 1, 0.0f, frows));
        const int right = (int)roundf(clampf(cx + radius + 1, 0.0f, fcols)), bottom = (int)roundf(clampf(cy + radius + 1, 0.0f, frows));
        if (left >= right || top >= bottom) return;
        if (col < left || col >= right || row < top || row >= bottom) return;
        const float y = fy - cy, x = fx - cx;
        const float dist_sq = x * x + y * y;
        if (dist_sq > (radius + 1) * (radius + 1)) return;
        const float cos_s = dev_cosf(arc.start), sin_s = dev_sinf(arc.start), cos_e = dev_cosf(arc.end), sin_e = dev_sinf(arc.end);
        const bool in_arc = cv_arc_contains(arc, dev_atan2f(y, x));
        const float start_cross_product = x * sin_s - y * cos_s, end_cross_product = x * sin_e - y * cos_e; // Point.cross
        const float start_cross = fabsf(start_cross_product), end_cross = fabsf(end_cross_product);
        const float eps = 1e-5f;
        const bool near_start = start_cross < 1.0f && start_cross_product < eps, near_end = end_cross < 1.0f && end_cross_product > -eps;
        if (!in_arc && !near_start && !near_end) return;
        const float dist = sqrtf(dist_sq);
        const float circ_coverage = dist <= radius - 1.0f ? 1.0f : (dist < radius + 1.0f ? clampf(radius - dist + 0.5f, 0.0f, 1.0f) : 0.0f);
        float coverage;
        if (!in_arc) {
            float edge_coverage = 0.0f;
            if (near_start) edge_coverage = fmaxf(edge_coverage, 1.0f - start_cross);
            if (near_end) edge_coverage = fmaxf(edge_coverage, 1.0f - end_cross);
            coverage = circ_coverage * edge_coverage;
        } else {
            coverage = circ_coverage;
            if (start_cross < 1.0f && start_cross_product >= -eps) coverage = fminf(coverage, start_cross);
            if (end_cross < 1.0f && end_cross_product <= eps) coverage = fminf(coverage, end_cross);
        }
        if (coverage > 0) pixel(fade(color, coverage));
    }

    // fillPolygon (:935-1017) of the n >= 3 vertices in s_vx / s_vy. Lanes 0-15 each take one row of the tile: the intersections in the
    // reference's formula and edge rule, sorted ascending; then every lane reads its row's spans in pairs, left to right.
    __device__ __forceinline__ void poly_fill(int n, Rgba8 color, int mode) {
        __syncthreads();
        if (tid < CV_TILE) {
            const float y = (float)(ty0 + tid);
            float min_y = s_vy[0], max_y = s_vy[0];
            for (int i = 1; i < n; ++i) { min_y = fminf(min_y, s_vy[i]); max_y = fmaxf(max_y, s_vy[i]); }
            const float start_y = fmaxf(0.0f, floorf(min_y)), end_y = fminf(frows - 1, ceilf(max_y));
            float *xs = s_ix + tid * CV_POINTS;
            int count = 0;
            if (y >= start_y && y <= end_y) {
                for (int i = 0; i < n; ++i) {
                    const int j = i + 1 == n ? 0 : i + 1;
                    const float p1x = s_vx[i], p1y = s_vy[i], p2x = s_vx[j], p2y = s_vy[j];
                    if ((p1y <= y && p2y > y) || (p2y <= y && p1y > y)) {
                        const float x = p1x + (y - p1y) * (p2x - p1x) / (p2y - p1y);
                        int k = count++;
                        for (; k > 0 && xs[k - 1] > x; --k) xs[k] = xs[k - 1];
                        xs[k] = x;
                    }
                }
            }
            s_icnt[tid] = count;
        }
        __syncthreads();
        const int count = s_icnt[tid >> 4];
        const float *xs = s_ix + (tid >> 4) * CV_POINTS;
        for (int i = 0; i + 1 < count; i += 2) {
            const float left_edge = xs[i], right_edge = xs[i + 1];
            if (mode == ZG_DRAW_SOFT) {
                const float x = fx, x_start = fmaxf(0.0f, floorf(left_edge)), x_end = fminf(fcols - 1, ceilf(right_edge));
                if (x >= x_start && x <= x_end) {
                    float alpha = 1.0f;
                    if (x < left_edge + 1) alpha = fminf(alpha, x + 0.5f - left_edge);
                    if (x > right_edge - 1) alpha = fminf(alpha, right_edge - (x - 0.5f));
                    alpha = clampf(alpha, 0.0f, 1.0f);
                    if (alpha > 0) pixel(fade(color, alpha));
                }
            } else {
                span(left_edge, right_edge, fy, color);
            }
        }
        __syncthreads();
    }

    // drawLineBresenham (:187-240)
    __device__ __forceinline__ void line_bresenham(float p1x, float p1y, float p2x, float p2y, Rgba8 color) {
        const int x1 = (int)p1x, y1 = (int)p1y, x2 = (int)p2x, y2 = (int)p2y;
        if (y1 == y2) {
            span((float)min(x1, x2), (float)max(x1, x2), (float)y1, color);
            return;
        }
        if (x1 == x2) {
            if (col == x1 && row >= min(y1, y2) && row <= max(y1, y2)) solid(color);
            return;
        }
        // The general walk takes one major-axis step per iteration; after m of them it has taken floor((2 m dmin + dmaj - 1) / (2 dmaj))
        // minor-axis steps (tests/test_canvas_oracle.py compares this with the literal walk for every (dx, dy) up to 64 in all octants).
        const int dx = abs(x2 - x1), dy = abs(y2 - y1);
        const int sx = x1 < x2 ? 1 : -1, sy = y1 < y2 ? 1 : -1;
        const int mx = (col - x1) * sx, my = (row - y1) * sy;
        if (mx < 0 || mx > dx || my < 0 || my > dy) return;
        if (dx >= dy) {
            if ((long long)my == (2ll * mx * dy + dx - 1) / (2ll * dx)) solid(color);
        } else {
            if ((long long)mx == (2ll * my * dx + dy - 1) / (2ll * dy)) solid(color);
        }
    }

    // drawLineXiaolinWu (:246-341): end point 1 (two pixels), end point 2 (two pixels), then the main loop's two pixels of this lane's column
    // (row, when steep), each applied when it names this pixel — a line whose end points round to one column blends that column twice.
    __device__ __forceinline__ void line_wu(float x1, float y1, float x2, float y2, Rgba8 c2) {
        if (fabsf(y2 - y1) < 0.01f) {
            const float y = roundf(y1), min_x = fminf(x1, x2), max_x = fmaxf(x1, x2);
            const float left_x = floorf(min_x), right_x = ceilf(max_x);
            if (min_x > left_x) point(left_x, y, fade(c2, min_x - left_x));
            const float solid_start = ceilf(min_x), solid_end = floorf(max_x);
            if (solid_end >= solid_start) span(solid_start, solid_end, y, c2);
            if (max_x < right_x) point(right_x, y, fade(c2, right_x - max_x));
            return;
        }
        const bool steep = fabsf(y2 - y1) > fabsf(x2 - x1);
        if (steep) { float t = x1; x1 = y1; y1 = t; t = x2; x2 = y2; y2 = t; }
        if (x1 > x2) { float t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        const float dx = x2 - x1, dy = y2 - y1;
        const float gradient = dx == 0 ? 1.0f : dy / dx;
        const float major = steep ? fy : fx; // this pixel along the line's major axis
        float x_px1, x_px2, intery;
        {
            const float x_end = roundf(x1), y_end = y1 + gradient * (x_end - x1), x_gap = cv_rfpart(x1 + 0.5f), y_px = floorf(y_end);
            if (steep) { point(y_px, x_end, fade(c2, cv_rfpart(y_end) * x_gap)); point(y_px + 1, x_end, fade(c2, cv_fpart(y_end) * x_gap)); }
            else { point(x_end, y_px, fade(c2, cv_rfpart(y_end) * x_gap)); point(x_end, y_px + 1, fade(c2, cv_fpart(y_end) * x_gap)); }
            x_px1 = x_end;
            intery = y_end + gradient;
        }
        {
            const float x_end = roundf(x2), y_end = y2 + gradient * (x_end - x2), x_gap = cv_fpart(x2 + 0.5f), y_px = floorf(y_end);
            if (steep) { point(y_px, x_end, fade(c2, cv_rfpart(y_end) * x_gap)); point(y_px + 1, x_end, fade(c2, cv_fpart(y_end) * x_gap)); }
            else { point(x_end, y_px, fade(c2, cv_rfpart(y_end) * x_gap)); point(x_end, y_px + 1, fade(c2, cv_fpart(y_end) * x_gap)); }
            x_px2 = x_end;
        }
        if (!(major > x_px1 && major < x_px2)) return;
        const int steps = (int)(major - x_px1) - 1; // additions before the loop reaches this column
        for (int k = 0; k < steps; ++k) intery += gradient;
        if (steep) { point(intery, major, fade(c2, cv_rfpart(intery))); point(floorf(intery) + 1, major, fade(c2, cv_fpart(intery))); }
        else { point(major, intery, fade(c2, cv_rfpart(intery))); point(major, floorf(intery) + 1, fade(c2, cv_fpart(intery))); }
    }

    __device__ __forceinline__ static float perpendicular_alpha(float sample, float center, float half_width) { // :491-496
        const float dist = fabsf(sample - center);
        if (dist > half_width + 0.5f) return 0.0f;
        if (dist > half_width - 0.5f) return half_width + 0.5f - dist;
        return 1.0f;
    }

    // drawLine (:152-181) and everything under it
    __device__ __forceinline__ void line(float p1x, float p1y, float p2x, float p2y, Rgba8 color, uint32_t width, int mode) {
        { // the tile against the segment: nothing the line writes is farther from it than `pad`
            const float pad = cv_line_pad(p1x, p1y, p2x, p2y, width, mode);
            if (cv_far_from_segment((float)tx0 + 7.5f, (float)ty0 + 7.5f, p1x, p1y, p2x, p2y, pad + CV_TILE_REACH + 0.5f)) return;
        }
        const float half_width = (float)width / 2.0f;
        if (mode == ZG_DRAW_FAST) {
            if (width == 1) { line_bresenham(p1x, p1y, p2x, p2y, color); return; }
            // drawLineRectangle (:347-381)
            const float dx = p2x - p1x, dy = p2y - p1y;
            const float line_length = sqrtf(dx * dx + dy * dy);
            if (line_length == 0) { disc_fast(p1x, p1y, half_width, color); return; }
            const float perp_x = -dy / line_length * half_width, perp_y = dx / line_length * half_width;
            if (tid == 0) {
                s_vx[0] = p1x - perp_x; s_vy[0] = p1y - perp_y;
                s_vx[1] = p1x + perp_x; s_vy[1] = p1y + perp_y;
                s_vx[2] = p2x + perp_x; s_vy[2] = p2y + perp_y;
                s_vx[3] = p2x - perp_x; s_vy[3] = p2y - perp_y;
            }
            poly_fill(4, color, ZG_DRAW_FAST);
            disc_fast(p1x, p1y, half_width, color);
            disc_fast(p2x, p2y, half_width, color);
            return;
        }
        if (width == 1) { line_wu(p1x, p1y, p2x, p2y, color); return; }
        // drawLineDistance (:387-437)
        const float dx = p2x - p1x, dy = p2y - p1y;
        const float length_sq = dx * dx + dy * dy;
        if (length_sq == 0) { ring(p1x, p1y, 0.0f, half_width, color, ZG_DRAW_SOFT); return; }
        int left, top, right, bottom;
        if (dx == 0 || dy == 0) { // drawAxisAlignedThickLine (:443-487)
            const bool is_horizontal = p1y == p2y;
            const bool ok = is_horizontal ? clamp_rect(fminf(p1x, p2x), p1y - half_width, fmaxf(p1x, p2x) + 1, p1y + half_width + 1, left, top, right, bottom)
                                          : clamp_rect(p1x - half_width, fminf(p1y, p2y), p1x + half_width + 1, fmaxf(p1y, p2y) + 1, left, top, right, bottom);
            // the coverage is the same along a row (horizontal) or a column (vertical) of the tile: once per row or column, by lanes 0-15
            if (tid < CV_TILE) s_row[tid] = is_horizontal ? perpendicular_alpha((float)(ty0 + tid), p1y, half_width) : perpendicular_alpha((float)(tx0 + tid), p1x, half_width);
            __syncthreads();
            const float alpha = s_row[is_horizontal ? tid >> 4 : tid & 15];
            __syncthreads();
            if (ok && col >= left && col < right && row >= top && row < bottom) {
                if (alpha > 0) {
                    if (is_horizontal && alpha >= 1.0f && color[3] == 255) solid(color); // setHorizontalSpan over the box's columns
                    else pixel(fade(color, alpha));
                }
            }
            ring(p1x, p1y, 0.0f, half_width, color, ZG_DRAW_SOFT);
            ring(p2x, p2y, 0.0f, half_width, color, ZG_DRAW_SOFT);
            return;
        }
        const float inv_length_sq = 1.0f / length_sq;
        if (!clamp_rect(fminf(p1x, p2x) - half_width, fminf(p1y, p2y) - half_width, fmaxf(p1x, p2x) + half_width + 1, fmaxf(p1y, p2y) + half_width + 1,
                        left, top, right, bottom)) return;
        if (col < left || col >= right || row < top || row >= bottom) return;
        const float dpx = fx - p1x, dpy = fy - p1y;
        const float t = clampf((dpx * dx + dpy * dy) * inv_length_sq, 0.0f, 1.0f);
        const float dist_x = dpx - t * dx, dist_y = dpy - t * dy;
        const float dist = sqrtf(dist_x * dist_x + dist_y * dist_y);
        if (dist > half_width + 0.5f) return;
        float alpha = 1.0f;
        if (dist > half_width - 0.5f) alpha = half_width + 0.5f - dist;
        if (alpha > 0) pixel(fade(color, alpha));
    }

    // evalQuadraticBezier (:1360-1368) and evalCubicBezier (:1373-1383), the sums left to right as written
    __device__ __forceinline__ static CvPoint eval_quadratic(CvPoint p0, CvPoint p1, CvPoint p2, float t) {
        const float u = 1.0f - t, uu = u * u, tt = t * t;
        return {uu * p0.x + 2.0f * u * t * p1.x + tt * p2.x, uu * p0.y + 2.0f * u * t * p1.y + tt * p2.y};
    }
    __device__ __forceinline__ static CvPoint eval_cubic(CvPoint p0, CvPoint p1, CvPoint p2, CvPoint p3, float t) {
        const float u = 1.0f - t, uu = u * u, uuu = uu * u, tt = t * t, ttt = tt * t;
        return {uuu * p0.x + 3.0f * uu * t * p1.x + 3.0f * u * tt * p2.x + ttt * p3.x,
                uuu * p0.y + 3.0f * uu * t * p1.y + 3.0f * u * tt * p2.y + ttt * p3.y};
    }
    // tessellateBezier (:1407-1425): `segments` points at t = i / (segments - 1), one lane each, into s_vx / s_vy from `base` on.
    // The caller's barrier comes before anything reads them.
    __device__ __forceinline__ void tessellate(bool cubic, CvPoint p0, CvPoint p1, CvPoint p2, CvPoint p3, int segments, int base) {
        if (tid < segments) {
            const float t = (float)tid / (float)(segments - 1);
            const CvPoint q = cubic ? eval_cubic(p0, p1, p2, p3, t) : eval_quadratic(p0, p1, p2, t);
            s_vx[base + tid] = q.x; s_vy[base + tid] = q.y;
        }
    }
    // Every kind that is one fillPolygon over points the lanes put into s_vx / s_vy, through one call of poly_fill: fillPolygon itself
    // (:935-1017) and fillSplinePolygon (:1296-1355), every edge's points one after the other. Entered by all lanes together.
    // ARCS: also the soft arc outline of width > 1 (:909-913), fillArcRing's (:919-927) outer ring from arc.start by +step and inner ring
    // from arc.end by -step, 2 (segments + 1) <= 402 points.
    template <bool ARCS> __device__ __forceinline__ void filled(const zg_draw_cmd &c, const float *vertices, Rgba8 color, const CvArc &arc) {
        const float *v = vertices + 2 * (size_t)c.first_vertex;
        int n = (int)c.n_vertices;
        __syncthreads(); // the previous user of s_vx / s_vy has read them
        if (ARCS && c.kind == ZG_DRAW_ARC) { // never taken, and not compiled in, without the flag
            const float line_width = (float)c.width;
            n = 2 * (arc.segments + 1);
            for (int i = tid; i < n; i += 256) {
                const bool outer = i <= arc.segments;
                const float fi = (float)(outer ? i : i - (arc.segments + 1));
                const float radius = outer ? c.p[2] + line_width / 2.0f : c.p[2] - line_width / 2.0f;
                const float angle = outer ? arc.start + fi * arc.step : arc.end + fi * -arc.step;
                s_vx[i] = c.p[0] + radius * dev_cosf(angle); s_vy[i] = c.p[1] + radius * dev_sinf(angle);
            }
        } else if (c.kind == ZG_DRAW_FILL_SPLINE_POLYGON) {
            if (n < 3) return;
            int total = 0;
            for (uint32_t i = 0; i < c.n_vertices; ++i) {
                CvPoint p0, cp1, cp2, p1;
                cv_spline_edge(v, c.n_vertices, i, c.p[0], p0, cp1, cp2, p1);
                const int segments = cv_segments(cv_cubic_length(p0, cp1, cp2, p1), CV_PPS_FAST, CV_SPLINE_MIN_SEGMENTS, CV_SPLINE_MAX_SEGMENTS);
                if (total + segments > CV_POINTS) break; // k_canvas_prep has skipped such a command: never taken
                tessellate(true, p0, cp1, cp2, p1, segments, total);
                total += segments;
            }
            n = total;
        } else {
            if (n < 3) return;
            if (tid < n) { s_vx[tid] = v[2 * tid]; s_vy[tid] = v[2 * tid + 1]; }
        }
        poly_fill(n, color, c.mode);
    }

    // A value every lane holds alike, said so: line() branches round barriers on its arguments
    __device__ __forceinline__ static float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

    // Every kind that is a sequence of drawLine calls, through one call of line() (the routine is large: one copy of it in the kernel):
    // drawLine itself, drawRectangle (:590-601) and drawPolygon (:579-587) with their end points from the command, and the curves, whose
    // points the lanes evaluate into LDS first — drawBezierTessellated (:1428-1455) for drawQuadraticBezier (:1221-1245) and
    // drawCubicBezier (:1249-1275), and drawSplinePolygon (:1280-1291), one cubic per edge. Entered by all lanes together.
    // ARCS: also the soft arc outline of width 1 (:904-908), segments + 1 <= 201 points of fillArcRing (:919-927) and a line per pair.
    template <bool ARCS> __device__ __forceinline__ void outline(const zg_draw_cmd &c, const float *vertices, Rgba8 color, const CvArc &arc) {
        const float *v = vertices + 2 * (size_t)c.first_vertex;
        const bool arc_points = ARCS && c.kind == ZG_DRAW_ARC;
        const bool curve = c.kind >= ZG_DRAW_QUAD_BEZIER || arc_points, spline = c.kind == ZG_DRAW_SPLINE_POLYGON;
        if (!c.width || (spline && c.n_vertices < 3)) return;
        const uint32_t curves = spline ? c.n_vertices : 1u;
        for (uint32_t e = 0; e < curves; ++e) {
            uint32_t calls = c.kind == ZG_DRAW_LINE ? 1u : c.kind == ZG_DRAW_RECT ? 4u : c.n_vertices;
            if (arc_points) { // false, and its branch not compiled in, without the flag
                __syncthreads(); // the previous user of s_vx / s_vy has read them
                if (tid <= arc.segments) {
                    const float angle = arc.start + (float)tid * arc.step;
                    s_vx[CV_CURVE_BASE + tid] = c.p[0] + c.p[2] * dev_cosf(angle); s_vy[CV_CURVE_BASE + tid] = c.p[1] + c.p[2] * dev_sinf(angle);
                }
                __syncthreads();
                calls = (uint32_t)arc.segments;
            } else if (curve) {
                CvPoint p0, p1, p2, p3;
                int segments;
                if (spline) cv_spline_edge(v, c.n_vertices, e, c.p[0], p0, p1, p2, p3);
                else { p0 = {v[0], v[1]}; p1 = {v[2], v[3]}; p2 = {v[4], v[5]}; p3 = c.kind == ZG_DRAW_CUBIC_BEZIER ? CvPoint{v[6], v[7]} : p2; }
                if (c.kind == ZG_DRAW_QUAD_BEZIER) { // estimateQuadraticBezierLength (:1388-1393)
                    const float length = (cv_distance(p0, p2) + (cv_distance(p0, p1) + cv_distance(p1, p2))) / 2.0f;
                    segments = cv_segments(length, CV_PPS_QUADRATIC, CV_QUADRATIC_MIN_SEGMENTS, CV_BEZIER_MAX_SEGMENTS);
                } else {
                    const float pps = (c.mode == ZG_DRAW_SOFT || c.width > 2) ? CV_PPS_SOFT : CV_PPS_FAST;
                    segments = cv_segments(cv_cubic_length(p0, p1, p2, p3), pps, CV_SPLINE_MIN_SEGMENTS, CV_BEZIER_MAX_SEGMENTS);
                }
                __syncthreads(); // the previous user of s_vx / s_vy has read them
                tessellate(c.kind != ZG_DRAW_QUAD_BEZIER, p0, p1, p2, p3, segments, CV_CURVE_BASE);
                __syncthreads();
                calls = (uint32_t)segments - 1u;
            }
            if (curve) { // one lane per segment asks what line() asks first, whether the segment can reach the tile, and only the ones that can are drawn
                bool near = false;
                if (tid < (int)calls) {
                    const float ax = s_vx[CV_CURVE_BASE + tid], ay = s_vy[CV_CURVE_BASE + tid], bx = s_vx[CV_CURVE_BASE + tid + 1], by = s_vy[CV_CURVE_BASE + tid + 1];
                    near = !cv_far_from_segment((float)tx0 + 7.5f, (float)ty0 + 7.5f, ax, ay, bx, by, cv_line_pad(ax, ay, bx, by, c.width, c.mode) + CV_TILE_REACH + 0.5f);
                }
                const unsigned long long ballot = __ballot(near);
                if ((tid & 63) == 0) s_near[tid >> 6] = ballot;
                __syncthreads();
            }
            unsigned long long near_bits = 0;
            for (uint32_t i = 0; i < calls; ++i) {
                if (curve) {
                    if ((i & 63u) == 0) {
                        const unsigned long long m = s_near[i >> 6];
                        near_bits = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
                    }
                    if (!((near_bits >> (i & 63u)) & 1ull)) continue;
                }
                float ax, ay, bx, by;
                if (curve) {
                    ax = uniform(s_vx[CV_CURVE_BASE + i]); ay = uniform(s_vy[CV_CURVE_BASE + i]);
                    bx = uniform(s_vx[CV_CURVE_BASE + i + 1]); by = uniform(s_vy[CV_CURVE_BASE + i + 1]);
                } else if (c.kind == ZG_DRAW_LINE) {
                    ax = c.p[0]; ay = c.p[1]; bx = c.p[2]; by = c.p[3];
                } else if (c.kind == ZG_DRAW_RECT) { // corners (l, t) (r, t) (r, b) (l, b) with r and b one less than the rectangle's
                    const uint32_t j = (i + 1u) & 3u;
                    ax = (i == 1 || i == 2) ? c.p[2] - 1 : c.p[0]; ay = i >= 2 ? c.p[3] - 1 : c.p[1];
                    bx = (j == 1 || j == 2) ? c.p[2] - 1 : c.p[0]; by = j >= 2 ? c.p[3] - 1 : c.p[1];
                } else {
                    const uint32_t j = i + 1 == c.n_vertices ? 0 : i + 1;
                    ax = v[2 * i]; ay = v[2 * i + 1]; bx = v[2 * j]; by = v[2 * j + 1];
                }
                line(ax, ay, bx, by, color, c.width, c.mode);
            }
            if (curve) __syncthreads();
        }
    }

    // One command: the reference's public call
    // ARCS: drawArc (:654-674) and fillArc (:1039-1059) too. What is the same for the whole command — the normalised range, the segment
    // count — is worked out here, once; an arc then takes the circle's, the lines' or the polygon's route below, so that the large routines
    // keep one call site each, or one of the two fills of its own.
    template <bool ARCS> __device__ __forceinline__ void apply(const zg_draw_cmd &c, const float *vertices) {
        const Rgba8 color = rgba_of(c.color);
        int kind = c.kind;
        CvArc arc = {};
        arc.full = true;
        bool arc_lines = false, arc_polygon = false;
        if constexpr (ARCS) {
            if (cv_is_arc(kind)) {
                const float start_angle = vertices[2 * (size_t)c.first_vertex], end_angle = vertices[2 * (size_t)c.first_vertex + 1];
                if (!(c.p[2] > 0) || (kind == ZG_DRAW_ARC && !c.width)) return;
                if (!(fabsf(start_angle) < INFINITY) || !(fabsf(end_angle) < INFINITY)) return;
                if (fabsf(end_angle - start_angle) >= CV_TWO_PI) {
                    kind = kind == ZG_DRAW_ARC ? ZG_DRAW_CIRCLE : ZG_DRAW_FILL_CIRCLE;
                } else {
                    arc = cv_arc_init(start_angle, end_angle, c.p[2]);
                    if (kind == ZG_DRAW_FILL_ARC) {
                        if (c.mode == ZG_DRAW_FAST) arc_fill_fast(c.p[0], c.p[1], c.p[2], color, arc);
                        else arc_fill_soft(c.p[0], c.p[1], c.p[2], color, arc);
                        return;
                    }
                    if (c.mode == ZG_DRAW_FAST) kind = ZG_DRAW_CIRCLE; // drawArcFast (:879-886): drawCircleFast's two routes, gated
                    else if (c.width == 1) arc_lines = true;
                    else arc_polygon = true;
                }
            }
        }
        if (kind == ZG_DRAW_LINE || kind == ZG_DRAW_RECT || kind == ZG_DRAW_POLYGON || kind == ZG_DRAW_QUAD_BEZIER || kind == ZG_DRAW_CUBIC_BEZIER ||
            kind == ZG_DRAW_SPLINE_POLYGON || arc_lines) {
            outline<ARCS>(c, vertices, color, arc);
            return;
        }
        if (kind == ZG_DRAW_FILL_POLYGON || kind == ZG_DRAW_FILL_SPLINE_POLYGON || arc_polygon) {
            filled<ARCS>(c, vertices, color, arc);
            return;
        }
        switch (kind) {
        case ZG_DRAW_FILL_RECT:
            fill_rect(c.p[0], c.p[1], c.p[2], c.p[3], color, c.mode);
            break;
        case ZG_DRAW_CIRCLE: { // :636-644, :863-876
            if (!(c.p[2] > 0) || !c.width) break;
            if (c.mode == ZG_DRAW_FAST && c.width == 1) { circle_bresenham<ARCS>(c.p[0], c.p[1], c.p[2], color, arc); break; }
            const float line_width = (float)c.width;
            ring_t<ARCS>(c.p[0], c.p[1], c.p[2] - line_width / 2.0f, c.p[2] + line_width / 2.0f, color, c.mode, arc);
            break;
        }
        case ZG_DRAW_FILL_CIRCLE: // :1021-1029
            if (!(c.p[2] > 0)) break;
            if (c.mode == ZG_DRAW_SOFT) ring(c.p[0], c.p[1], 0.0f, c.p[2], color, ZG_DRAW_SOFT);
            else disc_fast(c.p[0], c.p[1], c.p[2], color);
            break;
        }
    }
};

template <int PIX, bool ARCS>
__global__ __launch_bounds__(256) void k_canvas(DImg img, const zg_draw_cmd *cmds, uint32_t n, const float *vertices, const ushort4 *boxes) {
    __shared__ float s_vx[CV_POINTS], s_vy[CV_POINTS], s_ix[CV_TILE * CV_POINTS];
    __shared__ float s_row[CV_TILE * 3];
    __shared__ int s_icnt[CV_TILE];
    __shared__ unsigned long long s_near[4];
    Cv<PIX> cv;
    cv.place(img);
    cv.tid = (int)threadIdx.x;
    cv.tx0 = (int)blockIdx.x * CV_TILE; cv.ty0 = (int)blockIdx.y * CV_TILE;
    cv.fx = (float)cv.col; cv.fy = (float)cv.row; cv.fcols = (float)img.cols; cv.frows = (float)img.rows;
    cv.s_vx = s_vx; cv.s_vy = s_vy; cv.s_ix = s_ix; cv.s_icnt = s_icnt; cv.s_row = s_row; cv.s_near = s_near;
    tile_gather<PIX>(
        img, cv, n,
        [&](uint32_t i) { // the box, then for lines and circles, whose boxes are mostly empty, the shape itself
            return tile_meets_box(boxes[i], cv.tx0, cv.ty0) && cv_tile_may_touch<ARCS>(cmds[i], cv.tx0, cv.ty0);
        },
        [&](uint32_t i) { cv.template apply<ARCS>(cmds[i], vertices); });
}

template <typename T> __global__ __launch_bounds__(256) void k_canvas_build(const T *list, const uint32_t *count, uint32_t capacity, float radius, uint32_t color,
                                                                            uint32_t width, int mode, zg_draw_cmd *out, uint32_t *count_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t m = min(*count, capacity);
    if (i == 0) *count_out = m;
    if (i >= m) return;
    zg_draw_cmd c;
    c.mode = mode; c.width = width;
    c.color[0] = (uint8_t)color; c.color[1] = (uint8_t)(color >> 8); c.color[2] = (uint8_t)(color >> 16); c.color[3] = (uint8_t)(color >> 24);
    c.first_vertex = 0; c.n_vertices = 0;
    if constexpr (std::is_same<T, zg_hough_line>::value) {
        c.kind = ZG_DRAW_LINE;
        c.p[0] = list[i].p1[0]; c.p[1] = list[i].p1[1]; c.p[2] = list[i].p2[0]; c.p[3] = list[i].p2[1];
    } else {
        c.kind = ZG_DRAW_CIRCLE;
        c.p[0] = list[i].x; c.p[1] = list[i].y; c.p[2] = radius; c.p[3] = 0.0f;
    }
    out[i] = c;
}

// What every entry point checks first. who: the entry point, as the null checks' messages name it
static int check_draw_args(const zg_image *img, bool device_pointer, const zg_draw_cmd *cmds, uint32_t n, const float *vertices, uint32_t n_vertices, const char *who) {
    if (const int rc = check_draw_image(img, device_pointer, "canvas_draw")) return rc;
    ZG_REQUIRE(n == 0 || cmds != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null cmds", who);
    ZG_REQUIRE(n_vertices == 0 || vertices != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null vertices", who);
    return ZG_OK;
}

// The device lists of entry point `who` drawn into a device image (the host form hands over its staged copies, which pass the checks again).
// arcs: the kernel that knows drawArc and fillArc; without it they are skipped as no kinds
static int canvas_draw(const zg_image *img, const zg_draw_cmd *cmds, uint32_t n, const uint32_t *count_device, const float *vertices, uint32_t n_vertices,
                       hipStream_t s, bool arcs, const char *who) {
    if (const int rc = check_draw_args(img, true, cmds, n, vertices, n_vertices, who)) return rc;
    ZG_REQUIRE(n <= ZG_CANVAS_MAX_COMMANDS, ZG_ERR_UNSUPPORTED, "canvas_draw: %u commands (at most %u a call)", n, ZG_CANVAS_MAX_COMMANDS);
    if (n == 0 || img->rows == 0 || img->cols == 0) return ZG_OK;
    ScratchBlock sc(s);
    ushort4 *boxes;
    sc.take(boxes, n);
    int rc;
    if ((rc = sc.alloc())) return rc;
    k_canvas_prep<<<ceil_div(n, 256), 256, 0, s>>>(cmds, n, count_device, vertices, n_vertices, (int)img->rows, (int)img->cols, boxes, arcs);
    if ((rc = launch_ok("k_canvas_prep"))) return rc;
    const dim3 grid = tile_grid(img);
    const DImg d = dimg(img);
    dispatch_u8_pixel(img->pixel, [&](auto pix) {
        constexpr int PIX = decltype(pix)::value;
        if (arcs) k_canvas<PIX, true><<<grid, 256, 0, s>>>(d, cmds, n, vertices, boxes);
        else k_canvas<PIX, false><<<grid, 256, 0, s>>>(d, cmds, n, vertices, boxes);
    });
    return launch_ok(arcs ? "k_canvas (arcs)" : "k_canvas");
}

static int check_builder(const uint32_t *count, const uint8_t *color, uint32_t width, int mode, const uint32_t *count_out, const char *what) {
    ZG_REQUIRE(count != nullptr && count_out != nullptr && color != nullptr, ZG_ERR_INVALID_ARGUMENT, "%s: null count, count_out or color", what);
    ZG_REQUIRE(mode == ZG_DRAW_FAST || mode == ZG_DRAW_SOFT, ZG_ERR_INVALID_ARGUMENT, "%s: mode %d", what, mode);
    ZG_REQUIRE(width <= ZG_CANVAS_MAX_WIDTH, ZG_ERR_INVALID_ARGUMENT, "%s: width %u (at most %u)", what, width, ZG_CANVAS_MAX_WIDTH);
    return ZG_OK;
}

} // namespace zg

using namespace zg;

extern "C" {

size_t zg_sizeof_draw_cmd(void) { return sizeof(zg_draw_cmd); }
uint32_t zg_canvas_tile(void) { return CV_TILE; }

int zg_canvas_draw(const zg_image *img, const zg_draw_cmd *cmds, uint32_t n, const uint32_t *count_device, const float *vertices, uint32_t n_vertices,
                   zg_stream stream) {
    return canvas_draw(img, cmds, n, count_device, vertices, n_vertices, as_stream(stream), false, "canvas_draw");
}

int zg_canvas_draw_arcs(const zg_image *img, const zg_draw_cmd *cmds, uint32_t n, const uint32_t *count_device, const float *vertices, uint32_t n_vertices,
                        zg_stream stream) {
    return canvas_draw(img, cmds, n, count_device, vertices, n_vertices, as_stream(stream), true, "canvas_draw_arcs");
}

int zg_canvas_draw_host(const zg_image *img, const zg_draw_cmd *cmds, uint32_t n, const float *vertices, uint32_t n_vertices) {
    if (const int rc = check_draw_args(img, false, cmds, n, vertices, n_vertices, "canvas_draw")) return rc;
    bool arcs = false; // the host sees the list: the larger kernel only when it holds an arc
    for (uint32_t i = 0; i < n; ++i) {
        const int bad = cv_check(cmds[i], vertices, n_vertices, true);
        arcs = arcs || cv_is_arc(cmds[i].kind);
        ZG_REQUIRE(bad != 2, ZG_ERR_UNSUPPORTED, "canvas_draw: command %u is a polygon of %u vertices (at most %u)", i, cmds[i].n_vertices, ZG_CANVAS_MAX_VERTICES);
        ZG_REQUIRE(bad != 3, ZG_ERR_UNSUPPORTED, "canvas_draw: command %u is a filled spline polygon of more than %u points", i, ZG_CANVAS_MAX_CURVE_POINTS);
        ZG_REQUIRE(bad == 0, ZG_ERR_INVALID_ARGUMENT,
                   "canvas_draw: command %u is outside the contract (kind, mode, finite parameters of magnitude <= %g, width <= %u, vertex range or count)", i,
                   (double)ZG_CANVAS_MAX_COORD, ZG_CANVAS_MAX_WIDTH);
    }
    if (n == 0) return ZG_OK;
    ScratchBlock sc;
    zg_draw_cmd *dcmds;
    float *dvertices;
    sc.take(dcmds, n);
    sc.take(dvertices, 2 * (size_t)n_vertices + 1);
    int rc;
    if ((rc = sc.alloc())) return rc;
    if ((rc = upload_pageable(dcmds, cmds, (size_t)n * sizeof(zg_draw_cmd), nullptr))) return rc;
    if (n_vertices && (rc = upload_pageable(dvertices, vertices, 2 * (size_t)n_vertices * sizeof(float), nullptr))) return rc;
    return host_in_place(img, true, [&](const zg_image *d) { return canvas_draw(d, dcmds, n, nullptr, dvertices, n_vertices, nullptr, arcs, "canvas_draw"); });
}

int zg_canvas_cmds_from_hough_lines(const zg_hough_line *lines, const uint32_t *counts, uint32_t capacity, const uint8_t *color, uint32_t width, int mode,
                                    zg_draw_cmd *cmds_out, uint32_t *count_out, zg_stream stream) {
    if (const int rc = check_builder(counts, color, width, mode, count_out, "canvas_cmds_from_hough_lines")) return rc;
    ZG_REQUIRE(capacity == 0 || (lines != nullptr && cmds_out != nullptr), ZG_ERR_INVALID_ARGUMENT, "canvas_cmds_from_hough_lines: null lines or cmds_out");
    uint32_t packed;
    std::memcpy(&packed, color, 4);
    k_canvas_build<zg_hough_line><<<ceil_div(capacity ? capacity : 1u, 256), 256, 0, as_stream(stream)>>>(lines, counts + 1, capacity, 0.0f, packed, width, mode, cmds_out,
                                                                                                    count_out);
    return launch_ok("k_canvas_build");
}

int zg_canvas_cmds_from_keypoints(const zg_keypoint *keypoints, const uint32_t *count, uint32_t capacity, float radius, const uint8_t *color, uint32_t width,
                                  int mode, zg_draw_cmd *cmds_out, uint32_t *count_out, zg_stream stream) {
    if (const int rc = check_builder(count, color, width, mode, count_out, "canvas_cmds_from_keypoints")) return rc;
    ZG_REQUIRE(capacity == 0 || (keypoints != nullptr && cmds_out != nullptr), ZG_ERR_INVALID_ARGUMENT, "canvas_cmds_from_keypoints: null keypoints or cmds_out");
    ZG_REQUIRE(std::fabs(radius) <= ZG_CANVAS_MAX_COORD, ZG_ERR_INVALID_ARGUMENT, "canvas_cmds_from_keypoints: radius %g", (double)radius);
    uint32_t packed;
    std::memcpy(&packed, color, 4);
    k_canvas_build<zg_keypoint><<<ceil_div(capacity ? capacity : 1u, 256), 256, 0, as_stream(stream)>>>(keypoints, count, capacity, radius, packed, width, mode, cmds_out,
                                                                                                  count_out);
    return launch_ok("k_canvas_build");
}

} // extern "C"

/* zignal_hip_canvas.h — the Canvas module of libzignal_hip.so: Canvas(T)'s lines, rectangles, circles, arcs, polygons, Bézier curves and
 * spline polygons (reference src/canvas/Canvas.zig) as one device operation that executes a list of draw commands into an image in place. Included by zignal_hip.h
 * (include that one); zg_image, zg_stream, zg_keypoint and the status codes come from there, zg_hough_line from zignal_hip_hough.h. */
#ifndef ZIGNAL_HIP_CANVAS_H
#define ZIGNAL_HIP_CANVAS_H

#include "zignal_hip.h"
#include "zignal_hip_hough.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- canvas: drawLine, drawRectangle, fillRectangle, drawCircle, fillCircle, drawPolygon, fillPolygon ------------------------- */

#define ZG_DRAW_LINE 0         /* drawLine(p1, p2, color, width, mode)              p = x1 y1 x2 y2  (Canvas.zig:152-487) */
#define ZG_DRAW_RECT 1         /* drawRectangle(rect, color, width, mode)           p = l t r b      (:590-601) */
#define ZG_DRAW_FILL_RECT 2    /* fillRectangle(rect, color, mode)                  p = l t r b      (:608-632) */
#define ZG_DRAW_CIRCLE 3       /* drawCircle(center, radius, color, width, mode)    p = cx cy radius (:636-644) */
#define ZG_DRAW_FILL_CIRCLE 4  /* fillCircle(center, radius, color, mode)           p = cx cy radius (:1021-1029) */
#define ZG_DRAW_POLYGON 5      /* drawPolygon(vertices, color, width, mode)         first_vertex, n_vertices (:579-587) */
#define ZG_DRAW_FILL_POLYGON 6 /* fillPolygon(vertices, color, mode)                first_vertex, n_vertices (:935-1017) */
/* Kinds 7-15 are no kinds. The arcs are kinds of zg_canvas_draw_arcs and zg_canvas_draw_host only; to zg_canvas_draw, 16 and 17 are no
 * kinds either. Their two angles (radians from the positive x axis towards positive y, as the reference takes them) travel as one entry
 * of the vertex array, vertices[first_vertex] = (start_angle, end_angle): n_vertices must be exactly 1, p[3] is ignored. */
#define ZG_DRAW_ARC 16       /* drawArc(center, radius, start, end, color, width, mode)   p = cx cy radius; angles in one vertex (:646-674, :878-927) */
#define ZG_DRAW_FILL_ARC 17  /* fillArc(center, radius, start, end, color, mode)          p = cx cy radius; angles in one vertex (:1039-1059, :1086-1218) */
/* The curves take their points from the vertex array: */
#define ZG_DRAW_QUAD_BEZIER 18         /* drawQuadraticBezier(p0, p1, p2, color, width, mode)   n_vertices == 3 (:1221-1245) */
#define ZG_DRAW_CUBIC_BEZIER 19        /* drawCubicBezier(p0, p1, p2, p3, color, width, mode)   n_vertices == 4 (:1249-1275) */
#define ZG_DRAW_SPLINE_POLYGON 20      /* drawSplinePolygon(vertices, color, width, tension, mode)  vertex range, p[0] = tension (:1280-1291) */
#define ZG_DRAW_FILL_SPLINE_POLYGON 21 /* fillSplinePolygon(vertices, color, tension, mode)         vertex range, p[0] = tension (:1296-1355) */

#define ZG_DRAW_FAST 0 /* DrawMode.fast: hard edges */
#define ZG_DRAW_SOFT 1 /* DrawMode.soft: antialiased edges, Rgba alpha honoured */

#define ZG_CANVAS_MAX_VERTICES 64u  /* vertices of one polygon or spline polygon: the reference's stack buffer (Canvas.zig:52) */
/* points of the polygon a filled spline polygon is tessellated into: the sum over its edges of clamp(trunc(length / 3), 4, 50), length
 * being the reference's estimate for the edge's cubic (:1318-1328). The reference spills to the heap past 400; this is the library's bound.
 * It also holds the polygon a soft arc outline of width > 1 is filled as: 2 (segments + 1) points, segments =
 * max(8, min(200, ceil(span * radius / 5))), 402 at the most (:889-913). */
#define ZG_CANVAS_MAX_CURVE_POINTS 512u
#define ZG_CANVAS_MAX_COORD 65536.0f /* every float parameter and vertex coordinate: finite and |v| <= this */
#define ZG_CANVAS_MAX_WIDTH 65536u  /* width */
#define ZG_CANVAS_MAX_SIZE 32768u   /* rows and cols of the image drawn into */
#define ZG_CANVAS_MAX_COMMANDS 16777216u /* n of one call */

/* One call of the reference's Canvas(T) with an Rgba(u8) colour. The .fast paths store convertColor(T, color). Everything else goes
 * through setPixel, which converts the (faded) colour to the pixel type before assignPixel sees it: an Rgba(u8) image is composited
 * into with Rgba.blend(.normal) when a != 255; a u8 or Rgb(u8) image is stored to with convertColor(T, color) whatever the alpha —
 * soft edges and translucent colours overwrite there, exactly as in the reference. width is ignored by the fills; width == 0, radius <= 0 and a filled polygon of
 * fewer than 3 vertices draw nothing, as in the reference (drawPolygon draws its edges whatever their number); so do a Bézier of width 0
 * and a spline polygon of width 0 (the outline) or of fewer than 3 vertices. An arc of radius <= 0, an arc outline of width 0, an arc
 * with a NaN or infinite angle and a fast filled arc of span <= 0 draw nothing; an arc with |end - start| >= 2 pi (in f32) is the circle;
 * any other pair of finite angles is normalised as ArcRange.init does (:679-701). 40 bytes, no padding. */
typedef struct zg_draw_cmd {
    int32_t kind;  /* ZG_DRAW_* */
    int32_t mode;  /* ZG_DRAW_FAST | ZG_DRAW_SOFT */
    uint32_t width;
    uint8_t color[4]; /* r g b a */
    float p[4];
    uint32_t first_vertex, n_vertices; /* polygons and curves: vertices[first_vertex .. first_vertex + n_vertices) of the call's vertex array; arcs: the angle pair */
} zg_draw_cmd;
/* sizeof(zg_draw_cmd) as the library was built: a binding that declares the struct itself compares and refuses to go on when they
 * differ (the zg_sizeof_step rule). */
ZG_API size_t zg_sizeof_draw_cmd(void);
/* The side of the square pixel tiles a workgroup rasterises (tests put shapes on both sides of it). */
ZG_API uint32_t zg_canvas_tile(void);

/* Executes cmds[0 .. count) in list order into img (u8, Rgb(u8) or Rgba(u8); another type: ZG_ERR_UNSUPPORTED; rows or cols above
 * ZG_CANVAS_MAX_SIZE: ZG_ERR_UNSUPPORTED), in place. The result equals the reference making the same calls one after another, byte
 * for byte: a pixel's lane keeps the pixel in a register, applies every write that any command makes to that pixel in the
 * reference's order — repeated writes repeated (the eight symmetric points of a Bresenham circle, the end points of a short Wu line,
 * spans of a polygon that share a pixel; it matters on Rgba(u8), where they blend) — and stores once. Pixels that nothing writes are not stored; bytes between cols and stride
 * are never touched.
 * cmds: n commands on the device. count_device: NULL (count = n), or a device word holding the count, of which min(word, n) are
 * executed. vertices: n_vertices float pairs (x, y) on the device, NULL when n_vertices is 0.
 * A command outside the contract — a kind or mode that is none of the above, a float parameter or vertex that is not finite or
 * exceeds ZG_CANVAS_MAX_COORD in magnitude, a width above ZG_CANVAS_MAX_WIDTH, more than ZG_CANVAS_MAX_VERTICES vertices or a vertex
 * range outside the array (the reference would trap in its @trunc casts or index past a slice), a Bézier whose n_vertices is not its
 * number of control points, a spline polygon's tension that is not finite, a filled spline polygon of more than
 * ZG_CANVAS_MAX_CURVE_POINTS points, an arc (every arc here; in zg_canvas_draw_arcs one whose n_vertices is not 1, whose angle pair lies
 * outside the array or whose centre or radius breaks the rule for float parameters: the rule does not apply to the two angles) — is
 * skipped on the device.
 * n above ZG_CANVAS_MAX_COMMANDS: ZG_ERR_UNSUPPORTED. Cost: every tile tests every command's box; a width-1 soft line and a width-1 fast
 * circle are re-walked from their start by the tiles they cross, so their time grows with their length as well as with the tiles; a
 * Bézier is its 3 to 200 lines, each tested against the tile before it is drawn.
 * Asynchronous on `stream`, two launches, 8 bytes of scratch per command, no host synchronisation, copy or upload, recordable into a
 * graph from a process's first call. In a process without a device the call answers its argument errors, then ZG_ERR_HIP. */
ZG_API int zg_canvas_draw(const zg_image *img, const zg_draw_cmd *cmds, uint32_t n, const uint32_t *count_device, const float *vertices,
                          uint32_t n_vertices, zg_stream stream);

/* zg_canvas_draw with ZG_DRAW_ARC and ZG_DRAW_FILL_ARC among the kinds: the same arguments, contract, launches and scratch, and the same
 * result for a list without arcs. It is an entry point of its own because its kernel is the larger one: with the arcs' code in it a list
 * that holds no arc runs slower too, so zg_canvas_draw keeps the kernel without them and the caller, who built the list and knows whether
 * it may hold an arc, chooses. Cost of the arcs: the fast outlines and both fills are tested per pixel of the circle's box (a fast outline
 * of width 1 is the re-walked Bresenham circle; a fast fill re-walks its row's x sequence a binade at a time); a soft outline of width 1
 * is 8 to 200 Wu lines, each tested against the tile and re-walked by the tiles it crosses; a soft outline of width > 1 is one filled
 * polygon of up to 402 points. */
ZG_API int zg_canvas_draw_arcs(const zg_image *img, const zg_draw_cmd *cmds, uint32_t n, const uint32_t *count_device, const float *vertices,
                               uint32_t n_vertices, zg_stream stream);

/* Host pointers (img->data, cmds, vertices), synchronous. Arcs are among the kinds: the call sees the list and takes the larger kernel
 * only when it holds one. Here a command outside the contract is refused before anything is drawn:
 * ZG_ERR_UNSUPPORTED for a polygon or spline polygon of more than ZG_CANVAS_MAX_VERTICES vertices and for a filled spline polygon of
 * more than ZG_CANVAS_MAX_CURVE_POINTS points, ZG_ERR_INVALID_ARGUMENT for everything else. */
ZG_API int zg_canvas_draw_host(const zg_image *img, const zg_draw_cmd *cmds, uint32_t n, const float *vertices, uint32_t n_vertices);

/* Device-side builders, one lane per entry, so that a detector's list becomes a command list without the host seeing either.
 * zg_canvas_cmds_from_hough_lines: one ZG_DRAW_LINE from p1 to p2 per line of zg_hough_find_lines; counts is that call's two device
 * words (counts[1] = the number of lines). zg_canvas_cmds_from_keypoints: one ZG_DRAW_CIRCLE of `radius` at each keypoint's (x, y);
 * count is the detector's device count word. capacity is the length of the list and of cmds_out: min(count, capacity) commands are
 * written and *count_out (a device word, the count_device of zg_canvas_draw) receives that number. color: four host bytes, r g b a.
 * Asynchronous on `stream`, one launch, no synchronisation, recordable into a graph. */
ZG_API int zg_canvas_cmds_from_hough_lines(const zg_hough_line *lines, const uint32_t *counts, uint32_t capacity, const uint8_t *color,
                                           uint32_t width, int mode, zg_draw_cmd *cmds_out, uint32_t *count_out, zg_stream stream);
ZG_API int zg_canvas_cmds_from_keypoints(const zg_keypoint *keypoints, const uint32_t *count, uint32_t capacity, float radius,
                                         const uint8_t *color, uint32_t width, int mode, zg_draw_cmd *cmds_out, uint32_t *count_out,
                                         zg_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* ZIGNAL_HIP_CANVAS_H */

"""Canvas(T)'s Bézier curves and spline polygons restated call by call (reference src/canvas/Canvas.zig:1221-1472), on top of
tests/canvas_ref.py's Canvas: sequential, scalar np.float32, the reference's expressions in the reference's order. The yardstick of
tests/test_gpu_canvas_curves.py; tests/test_canvas_curves_oracle.py pins it to the reference's own MD5 sums
(tests/golden/canvas_curves_md5.json: each call's parameters transcribed as data from src/canvas/tests/regression.zig, with the MD5 the
reference records for it).

A curve command is canvas_ref's dict with pts (the control points or the polygon) and, for the spline polygons, p = [tension]."""
from __future__ import annotations

import json
import os

import numpy as np

from tests import canvas_ref as ref
from tests.canvas_ref import F, FAST, SOFT

KIND_QUAD_BEZIER, KIND_CUBIC_BEZIER, KIND_SPLINE_POLYGON, KIND_FILL_SPLINE_POLYGON = 18, 19, 20, 21
CURVE_KINDS = (KIND_QUAD_BEZIER, KIND_CUBIC_BEZIER, KIND_SPLINE_POLYGON, KIND_FILL_SPLINE_POLYGON)
MAX_CURVE_POINTS = 512  # ZG_CANVAS_MAX_CURVE_POINTS
# :36-48
BEZIER_MAX_SEGMENTS, SPLINE_MAX_SEGMENTS, SPLINE_MIN_SEGMENTS, QUADRATIC_MIN_SEGMENTS = 200, 50, 4, 3
PPS_SOFT, PPS_FAST, PPS_QUADRATIC = F(1.5), F(3.0), F(2.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canvas_curves_md5.json")
_TWO, _THREE = F(2.0), F(3.0)


def _pt(p):
    return (F(p[0]), F(p[1]))


def _distance(a, b):  # Point.distance: sub, dot with itself, @sqrt
    dx, dy = F(a[0] - b[0]), F(a[1] - b[1])
    return np.sqrt(F(F(dx * dx) + F(dy * dy)))


def eval_quadratic(p0, p1, p2, t):  # :1360-1368
    u = F(F(1.0) - t)
    uu, tt = F(u * u), F(t * t)
    k = F(F(_TWO * u) * t)
    return tuple(F(F(F(uu * p0[i]) + F(k * p1[i])) + F(tt * p2[i])) for i in range(2))


def eval_cubic(p0, p1, p2, p3, t):  # :1373-1383
    u = F(F(1.0) - t)
    uu = F(u * u)
    uuu = F(uu * u)
    tt = F(t * t)
    ttt = F(tt * t)
    k1, k2 = F(F(_THREE * uu) * t), F(F(_THREE * u) * tt)
    return tuple(F(F(F(F(uuu * p0[i]) + F(k1 * p1[i])) + F(k2 * p2[i])) + F(ttt * p3[i])) for i in range(2))


def quadratic_length(p0, p1, p2):  # :1388-1393
    chord = _distance(p0, p2)
    control_net = F(_distance(p0, p1) + _distance(p1, p2))
    return F(F(chord + control_net) / _TWO)


def cubic_length(p0, p1, p2, p3):  # :1398-1403
    chord = _distance(p0, p3)
    control_net = F(F(_distance(p0, p1) + _distance(p1, p2)) + _distance(p2, p3))
    return F(F(chord + control_net) / _TWO)


def segment_count(length, pixels_per_segment, min_segments, max_segments):  # :1416
    return max(min_segments, min(max_segments, int(np.trunc(F(length / pixels_per_segment)))))


def tessellate(length, pixels_per_segment, min_segments, max_segments, eval_fn, args):  # :1407-1425
    segments = segment_count(length, pixels_per_segment, min_segments, max_segments)
    return [eval_fn(*args, F(F(i) / F(segments - 1))) for i in range(segments)]


def smooth_control_points(p0, p1, p2, tension):  # :1460-1472
    tf = F(F(1.0) - ref._clamp(tension, 0, 1))
    cp1 = tuple(F(p0[i] + F(F(p1[i] - p0[i]) * tf)) for i in range(2))
    cp2 = tuple(F(p1[i] - F(F(p2[i] - p1[i]) * tf)) for i in range(2))
    return cp1, cp2


def spline_fill_points(points, tension):
    """fillSplinePolygon's total_points (:1318-1328)."""
    pts = [_pt(p) for p in points]
    n = len(pts)
    total = 0
    for i in range(n):
        p0, p1, p2 = pts[i], pts[(i + 1) % n], pts[(i + 2) % n]
        cp1, cp2 = smooth_control_points(p0, p1, p2, F(tension))
        total += segment_count(cubic_length(p0, cp1, cp2, p1), PPS_FAST, SPLINE_MIN_SEGMENTS, SPLINE_MAX_SEGMENTS)
    return total


class Canvas(ref.Canvas):
    def _bezier_tessellated(self, length, pps, min_segments, eval_fn, args, color, width, mode):  # :1428-1455
        pts = tessellate(length, pps, min_segments, BEZIER_MAX_SEGMENTS, eval_fn, args)
        for i in range(1, len(pts)):
            self.draw_line(pts[i - 1], pts[i], color, width, mode)

    def draw_quadratic_bezier(self, p0, p1, p2, color, width, mode):  # :1221-1245
        if width == 0:
            return
        p0, p1, p2 = _pt(p0), _pt(p1), _pt(p2)
        self._bezier_tessellated(quadratic_length(p0, p1, p2), PPS_QUADRATIC, QUADRATIC_MIN_SEGMENTS, eval_quadratic, (p0, p1, p2), color, width, mode)

    def draw_cubic_bezier(self, p0, p1, p2, p3, color, width, mode):  # :1249-1275
        if width == 0:
            return
        p0, p1, p2, p3 = _pt(p0), _pt(p1), _pt(p2), _pt(p3)
        pps = PPS_SOFT if (mode == SOFT or width > 2) else PPS_FAST
        self._bezier_tessellated(cubic_length(p0, p1, p2, p3), pps, SPLINE_MIN_SEGMENTS, eval_cubic, (p0, p1, p2, p3), color, width, mode)

    def draw_spline_polygon(self, points, color, width, tension, mode):  # :1280-1291
        n = len(points)
        if width == 0 or n < 3:
            return
        pts = [_pt(p) for p in points]
        for i in range(n):
            p0, p1, p2 = pts[i], pts[(i + 1) % n], pts[(i + 2) % n]
            cp1, cp2 = smooth_control_points(p0, p1, p2, F(tension))
            self.draw_cubic_bezier(p0, cp1, cp2, p1, color, width, mode)

    def fill_spline_polygon(self, points, color, tension, mode):  # :1296-1355
        n = len(points)
        if n < 3:
            return
        pts = [_pt(p) for p in points]
        buffer = []
        for i in range(n):
            p0, p1, p2 = pts[i], pts[(i + 1) % n], pts[(i + 2) % n]
            cp1, cp2 = smooth_control_points(p0, p1, p2, F(tension))
            buffer += tessellate(cubic_length(p0, cp1, cp2, p1), PPS_FAST, SPLINE_MIN_SEGMENTS, SPLINE_MAX_SEGMENTS, eval_cubic, (p0, cp1, cp2, p1))
        self.fill_polygon(buffer, color, mode)


def run(image: np.ndarray, commands) -> np.ndarray:
    """canvas_ref.run over the old kinds and the curves: one reference call per command, in order, on a copy of `image`."""
    out = image.copy()
    cv = Canvas(out)
    for c in commands:
        kind = c["kind"]
        if kind not in CURVE_KINDS:
            out[...] = ref.run(out, [c])
            continue
        mode, width, color, pts = c.get("mode", FAST), c.get("width", 1), tuple(int(v) for v in c["color"]), c["pts"]
        if kind == KIND_QUAD_BEZIER:
            cv.draw_quadratic_bezier(*pts, color, width, mode)
        elif kind == KIND_CUBIC_BEZIER:
            cv.draw_cubic_bezier(*pts, color, width, mode)
        elif kind == KIND_SPLINE_POLYGON:
            cv.draw_spline_polygon(pts, color, width, c["p"][0], mode)
        else:
            cv.fill_spline_polygon(pts, color, c["p"][0], mode)
    return out


# ---- command builders (tests/canvas_cases.py's form)
OPAQUE, TRANSLUCENT = (200, 60, 120, 255), (40, 180, 90, 128)


def quad_bezier(p0, p1, p2, color=OPAQUE, width=1, mode=FAST):
    return {"kind": KIND_QUAD_BEZIER, "mode": mode, "width": width, "color": color, "pts": [tuple(p0), tuple(p1), tuple(p2)]}


def cubic_bezier(p0, p1, p2, p3, color=OPAQUE, width=1, mode=FAST):
    return {"kind": KIND_CUBIC_BEZIER, "mode": mode, "width": width, "color": color, "pts": [tuple(p0), tuple(p1), tuple(p2), tuple(p3)]}


def spline_polygon(pts, color=OPAQUE, width=1, tension=0.5, mode=FAST):
    return {"kind": KIND_SPLINE_POLYGON, "mode": mode, "width": width, "color": color, "pts": [tuple(p) for p in pts], "p": [tension]}


def fill_spline_polygon(pts, color=OPAQUE, tension=0.5, mode=FAST):
    return {"kind": KIND_FILL_SPLINE_POLYGON, "mode": mode, "width": 1, "color": color, "pts": [tuple(p) for p in pts], "p": [tension]}


_CALLS = {"quad_bezier": KIND_QUAD_BEZIER, "cubic_bezier": KIND_CUBIC_BEZIER, "spline_polygon": KIND_SPLINE_POLYGON,
          "fill_spline_polygon": KIND_FILL_SPLINE_POLYGON}


def golden_cases():
    """(name, md5, command) of the recorded curve cases of the reference's regression list, and the fixture's header."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for c in doc["cases"]:
        cmd = {"kind": _CALLS[c["call"]], "mode": {"fast": FAST, "soft": SOFT}[c["mode"]], "width": c["width"], "color": tuple(c["color"]),
               "pts": [tuple(p) for p in c["pts"]]}
        if "tension" in c:
            cmd["p"] = [c["tension"]]
        out.append((c["name"], c["md5"], cmd))
    return doc, out


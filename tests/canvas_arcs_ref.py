"""Canvas(T)'s drawArc and fillArc restated call by call (reference src/canvas/Canvas.zig:646-927, :1039-1218), on top of
tests/canvas_ref.py's and tests/canvas_curves_ref.py's Canvas: sequential, scalar np.float32, one rounding per operation, the reference's
expressions in the reference's order; atan2, sin and cos are the oracle library's musl restatements (what Zig uses for f32). The yardstick
of tests/test_gpu_canvas_arcs.py; tests/test_canvas_arcs_oracle.py pins it to the reference's own MD5 sums
(tests/golden/canvas_arcs_md5.json: each call's parameters transcribed as data from src/canvas/tests/regression.zig, with the MD5 the
reference records for it).

An arc command is canvas_ref's dict with p = [cx, cy, radius] and pts = [(start_angle, end_angle)]: the angle pair travels as one vertex.

`2 * std.math.pi` and `std.math.pi` are comptime values rounded to f32 where they meet an f32. One thing the sums do not pin is how the
compiler lowers @mod(angle, 2 pi) for a negative f32: MOD_FORM 1 (used; a < 0 ? fmod(fmod(a, b) + b, b) : fmod(a, b)) and MOD_FORM 0
(r = fmod(a, b); r < 0 ? r + b : r) differ only when fmod(a, b) lies in about (-2.4e-7, 0); the suites keep their angles out of
(-1e-6, 0) modulo 2 pi and check that both forms agree on every angle they use."""
from __future__ import annotations

import ctypes as C
import json
import math
import os

import numpy as np

from oracle import pyoracle
from tests import canvas_curves_ref as cref
from tests import canvas_ref as ref
from tests.canvas_ref import F, FAST, SOFT

KIND_ARC, KIND_FILL_ARC = 16, 17
ARC_KINDS = (KIND_ARC, KIND_FILL_ARC)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canvas_arcs_md5.json")
TWO_PI, PI = F(2 * math.pi), F(math.pi)
ARC_MIN_SEGMENTS, ARC_MAX_SEGMENTS = 8, 200
MOD_FORM = 1
_ONE, _ZERO, _HALF, _TWO = F(1.0), F(0.0), F(0.5), F(2.0)
_EPS = F(1e-5)


def _lib():
    l = pyoracle.lib()
    l.zo_atan2f.restype = C.c_float
    l.zo_atan2f.argtypes = [C.c_float, C.c_float]
    return l


def atan2(y, x):
    return F(_lib().zo_atan2f(C.c_float(float(y)), C.c_float(float(x))))  # float() keeps the sign of a zero


def sin(x):
    return F(_lib().zo_sinf(C.c_float(float(x))))


def cos(x):
    return F(_lib().zo_cosf(C.c_float(float(x))))


def _fmod(a, b):  # exact
    return F(np.fmod(F(a), F(b)))


def normalize(angle, form=None):  # ArcRange.normalize (:697-701)
    form = MOD_FORM if form is None else form
    a = F(angle)
    r = _fmod(a, TWO_PI)
    if form == 0:
        n = F(r + TWO_PI) if r < 0 else r
    else:
        n = _fmod(F(r + TWO_PI), TWO_PI) if a < 0 else r
    if n < 0:
        n = F(n + TWO_PI)
    return n


class ArcRange:  # :679-750
    def __init__(self, start, end):
        ns, ne = normalize(start), normalize(end)
        if ne < ns:
            ne = F(ne + TWO_PI)
        self.start, self.end = ns, ne

    def contains(self, angle):
        norm_angle = F(angle + TWO_PI) if angle < 0 else angle
        if self.start <= norm_angle <= self.end:
            return True
        shifted = F(norm_angle + TWO_PI)
        return self.start <= shifted <= self.end

    def span(self):
        return F(self.end - self.start)

    def is_long(self):
        return self.span() > PI

    def is_full(self):
        return self.span() >= TWO_PI

    def contains_cross(self, start_cross, end_cross):
        a, b = start_cross <= 0, end_cross >= 0
        return (a or b) if self.is_long() else (a and b)


def arc_segments(arc, radius):  # :890-893
    length = F(arc.span() * radius)
    segments = max(ARC_MIN_SEGMENTS, min(ARC_MAX_SEGMENTS, int(np.ceil(F(length / F(5.0))))))
    return segments, F(arc.span() / F(segments))


def arc_ring_points(n, center, radius, start_angle, angle_step):  # fillArcRing (:919-927)
    out = []
    for i in range(n):
        angle = F(start_angle + F(F(i) * angle_step))
        out.append((F(center[0] + F(radius * cos(angle))), F(center[1] + F(radius * sin(angle)))))
    return out


class Canvas(cref.Canvas):
    def _render_ring_arc(self, center, inner, outer, color, arc, mode):  # renderRing (:794-822) with a partial arc
        bbox = self._ring_bbox(center, outer)
        if bbox is None:
            return
        l, t, r, b = bbox
        solid = self._convert(color)
        full = arc.is_full()
        for row in range(t, b):
            y = F(F(row) - center[1])
            for col in range(l, r):
                x = F(F(col) - center[0])
                coverage = self._ring_coverage(x, y, inner, outer, mode)
                if coverage <= 0:
                    continue
                if not full and not arc.contains(atan2(y, x)):
                    continue
                if mode == SOFT:
                    self.set_pixel(row, col, ref.fade(color, coverage))
                else:
                    self._store(row, col, solid)

    def _bresenham_arc(self, center, radius, color, arc):  # drawBresenhamCircle (:826-860) with a partial arc
        cx, cy, r = ref._round(center[0]), ref._round(center[1]), ref._round(radius)
        x, y, err = F(r), _ZERO, _ZERO
        full = arc.is_full()
        while x >= y:
            for ox, oy in ((x, y), (-x, y), (x, -y), (-x, -y), (y, x), (-y, x), (y, -x), (-y, -x)):  # np.float32 negation keeps -0
                if not full and not arc.contains(atan2(oy, ox)):
                    continue
                self.set_point(F(cx + ox), F(cy + oy), color)
            if err <= 0:
                y = F(y + _ONE)
                err = F(err + F(F(_TWO * y) + _ONE))
            if err > 0:
                x = F(x - _ONE)
                err = F(err - F(F(_TWO * x) + _ONE))

    def draw_arc(self, center, radius, start_angle, end_angle, color, width, mode):  # :654-674
        center, radius = (F(center[0]), F(center[1])), F(radius)
        start_angle, end_angle = F(start_angle), F(end_angle)
        if radius <= 0 or width == 0:
            return
        if not (np.isfinite(start_angle) and np.isfinite(end_angle)):
            return
        if abs(F(end_angle - start_angle)) >= TWO_PI:
            self.draw_circle(center, radius, color, width, mode)
            return
        arc = ArcRange(start_angle, end_angle)
        line_width = F(width)
        if mode == FAST:  # drawArcFast (:879-886)
            if width == 1:
                self._bresenham_arc(center, radius, color, arc)
            else:
                self._render_ring_arc(center, F(radius - F(line_width / _TWO)), F(radius + F(line_width / _TWO)), color, arc, FAST)
            return
        segments, angle_step = arc_segments(arc, radius)  # drawArcSoft (:889-915)
        if width == 1:
            pts = arc_ring_points(segments + 1, center, radius, arc.start, angle_step)
            for i in range(segments):
                self.draw_line(pts[i], pts[i + 1], color, 1, SOFT)
        else:
            pts = arc_ring_points(segments + 1, center, F(radius + F(line_width / _TWO)), arc.start, angle_step)
            pts += arc_ring_points(segments + 1, center, F(radius - F(line_width / _TWO)), arc.end, F(-angle_step))
            self.fill_polygon(pts, color, SOFT)

    def fill_arc(self, center, radius, start_angle, end_angle, color, mode):  # :1039-1059
        center, radius = (F(center[0]), F(center[1])), F(radius)
        start_angle, end_angle = F(start_angle), F(end_angle)
        if radius <= 0:
            return
        if not (np.isfinite(start_angle) and np.isfinite(end_angle)):
            return
        if abs(F(end_angle - start_angle)) >= TWO_PI:
            self.fill_circle(center, radius, color, mode)
            return
        arc = ArcRange(start_angle, end_angle)
        if mode == FAST:
            self._fill_arc_fast(center, radius, arc, color)
        else:
            self._fill_arc_soft(center, radius, arc, color)

    def _fill_arc_fast(self, center, radius, arc, color):  # :1088-1146
        if arc.span() <= 0:
            return
        solid = self._convert(color)
        frows, fcols = F(self.rows), F(self.cols)
        cx, cy = center
        cos_s, sin_s, cos_e, sin_e = cos(arc.start), sin(arc.start), cos(arc.end), sin(arc.end)
        cx_sin_s, cx_sin_e = F(cx * sin_s), F(cx * sin_e)
        top, bottom = max(_ZERO, F(cy - radius)), min(F(frows - _ONE), F(cy + radius))
        left, right = max(_ZERO, F(cx - radius)), min(F(fcols - _ONE), F(cx + radius))
        radius_sq = F(radius * radius)
        y = F(top)
        while y <= bottom:
            dy = F(y - cy)
            dx_max_sq = F(radius_sq - F(dy * dy))
            if dx_max_sq > 0:
                dx_max = np.sqrt(dx_max_sq)
                scan_left, scan_right = max(left, F(cx - dx_max)), min(right, F(cx + dx_max))
                start_const, end_const = F(F(-cx_sin_s) - F(dy * cos_s)), F(F(-cx_sin_e) - F(dy * cos_e))
                x = F(scan_left)
                while x <= scan_right:
                    if arc.contains_cross(F(F(x * sin_s) + start_const), F(F(x * sin_e) + end_const)):
                        span_end = x
                        while span_end < scan_right:
                            nx = F(span_end + _ONE)
                            dnx = F(nx - cx)
                            if F(F(dnx * dnx) + F(dy * dy)) > radius_sq:
                                break
                            if not arc.contains_cross(F(F(nx * sin_s) + start_const), F(F(nx * sin_e) + end_const)):
                                break
                            span_end = F(span_end + _ONE)
                        self.set_horizontal_span(x, span_end, y, solid)
                        x = span_end
                    x = F(x + _ONE)
            y = F(y + _ONE)

    def _fill_arc_soft(self, center, radius, arc, color):  # :1179-1218 with calculateArcCoverage (:1149-1176)
        bbox = self._ring_bbox(center, radius)
        if bbox is None:
            return
        l, t, r, b = bbox
        cx, cy = center
        cos_s, sin_s, cos_e, sin_e = cos(arc.start), sin(arc.start), cos(arc.end), sin(arc.end)
        for row in range(t, b):
            y = F(F(row) - cy)
            for col in range(l, r):
                x = F(F(col) - cx)
                dist_sq = F(F(x * x) + F(y * y))
                if dist_sq > F(F(radius + _ONE) * F(radius + _ONE)):
                    continue
                in_arc = arc.contains(atan2(y, x))
                start_cp, end_cp = F(F(x * sin_s) - F(y * cos_s)), F(F(x * sin_e) - F(y * cos_e))  # Point.cross
                start_cross, end_cross = abs(start_cp), abs(end_cp)
                if not in_arc:
                    near_start = start_cross < 1 and start_cp < _EPS
                    near_end = end_cross < 1 and end_cp > -_EPS
                    if not near_start and not near_end:
                        continue
                dist = np.sqrt(dist_sq)
                if dist <= F(radius - _ONE):
                    circ = _ONE
                elif dist < F(radius + _ONE):
                    circ = ref._clamp(F(F(radius - dist) + _HALF), 0, 1)
                else:
                    circ = _ZERO
                if not in_arc:
                    edge = _ZERO
                    if start_cross < 1 and start_cp < _EPS:
                        edge = max(edge, F(_ONE - start_cross))
                    if end_cross < 1 and end_cp > -_EPS:
                        edge = max(edge, F(_ONE - end_cross))
                    coverage = F(circ * edge)
                else:
                    coverage = circ
                    if start_cross < 1 and start_cp >= -_EPS:
                        coverage = min(coverage, start_cross)
                    if end_cross < 1 and end_cp <= _EPS:
                        coverage = min(coverage, end_cross)
                if coverage > 0:
                    self.set_pixel(row, col, ref.fade(color, coverage))


def run(image: np.ndarray, commands) -> np.ndarray:
    """canvas_curves_ref.run over the old kinds, the curves and the arcs: one reference call per command, in order, on a copy of `image`."""
    out = image.copy()
    cv = Canvas(out)
    for c in commands:
        kind = c["kind"]
        if kind not in ARC_KINDS:
            out[...] = cref.run(out, [c])
            continue
        mode, width, color = c.get("mode", FAST), c.get("width", 1), tuple(int(v) for v in c["color"])
        p, (start_angle, end_angle) = c["p"], c["pts"][0]
        for angle in (F(start_angle), F(end_angle)):  # the yardstick answers only where both lowerings of @mod give one answer
            assert not np.isfinite(angle) or normalize(angle, form=0) == normalize(angle, form=1), f"angle {angle!r} is not pinned"
        if kind == KIND_ARC:
            cv.draw_arc((p[0], p[1]), p[2], start_angle, end_angle, color, width, mode)
        else:
            cv.fill_arc((p[0], p[1]), p[2], start_angle, end_angle, color, mode)
    return out


# ---- the device's form of fillArcFast, restated so that the CPU suite can hold it to the literal loops
def walk_to(start, target: int):
    """The sequence v0 = start, v += 1 in f32 at its first value whose trunc reaches `target`, and the value before it (None: there is
    none), replayed a binade at a time as canvas_ref.disc_row_y does."""
    v, before = F(start), None
    while True:
        t = int(np.trunc(v))
        if t >= target:
            return v, before
        if v < _ONE:
            before, v = v, F(v + _ONE)
            continue
        p = F(2.0) ** F(math.floor(math.log2(float(v))) + 1)
        n = min(int(np.ceil(F(p - v))) - 1, target - t)
        if n > 0:
            before, v = F(v + F(n - 1)), F(v + F(n))
        else:
            before, v = v, F(v + _ONE)


def arc_fill_fast_gather(image: np.ndarray, center, radius, start_angle, end_angle, color) -> np.ndarray:
    """fillArc(.fast) of a partial arc, pixel by pixel: a pixel is stored when a value of its row's x sequence that belongs to a span lies
    in (col - 1, col + 1) (zignal_amd/csrc/canvas.hip: arc_fill_fast)."""
    out = image.copy()
    cv = Canvas(out)
    cx, cy, radius = F(center[0]), F(center[1]), F(radius)
    arc = ArcRange(F(start_angle), F(end_angle))
    if arc.span() <= 0:
        return out
    solid = cv._convert(tuple(color))
    frows, fcols = F(cv.rows), F(cv.cols)
    cos_s, sin_s, cos_e, sin_e = cos(arc.start), sin(arc.start), cos(arc.end), sin(arc.end)
    cx_sin_s, cx_sin_e = F(cx * sin_s), F(cx * sin_e)
    top, bottom = max(_ZERO, F(cy - radius)), min(F(frows - _ONE), F(cy + radius))
    left, right = max(_ZERO, F(cx - radius)), min(F(fcols - _ONE), F(cx + radius))
    radius_sq = F(radius * radius)
    for row in range(cv.rows):
        y, _ = walk_to(top, row)
        if not (y <= bottom and int(np.trunc(y)) == row):
            continue
        dy = F(y - cy)
        dx_max_sq = F(radius_sq - F(dy * dy))
        if dx_max_sq <= 0:
            continue
        dx_max = np.sqrt(dx_max_sq)
        scan_left, scan_right = max(left, F(cx - dx_max)), min(right, F(cx + dx_max))
        start_const, end_const = F(F(-cx_sin_s) - F(dy * cos_s)), F(F(-cx_sin_e) - F(dy * cos_e))

        def in_wedge(v):
            return arc.contains_cross(F(F(v * sin_s) + start_const), F(F(v * sin_e) + end_const))

        for col in range(cv.cols):
            v, before = walk_to(scan_left, col - 1)
            stored = False
            for _k in range(2):
                if F(col) - _ONE < v < F(col) + _ONE and in_wedge(v):
                    in_span = v <= scan_right
                    if not in_span and before is not None and before < scan_right:
                        dnx = F(v - cx)
                        in_span = (not F(F(dnx * dnx) + F(dy * dy)) > radius_sq) and in_wedge(before)
                    stored = stored or in_span
                before, v = v, F(v + _ONE)
            if stored:
                out[row, col] = solid
    return out


# ---- command builders (tests/canvas_cases.py's form)
OPAQUE, TRANSLUCENT = cref.OPAQUE, cref.TRANSLUCENT


def arc(center, radius, start_angle, end_angle, color=OPAQUE, width=1, mode=FAST):
    return {"kind": KIND_ARC, "mode": mode, "width": width, "color": color, "p": [center[0], center[1], radius],
            "pts": [(start_angle, end_angle)]}


def fill_arc(center, radius, start_angle, end_angle, color=OPAQUE, mode=FAST):
    return {"kind": KIND_FILL_ARC, "mode": mode, "width": 1, "color": color, "p": [center[0], center[1], radius],
            "pts": [(start_angle, end_angle)]}


def golden_cases():
    """(name, md5, command) of the recorded arc cases of the reference's regression list, and the fixture's header. The angles are stored
    as the f64 values of the reference's comptime expressions; they round to f32 where the call takes them."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for c in doc["cases"]:
        mode = {"fast": FAST, "soft": SOFT}[c["mode"]]
        if c["call"] == "arc":
            cmd = arc(c["center"], c["radius"], c["start"], c["end"], tuple(c["color"]), c["width"], mode)
        else:
            cmd = fill_arc(c["center"], c["radius"], c["start"], c["end"], tuple(c["color"]), mode)
        out.append((c["name"], c["md5"], cmd))
    return doc, out

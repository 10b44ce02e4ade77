"""Canvas(T) restated call by call (reference src/canvas/Canvas.zig): the reference's loops as written, sequential, in scalar np.float32
arithmetic, one call at a time. Deliberately not in the device's gather form: this is the yardstick tests/test_gpu_canvas.py holds
zg_canvas_draw to, byte for byte, and tests/test_canvas_oracle.py pins it to the reference's own MD5 sums
(src/canvas/tests/regression.zig, tests/golden/canvas_md5.json).

An image is a numpy u8 array: (rows, cols) for u8, (rows, cols, 3) for Rgb(u8), (rows, cols, 4) for Rgba(u8). Colours are Rgba(u8)
4-tuples, as the device interface takes them. Only an Rgba(u8) image is ever blended into: on u8 and Rgb(u8) the reference converts the
colour to the pixel type first, which drops the alpha, and stores it (see set_pixel). Modes: FAST = 0, SOFT = 1."""
from __future__ import annotations

import math

import numpy as np

F = np.float32
FAST, SOFT = 0, 1
KIND_LINE, KIND_RECT, KIND_FILL_RECT, KIND_CIRCLE, KIND_FILL_CIRCLE, KIND_POLYGON, KIND_FILL_POLYGON = range(7)
_HALF, _ONE, _ZERO = F(0.5), F(1.0), F(0.0)


def _round(x):  # @round: half away from zero (x - trunc(x) is exact)
    t = np.trunc(x)
    if abs(x - t) >= _HALF:
        t = t + (F(1.0) if x > 0 else F(-1.0))
    return F(t)


def _clamp(x, lo, hi):
    return F(max(F(lo), min(F(x), F(hi))))


def _to_u8(v):  # Rgba(f32).as(u8): round(255 * clamp(v, 0, 1))
    return int(_round(F(255.0) * _clamp(v, 0, 1)))


def blend_normal(base, overlay):
    """Rgba(u8).blend(overlay, .normal) (src/blending.zig:27-157)."""
    if overlay[3] == 0:
        return tuple(base)
    if base[3] == 0 or overlay[3] == 255:
        return tuple(overlay)
    b = [F(v) / F(255.0) for v in base]
    o = [F(v) / F(255.0) for v in overlay]
    result_a = F(o[3] + F(b[3] * F(_ONE - o[3])))
    if result_a <= 0:
        return (0, 0, 0, 0)
    base_weight = F(b[3] * F(_ONE - o[3]))
    inv = F(_ONE / result_a)
    out = [F(F(F(o[i] * o[3]) + F(b[i] * base_weight)) * inv) for i in range(3)]
    return (_to_u8(out[0]), _to_u8(out[1]), _to_u8(out[2]), _to_u8(result_a))


def fade(c, alpha):  # Rgba(u8).fade (src/color.zig:447-456)
    return (c[0], c[1], c[2], int(np.trunc(F(c[3]) * _clamp(alpha, 0, 1))))


def _gray(c):  # Rgb(u8) -> u8 luminance, BT.709 in 16.16 fixed point
    return min(255, (13933 * c[0] + 46871 * c[1] + 4732 * c[2] + 32768) >> 16)


class Canvas:
    def __init__(self, image: np.ndarray):
        assert image.dtype == np.uint8 and image.ndim in (2, 3)
        self.img = image
        self.rows, self.cols = image.shape[:2]
        self.ch = 1 if image.ndim == 2 else image.shape[2]

    # ---- convertColor / assignPixel (src/image.zig:67-94)
    def _convert(self, c):  # convertColor(T, Rgba)
        if self.ch == 1:
            return _gray(c)
        return tuple(c[: self.ch])

    def _store(self, r, c, v):
        self.img[r, c] = v

    def _as_rgba(self, r, c):  # an Rgba(u8) image's pixel
        return tuple(int(v) for v in self.img[r, c])

    def set_pixel(self, row, col, color):
        """setPixel with an Rgba colour (:504-514). It hands assignPixel convertColor(T, color): on an Rgba image that is still the Rgba
        colour and blends when a != 255; on u8 and Rgb the converted sample has no alpha left, assignPixel (image.zig:75) sees no Rgba sample
        and stores it, whatever the alpha was (a faded alpha of 0 included)."""
        if row >= self.rows or col >= self.cols:
            return
        if self.ch == 4 and color[3] != 255:
            self._store(row, col, blend_normal(self._as_rgba(row, col), color))
        else:
            self._store(row, col, self._convert(color))

    def set_point(self, x, y, color):  # :518-523
        row, col = math.floor(y), math.floor(x)
        if row < 0 or col < 0:
            return
        self.set_pixel(row, col, color)

    def _at_or_null_store(self, r, c, v):
        if 0 <= r < self.rows and 0 <= c < self.cols:
            self._store(r, c, v)

    def _clamp_rect(self, l, t, r, b):  # clampRectToImage (:62-79)
        left = int(np.trunc(_clamp(l, 0, F(self.cols))))
        top = int(np.trunc(_clamp(t, 0, F(self.rows))))
        right = int(np.trunc(_clamp(r, 0, F(self.cols))))
        bottom = int(np.trunc(_clamp(b, 0, F(self.rows))))
        if left >= right or top >= bottom:
            return None
        return left, top, right, bottom

    def set_horizontal_span(self, x1, x2, y, value):  # :129-145
        frows, fcols = F(self.rows), F(self.cols)
        if y < 0 or y >= frows:
            return
        if x2 < 0 or x1 >= fcols:
            return
        row = int(np.trunc(y))
        start = int(np.trunc(max(_ZERO, np.floor(x1))))
        end = int(np.trunc(min(F(fcols - _ONE), np.ceil(x2))))
        if start > end:
            return
        self.img[row, start:end + 1] = value

    # ---- lines (:152-496)
    def draw_line(self, p1, p2, color, width, mode):
        if width == 0:
            return
        p1 = (F(p1[0]), F(p1[1]))
        p2 = (F(p2[0]), F(p2[1]))
        if mode == FAST:
            if width == 1:
                self._line_bresenham(p1, p2, color)
            else:
                self._line_rectangle(p1, p2, width, color)
        elif width == 1:
            self._line_wu(p1, p2, color)
        else:
            self._line_distance(p1, p2, width, color)

    def _line_bresenham(self, p1, p2, color):
        x1, y1, x2, y2 = int(np.trunc(p1[0])), int(np.trunc(p1[1])), int(np.trunc(p2[0])), int(np.trunc(p2[1]))
        px = self._convert(color)
        if y1 == y2:
            self.set_horizontal_span(F(min(x1, x2)), F(max(x1, x2)), F(y1), px)
            return
        if x1 == x2:
            for y in range(min(y1, y2), max(y1, y2) + 1):
                self._at_or_null_store(y, x1, px)
            return
        dx, dy = abs(x2 - x1), abs(y2 - y1)
        sx = 1 if x1 < x2 else -1
        sy = 1 if y1 < y2 else -1
        err = dx - dy
        while True:
            self._at_or_null_store(y1, x1, px)
            if x1 == x2 and y1 == y2:
                break
            e2 = 2 * err
            if e2 > -dy:
                err -= dy
                x1 += sx
            if e2 < dx:
                err += dx
                y1 += sy

    @staticmethod
    def _fpart(x):
        return F(x - np.floor(x))

    @staticmethod
    def _rfpart(x):
        return F(_ONE - F(x - np.floor(x)))

    def _line_wu(self, p1, p2, c2):
        x1, y1, x2, y2 = p1[0], p1[1], p2[0], p2[1]
        if abs(F(y2 - y1)) < F(0.01):
            y = _round(y1)
            min_x, max_x = min(x1, x2), max(x1, x2)
            left_x, right_x = np.floor(min_x), np.ceil(max_x)
            if min_x > left_x:
                self.set_point(left_x, y, fade(c2, F(min_x - left_x)))
            solid_start, solid_end = np.ceil(min_x), np.floor(max_x)
            if solid_end >= solid_start:
                self.set_horizontal_span(solid_start, solid_end, y, self._convert(c2))
            if max_x < right_x:
                self.set_point(right_x, y, fade(c2, F(right_x - max_x)))
            return
        steep = abs(F(y2 - y1)) > abs(F(x2 - x1))
        if steep:
            x1, y1 = y1, x1
            x2, y2 = y2, x2
        if x1 > x2:
            x1, x2 = x2, x1
            y1, y2 = y2, y1
        dx, dy = F(x2 - x1), F(y2 - y1)
        gradient = _ONE if dx == 0 else F(dy / dx)
        x_px = [None, None]
        intery = None
        for idx, (ex, ey) in enumerate(((x1, y1), (x2, y2))):
            x_end = _round(ex)
            y_end = F(ey + F(gradient * F(x_end - ex)))
            x_gap = self._rfpart(F(ex + _HALF)) if idx == 0 else self._fpart(F(ex + _HALF))
            y_px = np.floor(y_end)
            a1, a2 = F(self._rfpart(y_end) * x_gap), F(self._fpart(y_end) * x_gap)
            if steep:
                self.set_point(y_px, x_end, fade(c2, a1))
                self.set_point(F(y_px + _ONE), x_end, fade(c2, a2))
            else:
                self.set_point(x_end, y_px, fade(c2, a1))
                self.set_point(x_end, F(y_px + _ONE), fade(c2, a2))
            x_px[idx] = x_end
            if idx == 0:
                intery = F(y_end + gradient)
        x = F(x_px[0] + _ONE)
        while x < x_px[1]:
            if steep:
                self.set_point(intery, x, fade(c2, self._rfpart(intery)))
                self.set_point(F(np.floor(intery) + _ONE), x, fade(c2, self._fpart(intery)))
            else:
                self.set_point(x, intery, fade(c2, self._rfpart(intery)))
                self.set_point(x, F(np.floor(intery) + _ONE), fade(c2, self._fpart(intery)))
            intery = F(intery + gradient)
            x = F(x + _ONE)

    def _line_rectangle(self, p1, p2, width, color):
        dx, dy = F(p2[0] - p1[0]), F(p2[1] - p1[1])
        length = np.sqrt(F(F(dx * dx) + F(dy * dy)))
        half_width = F(F(width) / F(2.0))
        if length == 0:
            self.fill_circle(p1, half_width, color, FAST)
            return
        perp_x = F(F(F(-dy) / length) * half_width)
        perp_y = F(F(dx / length) * half_width)
        corners = [(F(p1[0] - perp_x), F(p1[1] - perp_y)), (F(p1[0] + perp_x), F(p1[1] + perp_y)),
                   (F(p2[0] + perp_x), F(p2[1] + perp_y)), (F(p2[0] - perp_x), F(p2[1] - perp_y))]
        # fillPolygon gets convertColor(T, color): for a u8 or Rgb destination the colour it converts back is opaque either way in
        # .fast mode (only solid_color is used), so passing the Rgba colour is the same call
        self.fill_polygon(corners, color, FAST)
        self.fill_circle(p1, half_width, color, FAST)
        self.fill_circle(p2, half_width, color, FAST)

    def _line_distance(self, p1, p2, width, c2):
        half_width = F(F(width) / F(2.0))
        dx, dy = F(p2[0] - p1[0]), F(p2[1] - p1[1])
        length_sq = F(F(dx * dx) + F(dy * dy))
        if length_sq == 0:
            self.fill_circle(p1, half_width, c2, SOFT)
            return
        if dx == 0 or dy == 0:
            self._axis_aligned_thick_line(p1, p2, half_width, c2)
            return
        inv_length_sq = F(_ONE / length_sq)
        bbox = self._clamp_rect(F(min(p1[0], p2[0]) - half_width), F(min(p1[1], p2[1]) - half_width),
                                F(F(max(p1[0], p2[0]) + half_width) + _ONE), F(F(max(p1[1], p2[1]) + half_width) + _ONE))
        if bbox is None:
            return
        l, t, r, b = bbox
        for row in range(t, b):
            py = F(row)
            for col in range(l, r):
                px = F(col)
                dpx, dpy = F(px - p1[0]), F(py - p1[1])
                tt = _clamp(F(F(F(dpx * dx) + F(dpy * dy)) * inv_length_sq), 0, 1)
                dist_x, dist_y = F(dpx - F(tt * dx)), F(dpy - F(tt * dy))
                dist = np.sqrt(F(F(dist_x * dist_x) + F(dist_y * dist_y)))
                if dist > F(half_width + _HALF):
                    continue
                alpha = _ONE
                if dist > F(half_width - _HALF):
                    alpha = F(F(half_width + _HALF) - dist)
                if alpha > 0:
                    self.set_pixel(row, col, fade(c2, alpha))

    @staticmethod
    def _perpendicular_alpha(sample, center, half_width):
        dist = abs(F(sample - center))
        if dist > F(half_width + _HALF):
            return _ZERO
        if dist > F(half_width - _HALF):
            return F(F(half_width + _HALF) - dist)
        return _ONE

    def _axis_aligned_thick_line(self, p1, p2, half_width, c2):
        is_horizontal = p1[1] == p2[1]
        can_memset = c2[3] == 255
        if is_horizontal:
            rect = (min(p1[0], p2[0]), F(p1[1] - half_width), F(max(p1[0], p2[0]) + _ONE), F(F(p1[1] + half_width) + _ONE))
        else:
            rect = (F(p1[0] - half_width), min(p1[1], p2[1]), F(F(p1[0] + half_width) + _ONE), F(max(p1[1], p2[1]) + _ONE))
        bbox = self._clamp_rect(*rect)
        if bbox is not None:
            l, t, r, b = bbox
            center = p1[1] if is_horizontal else p1[0]
            if is_horizontal:
                for row in range(t, b):
                    alpha = self._perpendicular_alpha(F(row), center, half_width)
                    if alpha <= 0:
                        continue
                    if alpha >= 1.0 and can_memset:
                        self.set_horizontal_span(F(l), F(r - 1), F(row), self._convert(c2))
                    else:
                        faded = fade(c2, alpha)
                        for col in range(l, r):
                            self.set_pixel(row, col, faded)
            else:
                for col in range(l, r):
                    alpha = self._perpendicular_alpha(F(col), center, half_width)
                    if alpha <= 0:
                        continue
                    faded = fade(c2, alpha)
                    for row in range(t, b):
                        self.set_pixel(row, col, faded)
        self.fill_circle(p1, half_width, c2, SOFT)
        self.fill_circle(p2, half_width, c2, SOFT)

    # ---- polygons and rectangles (:579-632, :935-1017)
    def draw_polygon(self, points, color, width, mode):
        if width == 0:
            return
        n = len(points)
        for i in range(n):
            self.draw_line(points[i], points[(i + 1) % n], color, width, mode)

    def draw_rectangle(self, rect, color, width, mode):
        l, t, r, b = (F(v) for v in rect)
        self.draw_polygon([(l, t), (F(r - _ONE), t), (F(r - _ONE), F(b - _ONE)), (l, F(b - _ONE))], color, width, mode)

    def fill_rectangle(self, rect, color, mode):
        bounds = self._clamp_rect(*(F(v) for v in rect))
        if bounds is None:
            return
        l, t, r, b = bounds
        if mode == FAST:
            self.img[t:b, l:r] = self._convert(color)
        else:
            for row in range(t, b):
                for col in range(l, r):
                    self.set_pixel(row, col, color)

    def fill_polygon(self, points, color, mode):
        n = len(points)
        if n < 3:
            return
        pts = [(F(p[0]), F(p[1])) for p in points]
        frows, fcols = F(self.rows), F(self.cols)
        min_y = min(p[1] for p in pts)
        max_y = max(p[1] for p in pts)
        start_y = max(_ZERO, np.floor(min_y))
        end_y = min(F(frows - _ONE), np.ceil(max_y))
        solid = self._convert(color)
        y = F(start_y)
        while y <= end_y:
            xs = []
            for i in range(n):
                a, b = pts[i], pts[(i + 1) % n]
                if (a[1] <= y and b[1] > y) or (b[1] <= y and a[1] > y):
                    xs.append(F(a[0] + F(F(F(y - a[1]) * F(b[0] - a[0])) / F(b[1] - a[1]))))
            xs.sort()
            i = 0
            while i + 1 < len(xs):
                left_edge, right_edge = xs[i], xs[i + 1]
                if mode == SOFT:
                    x = F(max(_ZERO, np.floor(left_edge)))
                    x_end = min(F(fcols - _ONE), np.ceil(right_edge))
                    while x <= x_end:
                        alpha = _ONE
                        if x < F(left_edge + _ONE):
                            alpha = min(alpha, F(F(x + _HALF) - left_edge))
                        if x > F(right_edge - _ONE):
                            alpha = min(alpha, F(right_edge - F(x - _HALF)))
                        alpha = _clamp(alpha, 0, 1)
                        if alpha > 0:
                            self.set_point(x, y, fade(color, alpha))
                        x = F(x + _ONE)
                else:
                    self.set_horizontal_span(left_edge, right_edge, y, solid)
                i += 2
            y = F(y + _ONE)

    # ---- circles (:636-644, :752-876, :1021-1084)
    def draw_circle(self, center, radius, color, width, mode):
        radius = F(radius)
        center = (F(center[0]), F(center[1]))
        if radius <= 0 or width == 0:
            return
        if mode == FAST and width == 1:
            self._bresenham_circle(center, radius, color)
        else:
            lw = F(width)
            self._render_ring(center, F(radius - F(lw / F(2.0))), F(radius + F(lw / F(2.0))), color, mode)

    def fill_circle(self, center, radius, color, mode):
        radius = F(radius)
        center = (F(center[0]), F(center[1]))
        if radius <= 0:
            return
        if mode == SOFT:
            self._render_ring(center, _ZERO, radius, color, SOFT)
            return
        solid = self._convert(color)
        frows = F(self.rows)
        top = max(_ZERO, F(center[1] - radius))
        bottom = min(F(frows - _ONE), F(center[1] + radius))
        y = F(top)
        while y <= bottom:
            dy = F(y - center[1])
            dx = np.sqrt(max(_ZERO, F(F(radius * radius) - F(dy * dy))))
            if dx > 0:
                self.set_horizontal_span(F(center[0] - dx), F(center[0] + dx), y, solid)
            y = F(y + _ONE)

    def _ring_bbox(self, center, outer):
        frows, fcols = F(self.rows), F(self.cols)
        left = int(_round(_clamp(F(F(center[0] - outer) - _ONE), 0, fcols)))
        top = int(_round(_clamp(F(F(center[1] - outer) - _ONE), 0, frows)))
        right = int(_round(_clamp(F(F(center[0] + outer) + _ONE), 0, fcols)))
        bottom = int(_round(_clamp(F(F(center[1] + outer) + _ONE), 0, frows)))
        if left >= right or top >= bottom:
            return None
        return left, top, right, bottom

    @staticmethod
    def _ring_coverage(x, y, inner_r, outer_r, mode):
        dist_sq = F(F(x * x) + F(y * y))
        if mode == SOFT:
            dist = np.sqrt(dist_sq)
            if dist > F(outer_r + _HALF):
                return _ZERO
            if inner_r > 0 and dist < F(inner_r - _HALF):
                return _ZERO
            alpha = _ONE
            if dist > F(outer_r - _HALF):
                alpha = min(alpha, F(F(outer_r + _HALF) - dist))
            if inner_r > 0 and dist < F(inner_r + _HALF):
                alpha = min(alpha, F(dist - F(inner_r - _HALF)))
            return _clamp(alpha, 0, 1)
        inside_outer = dist_sq <= F(outer_r * outer_r)
        outside_inner = inner_r <= 0 or dist_sq >= F(inner_r * inner_r)
        return _ONE if (inside_outer and outside_inner) else _ZERO

    def _render_ring(self, center, inner, outer, color, mode):
        bbox = self._ring_bbox(center, outer)
        if bbox is None:
            return
        l, t, r, b = bbox
        solid = self._convert(color)
        for row in range(t, b):
            y = F(F(row) - center[1])
            for col in range(l, r):
                x = F(F(col) - center[0])
                coverage = self._ring_coverage(x, y, inner, outer, mode)
                if coverage <= 0:
                    continue
                if mode == SOFT:
                    self.set_pixel(row, col, fade(color, coverage))
                else:
                    self._store(row, col, solid)

    def _bresenham_circle(self, center, radius, color):
        cx, cy, r = _round(center[0]), _round(center[1]), _round(radius)
        x, y, err = F(r), _ZERO, _ZERO
        while x >= y:
            for ox, oy in ((x, y), (-x, y), (x, -y), (-x, -y), (y, x), (-y, x), (y, -x), (-y, -x)):
                self.set_point(F(cx + ox), F(cy + oy), color)
            if err <= 0:
                y = F(y + _ONE)
                err = F(err + F(F(F(2.0) * y) + _ONE))
            if err > 0:
                x = F(x - _ONE)
                err = F(err - F(F(F(2.0) * x) + _ONE))


def run(image: np.ndarray, commands) -> np.ndarray:
    """Execute a command list (tests/canvas_cases.py form) on a copy of `image`, one reference call per command, in order. A command is a
    dict: kind, mode, width, color, and p (the float parameters: x1 y1 x2 y2 | l t r b | cx cy radius) or pts (polygon vertices)."""
    out = image.copy()
    cv = Canvas(out)
    for c in commands:
        kind, mode, width, color = c["kind"], c.get("mode", FAST), c.get("width", 1), tuple(int(v) for v in c["color"])
        p = c.get("p")
        if kind == KIND_LINE:
            cv.draw_line((p[0], p[1]), (p[2], p[3]), color, width, mode)
        elif kind == KIND_RECT:
            cv.draw_rectangle(p[:4], color, width, mode)
        elif kind == KIND_FILL_RECT:
            cv.fill_rectangle(p[:4], color, mode)
        elif kind == KIND_CIRCLE:
            cv.draw_circle((p[0], p[1]), p[2], color, width, mode)
        elif kind == KIND_FILL_CIRCLE:
            cv.fill_circle((p[0], p[1]), p[2], color, mode)
        elif kind == KIND_POLYGON:
            cv.draw_polygon(c["pts"], color, width, mode)
        elif kind == KIND_FILL_POLYGON:
            cv.fill_polygon(c["pts"], color, mode)
        else:
            raise ValueError(kind)
    return out


# ---- closed forms the device uses in place of two sequential recurrences, restated so that the CPU suite can hold them to the literal walks
def bresenham_minor_offset(m: int, dmaj: int, dmin: int) -> int:
    """Minor-axis steps the general Bresenham line (:216-239) has taken once it has taken m major-axis steps; dmaj >= dmin >= 1."""
    return (2 * m * dmin + dmaj - 1) // (2 * dmaj)


def bresenham_line_pixels(x1, y1, x2, y2):
    """The pixels of the general case by the closed form, in walk order."""
    dx, dy = abs(x2 - x1), abs(y2 - y1)
    sx = 1 if x1 < x2 else -1
    sy = 1 if y1 < y2 else -1
    if dx >= dy:
        return [(x1 + sx * m, y1 + sy * bresenham_minor_offset(m, dx, dy)) for m in range(dx + 1)]
    return [(x1 + sx * bresenham_minor_offset(m, dy, dx), y1 + sy * m) for m in range(dy + 1)]


def bresenham_line_walk(x1, y1, x2, y2):
    """The literal walk of :216-239."""
    dx, dy = abs(x2 - x1), abs(y2 - y1)
    sx = 1 if x1 < x2 else -1
    sy = 1 if y1 < y2 else -1
    err = dx - dy
    out = []
    while True:
        out.append((x1, y1))
        if x1 == x2 and y1 == y2:
            return out
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x1 += sx
        if e2 < dx:
            err += dx
            y1 += sy


def disc_row_y(top, row: int):
    """fillCircleFast's y (:1073-1074, y = top; y += 1 in f32) when it reaches pixel row `row` (trunc(y) == row), or None when the walk
    steps over that row. Adding 1 is exact inside a binade; only the additions that cross a power of two round, so the walk is replayed
    one binade at a time."""
    y = F(top)
    while True:
        ty = int(np.trunc(y))
        if ty == row:
            return y
        if ty > row:
            return None
        if y < _ONE:
            y = F(y + _ONE)
            continue
        p = F(2.0) ** F(math.floor(math.log2(float(y))) + 1)  # the next power of two above y
        n_exact = int(np.ceil(F(p - y))) - 1                     # steps that stay below p (p - y is exact)
        n = min(n_exact, row - ty)
        if n > 0:
            y = F(y + F(n))
        else:
            y = F(y + _ONE)

"""Canvas(T).drawText restated line by line (reference src/canvas/Canvas.zig:1476-1658) with the BitmapFont lookups it calls
(src/font/BitmapFont.zig:61-170, :226-248), on top of tests/canvas_ref.py's Canvas (set_pixel, set_point, blend_normal, fade, which the
reference's own MD5 sums hold): sequential, scalar np.float32, one rounding per operation, the reference's expressions in the reference's
order. The yardstick of tests/test_gpu_canvas_text.py.

The three MD5 sums the reference records for drawText (src/canvas/tests/regression.zig:335-337) need its built-in 8 x 8 font, whose tables
are program text of the reference and are not restated anywhere in this project. So nothing pins this file to the reference but reading the
two side by side: drawText :1497-1541, renderGlyphUnscaled :1548-1582, renderGlyphFastScaled :1586-1605, renderGlyphSoftScaled :1609-1658,
getGlyphBit :1476-1482, calculateGlyphBytesPerRow :1486-1492; getCharData :67-92, getCharAdvanceWidth :118-139, getTextBounds :144-170,
getGlyphInfo :226-248.

A text is a str or a sequence of codepoints. A font is a Font: `glyphs is None` is the reference's fixed layout (glyph_map == null and
glyph_data == null), otherwise a list of Glyph, one per codepoint, stands for glyph_map + glyph_data.

One place has no defined result in the reference: renderGlyphFastScaled casts min(ceil(base + scale), clip) to u32, which is negative for
a bit whose block lies wholly left of or above the frame. Here such a bit writes nothing (under any other reading `x_start >= x_end`
would not `continue`), and UNDEFINED_CASTS counts how often it happened."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests import canvas_ref as ref
from tests.canvas_ref import F, FAST, SOFT

UNDEFINED_CASTS = 0
_ONE, _ZERO, _HALF = F(1.0), F(0.0), F(0.5)


@dataclass
class Glyph:  # GlyphData plus the map's key
    codepoint: int
    width: int
    height: int
    x_offset: int
    y_offset: int
    device_width: int
    bitmap_offset: int = 0


class Font:
    def __init__(self, char_width, char_height, first_char, last_char, data, glyphs=None):
        self.char_width, self.char_height, self.first_char, self.last_char = int(char_width), int(char_height), int(first_char), int(last_char)
        self.data = bytes(data)
        self.glyphs = None if glyphs is None else list(glyphs)
        self._map = None if glyphs is None else {g.codepoint: g for g in self.glyphs}  # glyph_map -> glyph_data[idx]

    def bytes_per_row(self):  # :61-63
        return (self.char_width + 7) // 8

    def get_char_data(self, cp):  # :67-92
        if self._map is None and cp <= 255 and self.first_char <= cp <= self.last_char:
            index = cp - self.first_char
            bytes_per_char = self.char_height * self.bytes_per_row()
            offset = index * bytes_per_char
            return self.data[offset:offset + bytes_per_char]
        if self._map is not None and cp in self._map:
            g = self._map[cp]
            size = g.height * ((g.width + 7) // 8)
            return self.data[g.bitmap_offset:g.bitmap_offset + size]
        return None

    def get_char_advance_width(self, cp):  # :118-139
        if self._map is None:
            return self.char_width
        if cp in self._map:
            g = self._map[cp]
            return g.device_width if g.device_width > 0 else 0
        return self.char_width

    def get_glyph_info(self, cp):  # :226-248
        if self._map is not None and cp in self._map:
            return self._map[cp]
        if cp <= 255 and self.first_char <= cp <= self.last_char:
            return Glyph(cp, self.char_width, self.char_height, 0, 0, self.char_width, 0)
        return None

    def get_text_bounds(self, text, scale):  # :144-170 -> (l, t, r, b)
        scale = F(scale)
        width, current_line_width, lines = _ZERO, _ZERO, _ONE
        char_height_scaled = F(F(self.char_height) * scale)
        for cp in codepoints(text):
            if cp == 10:
                width = max(width, current_line_width)
                current_line_width = _ZERO
                lines = F(lines + _ONE)
            else:
                current_line_width = F(current_line_width + F(F(self.get_char_advance_width(cp)) * scale))
        width = max(width, current_line_width)
        height = F(lines * char_height_scaled)
        return (_ZERO, _ZERO, F(width), height)


def codepoints(text):
    return [ord(ch) for ch in text] if isinstance(text, str) else [int(cp) for cp in text]


def get_glyph_bit(char_data, row, col, bytes_per_row):  # :1476-1482
    at = row * bytes_per_row + col // 8
    if at >= len(char_data):
        return 0
    return (char_data[at] >> (col % 8)) & 1


def glyph_bytes_per_row(glyph, font):  # :1486-1492
    return (glyph.width + 7) // 8 if font.glyphs is not None else font.bytes_per_row()


class Canvas(ref.Canvas):
    def draw_text(self, text, position, color, font, scale, mode):  # :1497-1541
        scale = F(scale)
        if scale <= 0:
            return
        color = tuple(int(v) for v in color)
        px, py = F(position[0]), F(position[1])
        tl, tt, tr, tb = font.get_text_bounds(text, scale)
        text_rect = (F(px + tl), F(py + tt), F(px + tr), F(py + tb))
        image_rect = (_ZERO, _ZERO, F(self.cols), F(self.rows))
        l, t = max(text_rect[0], image_rect[0]), max(text_rect[1], image_rect[1])  # Rectangle.intersect
        r, b = min(text_rect[2], image_rect[2]), min(text_rect[3], image_rect[3])
        if l >= r or t >= b:
            return
        clip_rect = (l, t, r, b)
        x, y = px, py
        start_x = x
        line_height = F(F(font.char_height) * scale)
        for cp in codepoints(text):
            if cp == 10:
                x = start_x
                y = F(y + line_height)
                continue
            glyph = font.get_glyph_info(cp)
            if glyph is not None:
                char_data = font.get_char_data(cp)
                if char_data is not None:
                    if scale == 1.0:
                        self._glyph_unscaled(glyph, char_data, font, x, y, color)
                    elif mode == FAST:
                        self._glyph_fast_scaled(glyph, char_data, font, x, y, scale, clip_rect, color)
                    else:
                        self._glyph_soft_scaled(glyph, char_data, font, x, y, scale, color)  # convertColor(Rgba, color) is the colour
            x = F(x + F(F(font.get_char_advance_width(cp)) * scale))

    def _glyph_unscaled(self, glyph, char_data, font, x, y, color):  # :1548-1582
        bytes_per_row = glyph_bytes_per_row(glyph, font)
        render_height = font.char_height if font.glyphs is None else glyph.height
        base_col = math.floor(x) + glyph.x_offset
        base_row = math.floor(y) + glyph.y_offset
        for row in range(render_height):
            py = base_row + row
            if py < 0 or py >= self.rows:
                continue
            for col in range(glyph.width):
                if get_glyph_bit(char_data, row, col, bytes_per_row) == 0:
                    continue
                px = base_col + col
                if px < 0 or px >= self.cols:
                    continue
                # dest.* = pixel, or assignPixel(dest, convertColor(T, color), .normal) when a != 255: set_pixel's rule
                self.set_pixel(py, px, color)

    def _glyph_fast_scaled(self, glyph, char_data, font, x, y, scale, clip_rect, color):  # :1586-1605
        global UNDEFINED_CASTS
        bytes_per_row = glyph_bytes_per_row(glyph, font)
        for row in range(glyph.height):
            for col in range(glyph.width):
                if get_glyph_bit(char_data, row, col, bytes_per_row) == 0:
                    continue
                base_x = F(x + F(F(F(col) + F(glyph.x_offset)) * scale))
                base_y = F(y + F(F(F(row) + F(glyph.y_offset)) * scale))
                x_start = int(np.trunc(max(np.floor(base_x), clip_rect[0])))
                y_start = int(np.trunc(max(np.floor(base_y), clip_rect[1])))
                x_end_f = min(np.ceil(F(base_x + scale)), clip_rect[2])
                y_end_f = min(np.ceil(F(base_y + scale)), clip_rect[3])
                if x_end_f <= -1 or y_end_f <= -1:  # @trunc of a negative float to u32: no defined result; the bit writes nothing
                    UNDEFINED_CASTS += 1
                    continue
                x_end, y_end = int(np.trunc(x_end_f)), int(np.trunc(y_end_f))
                if x_start >= x_end or y_start >= y_end:
                    continue
                for py in range(y_start, y_end):
                    for px in range(x_start, x_end):
                        self.set_point(F(px), F(py), color)

    def _glyph_soft_scaled(self, glyph, char_data, font, x, y, scale, rgba_color):  # :1609-1658
        bytes_per_row = glyph_bytes_per_row(glyph, font)
        glyph_width_f, glyph_height_f = F(glyph.width), F(glyph.height)
        dest_width = np.ceil(F(glyph_width_f * scale))
        dest_height = np.ceil(F(glyph_height_f * scale))
        sample_radius = F(_HALF / scale)
        dy = _ZERO
        while dy < dest_height:
            dx = _ZERO
            while dx < dest_width:
                dest_x = F(F(x + dx) + F(F(glyph.x_offset) * scale))
                dest_y = F(F(y + dy) + F(F(glyph.y_offset) * scale))
                ty, tx = int(np.trunc(dest_y)), int(np.trunc(dest_x))
                if not (ty < 0 or tx < 0 or ty >= self.rows or tx >= self.cols):  # atOrNull
                    src_x, src_y = F(dx / scale), F(dy / scale)
                    x0, x1 = F(src_x - sample_radius), F(src_x + sample_radius)
                    y0, y1 = F(src_y - sample_radius), F(src_y + sample_radius)
                    row_start_f, row_end_f = max(_ZERO, np.floor(y0)), min(F(glyph_height_f - _ONE), np.ceil(y1))
                    col_start_f, col_end_f = max(_ZERO, np.floor(x0)), min(F(glyph_width_f - _ONE), np.ceil(x1))
                    total_coverage = _ZERO
                    row_f = row_start_f
                    while row_f <= row_end_f:
                        col_f = col_start_f
                        while col_f <= col_end_f:
                            if get_glyph_bit(char_data, int(np.trunc(row_f)), int(np.trunc(col_f)), bytes_per_row) != 0:
                                overlap_x = ref._clamp(F(min(x1, F(col_f + _ONE)) - max(x0, col_f)), 0, 1)
                                overlap_y = ref._clamp(F(min(y1, F(row_f + _ONE)) - max(y0, row_f)), 0, 1)
                                total_coverage = F(total_coverage + F(overlap_x * overlap_y))
                            col_f = F(col_f + _ONE)
                        row_f = F(row_f + _ONE)
                    box_area = F(F(x1 - x0) * F(y1 - y0))
                    normalized_coverage = F(total_coverage / box_area)
                    if normalized_coverage > 0:
                        self.set_point(dest_x, dest_y, ref.fade(rgba_color, normalized_coverage))
                dx = F(dx + _ONE)
            dy = F(dy + _ONE)


def text(string, position, color, scale=1.0, mode=FAST):
    """One drawText call as a dict: text (str or codepoints), x, y, color, scale, mode."""
    return {"text": string, "x": float(position[0]), "y": float(position[1]), "color": tuple(color), "scale": float(scale), "mode": mode}


def run(image: np.ndarray, font: Font, commands) -> np.ndarray:
    """The reference making the calls of `commands` (text() dicts) one after another on a copy of `image`."""
    out = image.copy()
    cv = Canvas(out)
    for c in commands:
        cv.draw_text(c["text"], (c["x"], c["y"]), c["color"], font, c["scale"], c["mode"])
    return out

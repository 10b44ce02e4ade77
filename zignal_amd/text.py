"""BitmapFont and Canvas(T).drawText (reference src/font/BitmapFont.zig, src/canvas/Canvas.zig:1476-1658) over the text module's entry points
(include/zignal_hip_text.h). The font is the caller's: the library ships no glyph data.

    font = zg.BitmapFont.from_fixed(8, 8, 32, bitmaps)        # 8 x 8 glyphs for the codepoints from 32 on, one byte a row, bits LSB first
    zg.Canvas(image).draw_text("id 7", (12, 30), (255, 255, 0, 255), font, scale=2, mode="soft").flush()

The result equals the reference making the same drawText calls, byte for byte."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .image import Image, torch

# zg_text_cmd and zg_glyph as numpy structured dtypes: the bytes of the C structs
TEXT_CMD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("scale", "<f4"), ("mode", "<i4"), ("color", "u1", (4,)), ("first_codepoint", "<u4"),
                           ("n_codepoints", "<u4")])
GLYPH_DTYPE = np.dtype([("codepoint", "<u4"), ("bitmap_offset", "<u4"), ("width", "u1"), ("height", "u1"), ("x_offset", "<i2"), ("y_offset", "<i2"),
                        ("device_width", "<i2")])
assert TEXT_CMD_DTYPE.itemsize == C.sizeof(L.ZgTextCmd) and GLYPH_DTYPE.itemsize == C.sizeof(L.ZgGlyph)


def codepoints_of(text) -> np.ndarray:
    """A str decoded to its codepoints (the C interface takes codepoints, not UTF-8); a sequence of integers is taken as it is."""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("utf-8")
    if isinstance(text, str):
        return np.fromiter((ord(ch) for ch in text), np.uint32, len(text))
    return np.ascontiguousarray(text, np.uint32).reshape(-1)


class BitmapFont:
    """A bitmap font in one of the reference's two forms. It is checked when made (zg_font_check) and uploaded on first use, once per device."""

    def __init__(self, char_width, char_height, first_char, last_char, data, glyphs=None):
        self.char_width, self.char_height, self.first_char, self.last_char = int(char_width), int(char_height), int(first_char), int(last_char)
        self.data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).reshape(-1)
        self.glyphs = None if glyphs is None else np.ascontiguousarray(glyphs, GLYPH_DTYPE).reshape(-1)
        self._device = {}
        L.check(L.lib().zg_font_check(C.byref(self._host_font())))

    @classmethod
    def from_fixed(cls, char_width: int, char_height: int, first_char: int, data) -> "BitmapFont":
        """The fixed layout: glyph c is char_height rows of (char_width + 7) // 8 bytes at (c - first_char) times that, bits LSB first. The
        font ends with the last whole glyph of `data` (at codepoint 255 at the latest)."""
        raw = bytes(data) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8).tobytes()
        per_char = int(char_height) * ((int(char_width) + 7) // 8)
        count = len(raw) // per_char if per_char else 0
        if count < 1 or not 0 <= int(first_char) <= 255:
            raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, "BitmapFont.from_fixed: no whole glyph in data, or first_char outside 0..255")
        return cls(char_width, char_height, first_char, min(255, int(first_char) + count - 1), raw)

    @classmethod
    def from_glyphs(cls, char_height: int, glyphs, data, char_width=None) -> "BitmapFont":
        """The glyph table: `glyphs` is a GLYPH_DTYPE array or a sequence of dicts with its fields (bitmap_offset into `data`, rows of
        (width + 7) // 8 bytes); it is sorted by codepoint here. A line is char_height high; a codepoint the table lacks advances by
        char_width (default: the widest glyph)."""
        if not isinstance(glyphs, np.ndarray):
            table = np.zeros(len(glyphs), GLYPH_DTYPE)
            for i, g in enumerate(glyphs):
                for name in GLYPH_DTYPE.names:
                    table[i][name] = g[name]
            glyphs = table
        glyphs = np.sort(np.ascontiguousarray(glyphs, GLYPH_DTYPE), order="codepoint", kind="stable")
        if char_width is None:
            char_width = int(glyphs["width"].max()) if len(glyphs) else 0
        return cls(char_width, char_height, 0, 0, data, glyphs)

    def _font(self, data_ptr, glyphs_ptr) -> L.ZgFont:
        return L.ZgFont(data_ptr, glyphs_ptr, len(self.data), 0 if self.glyphs is None else len(self.glyphs), self.char_width, self.char_height,
                        self.first_char, self.last_char, 0)

    def _host_font(self) -> L.ZgFont:
        # a table font always has a table address, even when it is empty; a fixed font has none
        glyphs = None if self.glyphs is None else (self.glyphs.ctypes.data or 1)
        return self._font(self.data.ctypes.data if len(self.data) else None, glyphs)

    def _device_font(self, device) -> L.ZgFont:
        key = torch.device(device).index or 0
        if key not in self._device:
            out = L.ZgFont()
            with torch.cuda.device(key):
                L.check(L.lib().zg_font_upload(C.byref(self._host_font()), C.byref(out)))
            self._device[key] = out
        return self._device[key]

    def release(self) -> None:
        """Frees the device copies (they come back on the next use)."""
        fonts, self._device = self._device, {}
        for key, font in fonts.items():
            with torch.cuda.device(key):
                L.lib().zg_font_free(C.byref(font))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def text_bounds(self, text, scale: float = 1.0):
        """getTextBounds: (l, t, r, b) of the advance-width rectangle of `text` at `scale`, l = t = 0, r and b exclusive."""
        cps = codepoints_of(text)
        out = (C.c_float * 4)()
        L.check(L.lib().zg_text_bounds_host(C.byref(self._host_font()), cps.ctypes.data if len(cps) else None, len(cps), float(scale), out))
        return tuple(float(v) for v in out)


def pack_text(commands):
    """A list of text dicts — text (str or codepoints), x, y, scale, mode, color — as (a TEXT_CMD_DTYPE array, a uint32 codepoint array): the
    host form of zg_canvas_draw_text's two lists, the ranges tiling the array in list order."""
    from .canvas import _color, _mode

    cmds = np.zeros(len(commands), TEXT_CMD_DTYPE)
    parts, at = [], 0
    for i, c in enumerate(commands):
        cps = codepoints_of(c["text"])
        cmds[i]["x"], cmds[i]["y"], cmds[i]["scale"], cmds[i]["mode"] = float(c["x"]), float(c["y"]), float(c.get("scale", 1.0)), _mode(c.get("mode", L.DRAW_FAST))
        cmds[i]["color"] = _color(c["color"])
        cmds[i]["first_codepoint"], cmds[i]["n_codepoints"] = at, len(cps)
        parts.append(cps)
        at += len(cps)
    return cmds, (np.concatenate(parts) if parts else np.zeros(0, np.uint32)).astype(np.uint32)


def draw_text_host(image, font: BitmapFont, cmds: np.ndarray, codepoints) -> None:
    """zg_canvas_draw_text_host: host pixels, a TEXT_CMD_DTYPE array and uint32 codepoints. Synchronous; a command outside the contract raises."""
    img = image if isinstance(image, Image) else Image(image)
    cmds = np.ascontiguousarray(cmds, TEXT_CMD_DTYPE)
    cps = np.ascontiguousarray(codepoints, np.uint32).reshape(-1)
    d = img._desc()
    L.check(L.lib().zg_canvas_draw_text_host(C.byref(d), C.byref(font._host_font()), cmds.ctypes.data if len(cmds) else None, len(cmds),
                                             cps.ctypes.data if len(cps) else None, len(cps)))


def draw_text(image, font: BitmapFont, cmds, codepoints, count=None, n=None) -> None:
    """zg_canvas_draw_text, the device-list form: `cmds` a device tensor holding zg_text_cmd structs (n of them; by default as many as it
    holds), `codepoints` a device tensor of 32-bit codepoints, `count` an optional device tensor whose first 4 bytes are the number of
    commands to execute. Asynchronous on the current stream; nothing is synchronised, copied or uploaded once the font is on the device."""
    img = image if isinstance(image, Image) else Image(image)
    from .canvas import _device_lists

    n = _device_lists("draw_text", img, cmds, TEXT_CMD_DTYPE.itemsize, n, count, codepoints)
    if codepoints.element_size() != 4 or not codepoints.is_contiguous():
        raise ValueError("codepoints must be a contiguous tensor of 32-bit integers")
    ncp = codepoints.numel()
    dfont = font._device_font(img.data.device)
    d = img._desc()
    with torch.cuda.device(img.data.device):
        L.check(L.lib().zg_canvas_draw_text(C.byref(d), C.byref(dfont), C.c_void_p(cmds.data_ptr()), n, C.c_void_p(count.data_ptr()) if count is not None else None,
                                            C.c_void_p(codepoints.data_ptr()) if ncp else None, ncp, img._stream()))

"""The fonts of the drawText suites, made here: bitmaps from a seeded generator plus three hand-drawn glyphs (H, I, O as bars and a box,
drawn for whatever cell size the font has). Nothing comes from the reference. Each maker returns a tests.canvas_text_ref.Font;
device_font() turns one into the zg.BitmapFont with the same tables."""
from __future__ import annotations

import numpy as np

from tests import canvas_text_ref as TR

FIXED_SIZES = ((5, 7), (8, 8), (12, 13))  # one and two bytes a row


def _pack_rows(bits: np.ndarray) -> bytes:
    """(height, width) 0/1 -> rows of (width + 7) // 8 bytes, bits LSB first."""
    h, w = bits.shape
    out = np.zeros((h, (w + 7) // 8), np.uint8)
    for r in range(h):
        for c in range(w):
            if bits[r, c]:
                out[r, c // 8] |= 1 << (c % 8)
    return out.tobytes()


def hand_drawn(letter: str, w: int, h: int) -> np.ndarray:
    bits = np.zeros((h, w), np.uint8)
    if letter == "H":
        bits[:, 0] = bits[:, w - 1] = 1
        bits[h // 2, :] = 1
    elif letter == "I":
        bits[:, w // 2] = 1
        bits[0, 1:w - 1] = bits[h - 1, 1:w - 1] = 1
    elif letter == "O":
        bits[0, :] = bits[h - 1, :] = 1
        bits[:, 0] = bits[:, w - 1] = 1
    return bits


def glyph_bits(font: TR.Font, cp: int) -> np.ndarray:
    """The (height, width) bits of a glyph as the reference reads them."""
    g, data = font.get_glyph_info(cp), font.get_char_data(cp)
    bpr = TR.glyph_bytes_per_row(g, font)
    return np.array([[TR.get_glyph_bit(data, r, c, bpr) for c in range(g.width)] for r in range(g.height)], np.uint8).reshape(g.height, g.width)


def fixed_font(width: int, height: int, first_char: int = 32, count: int = 96, seed: int = 1) -> TR.Font:
    rng = np.random.default_rng(seed * 1000 + width * 16 + height)
    bpr = (width + 7) // 8
    data = bytearray(rng.integers(0, 256, count * height * bpr, dtype=np.uint8).tobytes())  # the bits past `width` of a row's last byte are noise too
    for letter in "HIO":
        at = (ord(letter) - first_char) * height * bpr
        data[at:at + height * bpr] = _pack_rows(hand_drawn(letter, width, height))
    data[0:height * bpr] = bytes(height * bpr)  # the space is blank
    return TR.Font(width, height, first_char, first_char + count - 1, bytes(data))


# codepoint, width, height, x_offset, y_offset, device_width
_TABLE = (
    (ord("H"), 7, 9, 0, 0, 8),
    (ord("I"), 5, 9, 1, 0, 7),
    (ord("O"), 9, 9, 0, 0, 10),       # two bytes a row
    (ord("j"), 6, 12, -2, 1, 5),      # reaches left of the pen and below the line
    (0xE9, 7, 11, 0, -3, 8),          # é: rises above the line
    (0x3A9, 11, 14, -1, -2, 12),      # Ω: taller than char_height (10)
    (0x2192, 10, 5, 0, 3, 0),         # →: advances by nothing
    (0x2190, 10, 5, -4, 3, -6),       # ←: a negative device_width advances by nothing as well
    (0x2003, 0, 9, 0, 0, 6),          # an em space: a glyph of no width
    (0x1F600, 13, 13, 1, -1, 15),     # past the basic plane
)
TABLE_CHAR_HEIGHT, TABLE_CHAR_WIDTH = 10, 9
TABLE_TEXT = "HIjéΩ→O← \U0001F600"


def table_font(seed: int = 7) -> TR.Font:
    rng = np.random.default_rng(seed)
    data, glyphs = bytearray(b"\xa5\x5a\xff"), []  # three bytes no glyph owns
    for cp, w, h, xo, yo, dw in _TABLE:
        bits = hand_drawn(chr(cp), w, h) if chr(cp) in "HIO" else (rng.random((h, w)) < 0.55).astype(np.uint8)
        glyphs.append(TR.Glyph(cp, w, h, xo, yo, dw, len(data)))
        data += _pack_rows(bits) if w else b""
    rng.shuffle(glyphs)  # the reference's map has no order; BitmapFont.from_glyphs sorts
    return TR.Font(TABLE_CHAR_WIDTH, TABLE_CHAR_HEIGHT, 0, 0, bytes(data), glyphs)


def glyph_table(font: TR.Font) -> np.ndarray:
    import zignal_amd as zg

    table = np.zeros(len(font.glyphs), zg.GLYPH_DTYPE)
    for i, g in enumerate(font.glyphs):
        table[i] = (g.codepoint, g.bitmap_offset, g.width, g.height, g.x_offset, g.y_offset, g.device_width)
    return table


def device_font(font: TR.Font):
    """The zg.BitmapFont with the same tables (host tables; it uploads itself on first use on a device)."""
    import zignal_amd as zg

    if font.glyphs is None:
        f = zg.BitmapFont.from_fixed(font.char_width, font.char_height, font.first_char, font.data)
        assert (f.first_char, f.last_char) == (font.first_char, font.last_char)
        return f
    return zg.BitmapFont.from_glyphs(font.char_height, glyph_table(font), font.data, char_width=font.char_width)

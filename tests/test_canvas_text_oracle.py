"""drawText without a device: properties of the restatement (tests/canvas_text_ref.py) that follow from the reference's code alone, the
library's host functions (zg_font_check, zg_text_bounds_host) against it, the declarations of the text module, and the host form's
argument errors, which answer before any device call."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import canvas_text_fonts as TF
from tests import canvas_text_ref as TR
from tests.canvas_ref import F, FAST, SOFT

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPAQUE, TRANSLUCENT = (200, 40, 90, 255), (30, 220, 120, 128)
FONTS = [TF.fixed_font(w, h) for w, h in TF.FIXED_SIZES]


def _blank(rows, cols, ch=4, value=7):
    return np.full((rows, cols, ch) if ch > 1 else (rows, cols), value, np.uint8)


def _layout(font, string, k=1):
    """Where the lit bits of `string` (one line, fixed font) fall with the pen at (0, 0) and every bit a k x k block."""
    lit = np.zeros((font.char_height * k, font.char_width * len(string) * k), bool)
    for i, ch in enumerate(string):
        bits = TF.glyph_bits(font, ord(ch)).astype(bool)
        lit[:, i * font.char_width * k:(i + 1) * font.char_width * k] = np.kron(bits, np.ones((k, k), bool))
    return lit


@pytest.mark.parametrize("font", FONTS, ids=lambda f: f"{f.char_width}x{f.char_height}")
def test_unscaled_opaque_text_lights_exactly_the_glyphs_bits_at_the_floor_of_the_position(font):
    string = "HIO~#"
    lit = _layout(font, string)
    for mode in (FAST, SOFT):  # scale == 1 takes the unscaled path in either mode
        for pos in ((3, 2), (3.75, 2.25), (-2.5, -1.5)):
            frame = _blank(font.char_height + 6, lit.shape[1] + 8)
            got = TR.run(frame, font, [TR.text(string, pos, OPAQUE, 1.0, mode)])
            want = frame.copy()
            ox, oy = int(np.floor(pos[0])), int(np.floor(pos[1]))
            for r, c in zip(*np.nonzero(lit)):
                if 0 <= r + oy < want.shape[0] and 0 <= c + ox < want.shape[1]:
                    want[r + oy, c + ox] = OPAQUE
            assert np.array_equal(got, want), (mode, pos)


@pytest.mark.parametrize("font", FONTS, ids=lambda f: f"{f.char_width}x{f.char_height}")
@pytest.mark.parametrize("k", (2, 3))
def test_fast_at_an_integer_scale_is_the_unscaled_image_with_each_bit_a_block(font, k):
    string = "HO%"
    lit = _layout(font, string, k)
    frame = _blank(lit.shape[0] + 5, lit.shape[1] + 5)
    got = TR.run(frame, font, [TR.text(string, (2, 3), OPAQUE, k, FAST)])
    want = frame.copy()
    want[3:3 + lit.shape[0], 2:2 + lit.shape[1]][lit] = OPAQUE
    assert np.array_equal(got, want)


@pytest.mark.parametrize("font", FONTS, ids=lambda f: f"{f.char_width}x{f.char_height}")
@pytest.mark.parametrize("k", (2, 4))
def test_soft_at_an_integer_scale_has_full_coverage_inside_a_lit_block(font, k):
    """The sample box of destination pixel d is centred on d / k and 1 / k wide: for the pixels 1 .. k - 1 of a bit's block it lies inside
    the bit, so a lit bit gives coverage 1 (k a power of two: exact), the colour unfaded; inside an unlit bit nothing is written."""
    string = "HI"
    frame = _blank(font.char_height * k + 4, font.char_width * k * len(string) + 4)
    got = TR.run(frame, font, [TR.text(string, (1, 2), OPAQUE, k, SOFT)])
    lit = _layout(font, string, 1)
    for r, c in np.ndindex(lit.shape):
        inner = got[2 + r * k + 1:2 + (r + 1) * k, 1 + c * k + 1:1 + (c + 1) * k]
        assert (inner == (OPAQUE if lit[r, c] else 7)).all(), (r, c)


def test_text_outside_the_frame_changes_nothing_in_any_path():
    font, table = FONTS[1], TF.table_font()
    for f, string in ((font, "HIO"), (table, TF.TABLE_TEXT)):
        for scale, mode in ((1.0, FAST), (2.0, FAST), (2.5, SOFT), (0.5, FAST), (0.5, SOFT)):
            for pos in ((-400, 5), (5, -300), (45, 5), (5, 60), (-0.0, 56), (40, 0)):
                for ch in (1, 3, 4):
                    frame = _blank(56, 40, ch)
                    assert np.array_equal(TR.run(frame, f, [TR.text(string, pos, TRANSLUCENT, scale, mode)]), frame), (scale, mode, pos, ch)
    frame = _blank(20, 20)
    assert np.array_equal(TR.run(frame, font, [TR.text("HIO", (2, 2), OPAQUE, 0.0, FAST), TR.text("HIO", (2, 2), OPAQUE, -2.0, SOFT), TR.text("", (2, 2), OPAQUE)]), frame)


def test_the_undefined_cast_is_counted_and_writes_nothing():
    """A .fast scaled text cut by the left and top edges: bits whose whole block lies at or beyond -1 would cast a negative float to u32."""
    font = FONTS[1]
    before = TR.UNDEFINED_CASTS
    got = TR.run(_blank(30, 30), font, [TR.text("OH", (-13.5, -7.25), OPAQUE, 3.0, FAST)])
    assert TR.UNDEFINED_CASTS > before
    assert (got != 7).any() and (got[:, 0] != 7).any() and (got[0, :] != 7).any()  # what is inside the frame is drawn, up to both edges


def test_the_table_font_follows_the_references_quirks():
    table = TF.table_font()
    assert table.get_glyph_info(0x41) is None and table.get_char_advance_width(0x41) == TF.TABLE_CHAR_WIDTH  # missing: nothing drawn, advances
    assert table.get_char_advance_width(0x2192) == 0 and table.get_char_advance_width(0x2190) == 0
    frame = _blank(30, 60)
    with_missing = TR.run(frame, table, [TR.text("HAO", (2, 5), OPAQUE)])
    want = TR.run(TR.run(frame, table, [TR.text("H", (2, 5), OPAQUE)]), table, [TR.text("O", (2 + 8 + 9, 5), OPAQUE)])
    assert np.array_equal(with_missing, want)
    # .fast scaled is clipped to the advance-width rectangle, the other two paths are not: j reaches left of the pen
    pos = (6, 4)
    unscaled = TR.run(frame, table, [TR.text("j", pos, OPAQUE, 1.0)])
    fast = TR.run(frame, table, [TR.text("j", pos, OPAQUE, 2.0, FAST)])
    soft = TR.run(frame, table, [TR.text("j", pos, OPAQUE, 2.0, SOFT)])
    assert (unscaled[:, :6] != 7).any() and (soft[:, :6] != 7).any() and not (fast[:, :6] != 7).any()
    assert (fast[:, 6:] != 7).any()


# ---- the library's host functions

def _cps(string):
    return np.array([ord(c) for c in string], np.uint32)


def test_text_bounds_host_equals_the_restatement():
    import zignal_amd as zg

    for f in FONTS + [TF.table_font()]:
        d = TF.device_font(f)
        for string in ("", "H", "HIO", "HI\nO\n", "\n\n", TF.TABLE_TEXT, "xx\n" + TF.TABLE_TEXT + "\nA", "→←"):
            for scale in (1.0, 2.0, 0.5, 2.75, 1.0 / 3.0, 63.9):
                want = tuple(float(v) for v in f.get_text_bounds(string, scale))
                assert d.text_bounds(string, scale) == want, (string, scale)
    assert zg.BitmapFont is not None


def test_font_check_accepts_the_suites_fonts_and_refuses_broken_tables():
    import zignal_amd as zg
    from zignal_amd import _lib as L

    for f in FONTS + [TF.table_font()]:
        TF.device_font(f)  # the constructor checks
    table = TF.table_font()
    good = np.sort(TF.glyph_table(table), order="codepoint")
    data = np.frombuffer(table.data, np.uint8)

    def check(glyphs, data=data, **kw):
        fields = dict(char_width=9, char_height=10, first_char=0, last_char=0, reserved=0)
        fields.update(kw)
        font = L.ZgFont(data.ctypes.data, None if glyphs is None else glyphs.ctypes.data, len(data), 0 if glyphs is None else len(glyphs), fields["char_width"],
                        fields["char_height"], fields["first_char"], fields["last_char"], fields["reserved"])
        return zg.lib().zg_font_check(C.byref(font))

    assert check(good) == L.OK
    assert check(good[::-1].copy()) == L.ERR_INVALID_ARGUMENT  # unsorted
    twice = good.copy()
    twice[3]["codepoint"] = twice[2]["codepoint"]
    assert check(twice) == L.ERR_INVALID_ARGUMENT  # a codepoint twice
    outside = good.copy()
    outside[-1]["bitmap_offset"] = len(data) - 3
    assert check(outside) == L.ERR_INVALID_ARGUMENT  # a bitmap that leaves the data
    far = good.copy()
    far[-1]["codepoint"] = 0x110000
    assert check(far) == L.ERR_INVALID_ARGUMENT
    assert check(good, reserved=1) == L.ERR_INVALID_ARGUMENT
    assert zg.lib().zg_font_check(None) == L.ERR_INVALID_ARGUMENT
    # fixed fonts: the data covers first_char .. last_char
    fixed = np.zeros(96 * 13 * 2, np.uint8)
    assert check(None, fixed, char_width=12, char_height=13, first_char=32, last_char=127) == L.OK
    assert check(None, fixed[:-1], char_width=12, char_height=13, first_char=32, last_char=127) == L.ERR_INVALID_ARGUMENT
    assert check(None, fixed, char_width=12, char_height=13, first_char=32, last_char=128) == L.ERR_INVALID_ARGUMENT
    assert check(None, fixed, char_width=12, char_height=13, first_char=40, last_char=39) == L.ERR_INVALID_ARGUMENT
    with pytest.raises(zg.InvalidArgument):
        zg.BitmapFont.from_glyphs(10, twice, table.data)


def test_module_header_bindings_and_struct_sizes():
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import text as T

    main = open(os.path.join(_ROOT, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_canvas.h"') < main.index('#include "zignal_hip_text.h"')
    header = open(os.path.join(_ROOT, "include", "zignal_hip_text.h")).read()
    declared = set(re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(", header))
    assert declared == set(L.TEXT_EXPORTED_SYMBOLS) == {"zg_sizeof_font", "zg_sizeof_glyph", "zg_sizeof_text_cmd", "zg_font_check", "zg_font_upload", "zg_font_free",
                                                        "zg_text_bounds_host", "zg_canvas_draw_text", "zg_canvas_draw_text_host"}
    lib = zg.lib()
    for name in L.TEXT_EXPORTED_SYMBOLS:
        assert getattr(lib, name) is not None
        assert len(getattr(lib, name).argtypes) == len(L._TEXT_SIGNATURES[name])
    assert lib.zg_sizeof_font() == C.sizeof(L.ZgFont) == 32
    assert lib.zg_sizeof_glyph() == C.sizeof(L.ZgGlyph) == T.GLYPH_DTYPE.itemsize == 16
    assert lib.zg_sizeof_text_cmd() == C.sizeof(L.ZgTextCmd) == T.TEXT_CMD_DTYPE.itemsize == 28
    define = lambda name: float(re.search(r"#define %s\s+([\d.]+)" % name, header).group(1))
    assert (define("ZG_TEXT_MAX_SCALE"), define("ZG_TEXT_MAX_CODEPOINTS"), define("ZG_TEXT_MAX_COMMANDS"), define("ZG_TEXT_MAX_TOTAL")) == (
        L.TEXT_MAX_SCALE, L.TEXT_MAX_CODEPOINTS, L.TEXT_MAX_COMMANDS, L.TEXT_MAX_TOTAL)
    # the existing command list has not moved: text is no kind
    assert lib.zg_sizeof_draw_cmd() == 40 and not hasattr(L, "DRAW_TEXT")
    canvas_header = open(os.path.join(_ROOT, "include", "zignal_hip_canvas.h")).read()
    assert "Kinds 7-15 are no kinds" in canvas_header and "zg_canvas_draw_text" not in canvas_header


def test_packing_decodes_utf8_and_tiles_the_codepoint_array():
    import zignal_amd as zg
    from zignal_amd import text as T

    font = TF.device_font(FONTS[1])
    cv = zg.Canvas(np.zeros((8, 8, 4), np.uint8))
    cv.draw_text("Hé→", (1.5, -2), (1, 2, 3), font, 2.5, "soft").draw_text("", (0, 0), (9, 9, 9, 9), font).draw_text("\U0001F600\n", (3, 4), (5, 6, 7, 8), font)
    cmds, cps = T.pack_text(cv.commands)
    assert list(cps) == [0x48, 0xE9, 0x2192, 0x1F600, 10] and cps.dtype == np.uint32
    assert list(cmds["first_codepoint"]) == [0, 3, 3] and list(cmds["n_codepoints"]) == [3, 0, 2]
    assert list(cmds["mode"]) == [1, 0, 0] and list(cmds["scale"]) == [2.5, 1.0, 1.0] and tuple(cmds[0]["color"]) == (1, 2, 3, 255)
    assert (cmds[0]["x"], cmds[0]["y"]) == (1.5, -2.0)
    assert list(T.codepoints_of("é".encode())) == [0xE9]
    with pytest.raises(zg.InvalidArgument):
        cv.draw_text("x", (0, 0), (1, 2, 3), font, mode="bold")


def test_host_form_argument_errors_come_before_any_device():
    """What the device form skips, the host form refuses, with the frame untouched; what passes goes on to the device, and only a machine
    without one then answers ZG_ERR_HIP."""
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import text as T

    font = TF.device_font(FONTS[1])
    frame = _blank(20, 30)
    nan, inf = float("nan"), float("inf")
    good = TR.text("HIO", (2, 3), OPAQUE, 2.0, SOFT)
    refused = [dict(good, mode=2), dict(good, mode=-1), dict(good, x=nan), dict(good, y=inf), dict(good, x=-65537.0), dict(good, y=65536.5), dict(good, scale=nan),
               dict(good, scale=inf), dict(good, scale=-inf), dict(good, scale=64.5), dict(good, text=[0x48, 0x110000])]
    for bad in refused:
        out = frame.copy()
        with pytest.raises(zg.InvalidArgument):
            T.draw_text_host(out, font, *T.pack_text([bad]))
        assert out.tobytes() == frame.tobytes(), bad
    cmds, cps = T.pack_text([good, good])
    for first, n, error in ((4, 3, zg.InvalidArgument), (7, 0, zg.InvalidArgument), (0xFFFFFFFF, 2, zg.InvalidArgument), (0, L.TEXT_MAX_CODEPOINTS + 1, zg.InvalidArgument)):
        broken = cmds.copy()
        broken[1]["first_codepoint"], broken[1]["n_codepoints"] = first, n
        with pytest.raises(error):
            T.draw_text_host(frame.copy(), font, broken, cps)
    many = np.zeros(L.TEXT_MAX_CODEPOINTS + 1, np.uint32) + 0x48
    one = cmds[:1].copy()
    one[0]["n_codepoints"] = len(many)
    with pytest.raises(zg.ZignalError) as e:
        T.draw_text_host(frame.copy(), font, one, many)
    assert e.value.status == L.ERR_UNSUPPORTED  # more codepoints in one command than the bound
    shared = cmds.copy()
    shared[1]["first_codepoint"] = 1  # the two ranges name 3 + 3 codepoints, the array holds 6: allowed, and they may overlap
    over = np.concatenate([cmds, cmds[:1]])  # 9 of 6
    with pytest.raises(zg.ZignalError) as e:
        T.draw_text_host(frame.copy(), font, over, cps)
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(zg.ZignalError) as e:
        T.draw_text_host(np.zeros((4, 4), np.float32), font, cmds, cps)
    assert e.value.status == L.ERR_UNSUPPORTED  # the pixel type
    d = zg.Image(frame.copy())._desc()
    assert zg.lib().zg_canvas_draw_text_host(C.byref(d), None, cmds.ctypes.data, 2, cps.ctypes.data, len(cps)) == L.ERR_INVALID_ARGUMENT
    assert zg.lib().zg_canvas_draw_text_host(C.byref(d), C.byref(font._host_font()), None, 2, cps.ctypes.data, len(cps)) == L.ERR_INVALID_ARGUMENT
    assert zg.lib().zg_canvas_draw_text_host(C.byref(d), C.byref(font._host_font()), cmds.ctypes.data, 2, None, len(cps)) == L.ERR_INVALID_ARGUMENT
    assert zg.lib().zg_canvas_draw_text_host(C.byref(d), C.byref(font._host_font()), cmds.ctypes.data, L.TEXT_MAX_COMMANDS + 1, cps.ctypes.data, len(cps)) == L.ERR_UNSUPPORTED
    passes = [good, dict(good, scale=0.0), dict(good, scale=-1.0), dict(good, x=-65536.0, y=65536.0), dict(good, text=""), dict(good, text="A世\n"), dict(good, scale=64.0)]
    for ok in passes + [None]:
        try:
            if ok is None:
                T.draw_text_host(frame.copy(), font, shared, cps)
            else:
                T.draw_text_host(frame.copy(), font, *T.pack_text([ok]))
        except zg.ZignalError as e:
            assert e.status == L.ERR_HIP, (ok, e)

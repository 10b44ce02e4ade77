"""drawText on the device — zg_canvas_draw_text and the host form — against tests/canvas_text_ref.py (the reference's calls made one after
another), byte for byte: the three paths on every pixel type at scales 1, 2, 3, 1.5, 2.75 and 0.5, opaque and translucent; fixed fonts of
one and two bytes a row and a glyph table with offsets, zero advances and a glyph of no width; positions between pixels, negative, cut by
each edge and outside; newlines, missing codepoints, empty texts; order and multiplicity on Rgba(u8); the chunk boundary, the count word,
the contract, a view, a captured graph and the Canvas class."""
import ctypes as C

import numpy as np
import pytest

import zignal_amd as zg
from tests import canvas_cases as K
from tests import canvas_curves_ref as CR
from tests import canvas_text_fonts as TF
from tests import canvas_text_ref as TR
from tests.test_gpu_canvas import PIXELS, T, background, same_bytes
from zignal_amd import _lib as L
from zignal_amd import canvas
from zignal_amd import text as ZT

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FAST, SOFT = TR.FAST, TR.SOFT
ROWS, COLS = 40, 56   # no multiple of the tile either way; a line of text crosses three tile columns
SMALL = (33, 17)
OPAQUE, TRANSLUCENT = (200, 60, 120, 255), (40, 180, 90, 128)
SCALES = (1.0, 2.0, 3.0, 1.5, 2.75, 0.5)
REF_FONTS = {"5x7": TF.fixed_font(5, 7), "8x8": TF.fixed_font(8, 8), "12x13": TF.fixed_font(12, 13), "table": TF.table_font()}
_DEVICE_FONTS = {}


def dfont(name):
    if name not in _DEVICE_FONTS:
        _DEVICE_FONTS[name] = TF.device_font(REF_FONTS[name])
    return _DEVICE_FONTS[name]


def string_of(name):
    return TF.TABLE_TEXT if name == "table" else "HI%O"


def on_device(host, name, commands, count=None, n=None, font=None):
    """zg_canvas_draw_text of `commands` (TR.text dicts) into a device copy of `host`; returns the frame."""
    cmds, cps = ZT.pack_text(commands)
    dcps = torch.from_numpy(cps.view(np.int32).copy()).cuda()
    return K.on_device(host, cmds, lambda dev, dcmds: ZT.draw_text(dev, font or dfont(name), dcmds, dcps, count=count, n=len(cmds) if n is None else n))


def on_host(host, name, commands):
    return K.on_host(host, ZT.draw_text_host, dfont(name), *ZT.pack_text(commands))


def check(host, name, commands, what, host_form=False):
    forms = [("zg_canvas_draw_text", lambda: on_device(host, name, commands))] + [("zg_canvas_draw_text_host", lambda: on_host(host, name, commands))] * host_form
    return K.check(TR.run(host, REF_FONTS[name], commands), what, *forms)


# ---- the three paths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", list(REF_FONTS))
@pytest.mark.parametrize("pixel", PIXELS)
def test_every_path_equals_the_reference(pixel, name, scale):
    host = background(ROWS, COLS, pixel, 3)
    string = string_of(name)
    for mode in (FAST, SOFT):
        for color in (OPAQUE, TRANSLUCENT):
            want = check(host, name, [TR.text(string, (3.25, 4.75), color, scale, mode)], (mode, color), host_form=mode == SOFT and color == TRANSLUCENT)
            assert not same_bytes(want, host)
    small = background(*SMALL, pixel, 4)
    check(small, name, [TR.text(string, (-2.5, 1.5), TRANSLUCENT, scale, SOFT), TR.text(string, (1, 17.25), TRANSLUCENT, scale, FAST)], "33 x 17")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["8x8", "table"])
@pytest.mark.parametrize("scale,mode", [(1.0, FAST), (2.75, FAST), (2.75, SOFT), (1.5, FAST), (0.5, SOFT), (0.5, FAST)])
def test_positions_between_pixels_negative_cut_by_each_edge_and_outside(name, scale, mode):
    host = background(ROWS, COLS, "rgba_u8", 5)
    string = string_of(name)
    before = TR.UNDEFINED_CASTS
    for pos in ((-5.5, 3.0), (3.0, -1.75), (COLS - 6.5, 3.0), (3.0, ROWS - 5.0), (-0.5, -0.5), (-0.999, 12.001), (COLS - 1.0, ROWS - 1.0)):
        want = check(host, name, [TR.text(string, pos, TRANSLUCENT, scale, mode)], pos)
        assert pos[0] == COLS - 1.0 or not same_bytes(want, host), pos
    for pos in ((-300.0, 5.0), (5.0, 400.0), (float(COLS), 2.0), (2.0, float(ROWS)), (5.0, -200.0), (-65536.0, 65536.0)):
        assert same_bytes(check(host, name, [TR.text(string, pos, TRANSLUCENT, scale, mode)], pos, host_form=pos[0] == 5.0), host), pos
    if scale > 1 and mode == FAST:  # the cast the reference leaves undefined was met at the left and top edges, and the bytes still agree
        assert TR.UNDEFINED_CASTS > before


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["5x7", "12x13", "table"])
def test_newlines_missing_codepoints_and_empty_texts(name):
    host = background(ROWS, COLS, "rgba_u8", 6)
    strings = ("HI\nO", "H\x01O世I", "", "\n", "\n\nHO", "A\n\nH\n")
    for scale, mode in ((1.0, SOFT), (2.0, FAST), (1.5, SOFT)):
        for s in strings:
            check(host, name, [TR.text(s, (2.5, 1.25), TRANSLUCENT, scale, mode)], (s, scale, mode), host_form=scale == 1.5)
        check(host, name, [TR.text(s, (1.0 + 3 * i, 2.0 * i), OPAQUE if i % 2 else TRANSLUCENT, scale, mode) for i, s in enumerate(strings)], "all")
    # scale <= 0 draws nothing and is inside the contract
    assert same_bytes(check(host, name, [TR.text("HIO", (2, 2), OPAQUE, 0.0, FAST), TR.text("HIO", (2, 2), OPAQUE, -3.0, SOFT)], "scale <= 0", host_form=True), host)


# ---- order and multiplicity -------------------------------------------------------------------------------------------------------------------
class _Counting(TR.Canvas):
    def set_pixel(self, row, col, color):
        if row < self.rows and col < self.cols:
            self.writes[row, col] += 1
        super().set_pixel(row, col, color)


def most_writes(host, font, command):
    cv = _Counting(host.copy())
    cv.writes = np.zeros(host.shape[:2], int)
    cv.draw_text(command["text"], (command["x"], command["y"]), command["color"], font, command["scale"], command["mode"])
    return int(cv.writes.max())


@pytest.mark.gpu
def test_overlapping_glyphs_and_overlapping_blocks_blend_as_often_as_the_reference_writes():
    host = background(ROWS, COLS, "rgba_u8", 7)
    # at a fractional scale the blocks of neighbouring bits share pixels: one glyph writes a pixel two or four times
    for scale in (1.5, 2.75, 1.25):
        command = TR.text("OH#%", (2.25, 3.5), TRANSLUCENT, scale, FAST)
        assert most_writes(host, REF_FONTS["8x8"], command) >= 2
        check(host, "8x8", [command], scale)
    # glyphs that advance by nothing or reach left of the pen lie over their neighbours
    for scale, mode in ((1.0, FAST), (2.0, FAST), (2.0, SOFT), (1.5, FAST), (1.5, SOFT)):
        command = TR.text("O→←j\U0001F600Ω", (4.5, 6.25), TRANSLUCENT, scale, mode)
        assert most_writes(host, REF_FONTS["table"], command) >= 2
        check(host, "table", [command], (scale, mode))


@pytest.mark.gpu
def test_two_overlapping_commands_in_both_orders():
    host = background(ROWS, COLS, "rgba_u8", 8)
    a = TR.text("HOH", (3.0, 5.0), (250, 20, 20, 128), 2.0, SOFT)
    b = TR.text("OIO", (6.5, 8.5), (20, 20, 250, 128), 1.5, FAST)
    ab, ba = check(host, "8x8", [a, b], "a b", host_form=True), check(host, "8x8", [b, a], "b a", host_form=True)
    assert not same_bytes(ab, ba)


@pytest.mark.gpu
def test_a_list_longer_than_one_compaction_chunk():
    """The tile kernel takes 1024 glyphs at a time: the two soft commands sit on the boundary, one glyph list entry either side of it."""
    host = background(ROWS, COLS, "rgba_u8", 9)
    rng = np.random.default_rng(11)
    commands = []
    for i in range(93):  # 93 x 11 = 1023 codepoints
        color = tuple(int(v) for v in rng.integers(0, 256, 3)) + (128,)
        commands.append(TR.text("HIO%#HIO&@H", (float(rng.integers(-6, COLS - 20)), float(rng.integers(-3, ROWS - 3))), color, 1.0, FAST))
    commands.append(TR.text("OH", (8.5, 9.25), (250, 10, 10, 128), 2.5, SOFT))   # entries 1023 and 1024
    commands.append(TR.text("HIO", (12.0, 14.5), (10, 10, 250, 128), 1.5, FAST))
    for i in range(6):
        commands.append(TR.text("I#O", (5.0 + 7 * i, 20.0 + i), (9, 200, 30, 128), 1.0, FAST))
    want = check(host, "8x8", commands, "1046 glyphs")
    assert not same_bytes(want, TR.run(host, REF_FONTS["8x8"], commands[:93] + commands[94:]))


@pytest.mark.gpu
def test_order_sensitive_glyphs_on_the_wave_slice_and_chunk_seams_of_the_gather():
    """One codepoint a command, so that a glyph's place in the entry list is its command's: pairs of overlapping translucent glyphs lie
    with one entry on either side of a seam of the gather (between two waves, two slices of 256, two chunks of 1024); every other glyph
    lies off the frame, has an empty box and must not hit. 17 x 17: two tiles each way, and each pair covers pixels of both tile columns."""
    host = background(T + 1, T + 1, "rgba_u8", 15)
    commands = [TR.text("HIO%#&@"[i % 7], (-60.0 - i % 9, -40.0 - i % 4), (i % 256, 90, 200, 128), 1.0, FAST) for i in range(1030)]
    for k, at in enumerate((63, 255, 767, 1023)):  # pair k from row 3 k on: the last one reaches the second tile row
        commands[at] = TR.text("#", (9.0, 3.0 * k), (250, 10 + 60 * k, 10, 128), 1.0, FAST)
        commands[at + 1] = TR.text("%", (10.0, 3.0 * k + 1), (10, 10 + 60 * k, 250, 128), 1.0, FAST)
    want = check(host, "8x8", commands, "1030 glyphs, pairs on the seams")
    assert (want != host).any(axis=2)[:, :T].any() and (want != host).any(axis=2)[:, T:].any()
    for at in (63, 255, 767, 1023):
        swapped = list(commands)
        swapped[at], swapped[at + 1] = commands[at + 1], commands[at]
        assert not same_bytes(want, TR.run(host, REF_FONTS["8x8"], swapped)), at


# ---- the device call ------------------------------------------------------------------------------------------------------------------------
def mixed_list():
    return [TR.text("HO", (2.0, 3.0), TRANSLUCENT, 2.0, SOFT), TR.text("I%", (10.5, 6.0), OPAQUE, 1.0, FAST), TR.text("OH", (4.0, 12.5), TRANSLUCENT, 1.5, FAST),
            TR.text("H\nI", (20.0, 2.0), TRANSLUCENT, 2.75, SOFT), TR.text("#", (30.0, 20.0), OPAQUE, 3.0, FAST)]


@pytest.mark.gpu
def test_count_word_shorter_than_the_list_draws_the_prefix():
    host = background(ROWS, COLS, "rgba_u8", 10)
    commands = mixed_list()
    word = lambda v: torch.tensor([v, 12345], dtype=torch.int32, device="cuda")
    assert same_bytes(on_device(host, "8x8", commands, word(0)), host)
    assert same_bytes(on_device(host, "8x8", commands, word(3)), TR.run(host, REF_FONTS["8x8"], commands[:3]))
    assert same_bytes(on_device(host, "8x8", commands, word(99)), TR.run(host, REF_FONTS["8x8"], commands))


@pytest.mark.gpu
def test_commands_outside_the_contract_are_skipped_with_their_neighbours_drawn_and_refused_by_the_host_form():
    host = background(ROWS, COLS, "rgb_u8", 11)
    good = [TR.text("HO", (2.0, 3.0), TRANSLUCENT, 2.0, SOFT), TR.text("OI", (6.0, 9.5), OPAQUE, 1.5, FAST)]
    want = TR.run(host, REF_FONTS["8x8"], good)
    nan, inf = float("nan"), float("inf")
    t = TR.text("HIO", (4.0, 4.0), OPAQUE, 2.0, FAST)
    bad = [dict(t, mode=2), dict(t, x=nan), dict(t, y=-inf), dict(t, x=65537.0), dict(t, y=-1e9), dict(t, scale=nan), dict(t, scale=inf), dict(t, scale=64.25),
           dict(t, text=[0x48, 0x110000, 0x49]), dict(t, text=[0xFFFFFFFF])]
    for b in bad:
        assert same_bytes(on_device(host, "8x8", [good[0], b, good[1]]), want), b
        out = host.copy()
        with pytest.raises(zg.InvalidArgument):
            ZT.draw_text_host(out, dfont("8x8"), *ZT.pack_text([good[0], b, good[1]]))
        assert same_bytes(out, host)

    def with_range(first, n):
        cmds, cps = ZT.pack_text([good[0], t, good[1]])
        cmds[1]["first_codepoint"], cmds[1]["n_codepoints"] = first, n
        dev = torch.from_numpy(host.copy()).cuda()
        ZT.draw_text(dev, dfont("8x8"), torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), torch.from_numpy(cps.view(np.int32).copy()).cuda())
        return dev.cpu().numpy()

    for first, n in ((6, 2), (8, 0), (0xFFFFFFFF, 3), (2, 0xFFFFFFFF)):  # a range outside the 7 codepoints
        assert same_bytes(with_range(first, n), want), (first, n)
    # ranges may overlap and repeat while the running total stays inside the array: here the middle command draws the first one's "HO" again
    again = TR.run(host, REF_FONTS["8x8"], [good[0], dict(t, text="HO"), good[1]])
    assert same_bytes(with_range(0, 2), again)
    # ... and from the command on at which the total passes the array's length, the device skips: 2 + 5 fit, the last 2 do not
    assert same_bytes(with_range(0, 5), TR.run(host, REF_FONTS["8x8"], [good[0], dict(t, text="HOHIO")]))
    assert same_bytes(with_range(0, 6), TR.run(host, REF_FONTS["8x8"], [good[0]]))
    # a glyph whose bitmap leaves data_len is skipped, and still advances: the font with its data cut off behind 'H'
    font = dfont("8x8")
    cut = L.ZgFont.from_buffer_copy(font._device_font("cuda"))
    cut.data_len = (ord("H") - 32 + 1) * 8
    shorter = TF.fixed_font(8, 8)
    shorter.last_char = ord("H")
    command = [TR.text("HIOH", (3.0, 4.0), TRANSLUCENT, 2.0, SOFT)]
    assert same_bytes(on_device(host, "8x8", command, font=_Borrowed(cut)), TR.run(host, shorter, command))


class _Borrowed:
    """A zg_font struct standing in for a BitmapFont in draw_text."""

    def __init__(self, font):
        self.font = font

    def _device_font(self, device):
        return self.font


@pytest.mark.gpu
def test_views_of_a_wider_tensor_leave_their_surroundings_alone():
    rows, cols = T + 3, 2 * T + 1
    commands = [TR.text("HO\nI#", (-3.5, -2.25), TRANSLUCENT, 2.75, SOFT), TR.text("OIH", (1.0, 2.0), OPAQUE, 1.0, FAST), TR.text("HIO", (6.5, 4.0), TRANSLUCENT, 1.5, FAST)]
    cmds, cps = ZT.pack_text(commands)
    dcmds, dcps = torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), torch.from_numpy(cps.view(np.int32).copy()).cuda()
    for pixel in PIXELS:
        inner = background(rows, cols, pixel, 5)
        wide = np.full((rows + 6, cols + 11) + inner.shape[2:], 0xA5, np.uint8)
        wide[2:2 + rows, 4:4 + cols] = inner
        dev = torch.from_numpy(wide).cuda()
        ZT.draw_text(dev[2:2 + rows, 4:4 + cols], dfont("12x13"), dcmds, dcps)
        expect = wide.copy()
        expect[2:2 + rows, 4:4 + cols] = TR.run(inner, REF_FONTS["12x13"], commands)
        assert same_bytes(dev.cpu().numpy(), expect), pixel


# ---- the Canvas class ------------------------------------------------------------------------------------------------------------------------
def flush_reference(host):
    out = CR.run(host, [K.fill_rect(4.0, 3.0, 44.0, 30.0, (20, 30, 200, 160), SOFT)])
    out = TR.run(out, REF_FONTS["8x8"], [TR.text("HI O", (6.5, 5.0), TRANSLUCENT, 2.0, SOFT)])
    out = CR.run(out, [K.line(2.0, 8.0, 50.0, 24.0, (250, 250, 10, 128), 3, SOFT)])
    out = TR.run(out, REF_FONTS["8x8"], [TR.text("OH", (8.0, 14.5), (250, 20, 20, 128), 1.5, FAST)])
    return TR.run(out, REF_FONTS["table"], [TR.text("Ωj", (30.0, 20.0), OPAQUE, 1.0, FAST)])


@pytest.mark.gpu
def test_flush_issues_runs_of_text_and_of_everything_else_in_list_order():
    host = background(ROWS, COLS, "rgba_u8", 12)
    want = flush_reference(host)
    for image in (torch.from_numpy(host.copy()).cuda(), host.copy()):
        cv = zg.Canvas(image)
        cv.fill_rectangle((4.0, 3.0, 44.0, 30.0), (20, 30, 200, 160), "soft").draw_text("HI O", (6.5, 5.0), TRANSLUCENT, dfont("8x8"), 2.0, "soft")
        cv.draw_line((2.0, 8.0), (50.0, 24.0), (250, 250, 10, 128), 3, "soft").draw_text("OH", (8.0, 14.5), (250, 20, 20, 128), dfont("8x8"), 1.5, "fast")
        cv.draw_text("Ωj", (30.0, 20.0), OPAQUE, dfont("table"))  # another font: a call of its own
        cv.flush()
        assert cv.commands == []
        got = zg.Image(image).to_numpy()
        if not same_bytes(got, want):
            raise K.differs(got, want, "rectangle, text, line, text, text", type(image).__name__)
    # a list order that matters: the line over the first text, under the second
    assert not same_bytes(want, TR.run(CR.run(host, [K.fill_rect(4.0, 3.0, 44.0, 30.0, (20, 30, 200, 160), SOFT), K.line(2.0, 8.0, 50.0, 24.0, (250, 250, 10, 128), 3, SOFT)]),
                                       REF_FONTS["8x8"], [TR.text("HI O", (6.5, 5.0), TRANSLUCENT, 2.0, SOFT), TR.text("OH", (8.0, 14.5), (250, 20, 20, 128), 1.5, FAST)]))


@pytest.mark.gpu
def test_a_flush_without_text_draws_todays_bytes():
    host = background(ROWS, COLS, "rgba_u8", 13)
    commands = K.every_kind(2, SOFT, K.TRANSLUCENT, ROWS, COLS)
    cmds, vertices = canvas.pack_commands(commands)
    direct = torch.from_numpy(host.copy()).cuda()
    canvas.draw(direct, torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), vertices=torch.from_numpy(vertices).cuda() if len(vertices) else None)
    image = torch.from_numpy(host.copy()).cuda()
    cv = zg.Canvas(image)
    cv.commands = [dict(c) for c in commands]
    cv.flush()
    assert same_bytes(image.cpu().numpy(), direct.cpu().numpy()) and same_bytes(image.cpu().numpy(), CR.run(host, commands))


# ---- a captured graph -------------------------------------------------------------------------------------------------------------------------
def graph_list(seed):
    rng = np.random.default_rng(seed)
    letters = "HIO%#&@ \n"
    out = []
    for k in range(8):
        s = "".join(letters[int(i)] for i in rng.integers(0, len(letters), 5))
        pos = (float(np.float32(rng.uniform(-6, COLS - 8))), float(np.float32(rng.uniform(-6, ROWS - 4))))
        color = tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.choice([255, 128])),)
        out.append(TR.text(s, pos, color, (1.0, 2.0, 1.5, 2.75)[k % 4], (FAST, SOFT)[(k // 2) % 2]))
    return out


def graph_replay():
    """Captures zg_canvas_draw_text as the first drawing call the process makes (the font is uploaded before: an upload is no part of a
    graph), then replays the graph on other codepoints, positions, frames and counts."""
    lists = [graph_list(seed) for seed in (501, 502, 503)]
    n = len(lists[0])
    font = dfont("8x8")
    font._device_font("cuda")
    frame = torch.zeros((ROWS, COLS, 4), dtype=torch.uint8, device="cuda")
    dcmds = torch.zeros(n * 28, dtype=torch.uint8, device="cuda")
    dcps = torch.zeros(5 * n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")

    def load(k, how_many):
        host = background(ROWS, COLS, "rgba_u8", 20 + k)
        cmds, cps = ZT.pack_text(lists[k])
        frame.copy_(torch.from_numpy(host))
        dcmds.copy_(torch.from_numpy(cmds.view(np.uint8).copy()))
        dcps.copy_(torch.from_numpy(cps.view(np.int32).copy()))
        count.fill_(how_many)
        return TR.run(host, REF_FONTS["8x8"], lists[k][:how_many])

    K.replay_captured(frame, lambda: ZT.draw_text(frame, font, dcmds, dcps, count=count), load, ((0, n), (1, n), (2, 5)))


@pytest.mark.gpu
def test_draw_text_is_captured_as_a_fresh_process_first_drawing_call_and_replays_on_changed_lists():
    K.graph_replay_in_a_fresh_process("test_gpu_canvas_text")

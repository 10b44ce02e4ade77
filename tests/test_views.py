"""The canvas helper of the destination-view tests (tests/views.py) on CPU tensors: an untouched canvas passes, and one stray byte in any
of the four margins or in the gap between cols and stride is named with its place."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import views as V

KINDS = tuple(V.LAYOUT)


def canvas(kind):
    return V.Canvas(kind, 7, 9, 17, 3, 18, 2, extra_stride_px=5, device="cpu")


@pytest.mark.parametrize("kind", KINDS)
def test_an_untouched_canvas_passes_and_returns_what_was_put(kind):
    c = canvas(kind)
    dtype, ch = V.LAYOUT[kind]
    host = (np.arange(7 * 9 * ch) % 251).reshape((7, 9) + ((ch,) if ch > 1 else ())).astype(np.uint8 if dtype == torch.uint8 else np.float32)
    c.put(host)
    got = c.take("untouched")
    assert got.dtype == host.dtype and np.array_equal(got, host)
    assert c.stray() is None
    f = c.facts()
    assert f["rows%2"] == 1 and f["cols%4"] == 1 and f["row_bytes%16"] == 9 * V.psize(kind) % 16
    assert f["stride_bytes%16"] == (17 + 9 + 18 + 5) * V.psize(kind) % 16


# (row, col) of the planted byte's pixel relative to the view: above, below, left, right, and in the stride gap past the right margin
SPOTS = {"above": (-1, 4), "below": (7, 4), "left": (3, -1), "right": (3, 9), "first_guard_pixel": (0, -17), "stride_gap": (3, 9 + 18 + 2),
         "last_row_tail": (6, 9), "top_left_corner": (-3, -17)}


@pytest.mark.parametrize("spot", SPOTS)
@pytest.mark.parametrize("kind", KINDS)
def test_take_names_a_stray_byte(kind, spot):
    c = canvas(kind)
    row, col = SPOTS[spot]
    p = V.psize(kind)
    off = ((c.top + row) * c.stride + c.left + col) * p + (p - 1)  # the pixel's last byte
    c.flat[off] = 0x5A
    assert c.stray() == (off, row, col)
    with pytest.raises(AssertionError, match=rf"byte {off} of the allocation, \(row, col\) = \({row}, {col}\)"):
        c.take(spot)
    c.flat[off] = V.SENTINEL
    assert c.stray() is None


def test_a_byte_inside_the_view_is_not_stray_and_the_shifted_frame_is_checked_too():
    c = V.Canvas("rgba_f32", 4, 4, 16, 2, 16, 2, shift_bytes=4, device="cpu")
    assert c.facts()["origin%16"] == 4
    c.view.fill_(1.0)
    assert c.stray() is None
    c.flat[3] = 0  # before the shifted frame's first byte
    assert c.stray()[0] == 3
    c.flat[3] = V.SENTINEL
    c.flat[c.shift + c.origin - 1] = 0  # the byte before the view's first pixel
    assert c.stray() == (c.shift + c.origin - 1, 0, -1)


def test_a_framed_buffer_names_a_written_guard_byte():
    f = V.Framed((3, 5, 7), 512 + 4, torch.float32, device="cpu")
    assert f.frames.shape == (3, 5, 7) and f.frames.data_ptr() % 16 == 4 and f.nbytes == 3 * 5 * 7 * 4
    f.frames.fill_(2.0)
    assert f.stray() is None and f.take().shape == (3, 5, 7)
    for off in (0, f.guard - 1, f.guard + f.nbytes, f.flat.numel() - 1):
        f.flat[off] = 0
        assert f.stray() == (off, off - f.guard)
        with pytest.raises(AssertionError, match=rf"byte {off - f.guard} relative to the buffer"):
            f.take("framed")
        f.flat[off] = V.SENTINEL
    assert f.stray() is None


def test_margins_below_the_guard_are_refused():
    for args in ((15, 2, 16, 2), (16, 1, 16, 2), (16, 2, 15, 2), (16, 2, 16, 1)):
        with pytest.raises(AssertionError):
            V.Canvas("u8", 4, 4, *args, device="cpu")


@pytest.mark.parametrize("kind", KINDS)
def test_every_placement_flips_the_term_it_names_and_no_other(kind):
    for name in V.placements(kind):
        for rows, cols in ((272, 272), (271, 269), (96, 287)):
            c = V.place(kind, rows, cols, name, device="cpu")  # place() asserts origin and stride from facts()
            f = c.facts()
            assert f["rows%2"] == rows % 2 and f["row_bytes%16"] == cols * V.psize(kind) % 16
            assert c.stray() is None

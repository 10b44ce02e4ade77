"""Image.convert between every ordered pair of the 17 storage forms (tests/color_routes.py: FORMS), bit for bit against the CPU oracle,
whose routing tests/test_color_routes.py pins to the reference's tables without a GPU. colorspaces.hip's next_hop restates thirteen dispatch
tables and the value is rounded to f32 after every hop, so a wrong hub moves last-place bits on some pixels and nothing else: every pair
has to be looked at, on colours that are in gamut and on values that are not.

The frame is 37 x 259 pixels: cols % 4 == 3 and one full 256-column wave plus a ragged end, every branch of the four-pixel kernels.
  in gamut   u8 forms: the lattice's own bytes read in that form (Rgba: a moving alpha; Gray: every byte value); float forms: the oracle's
             forward conversion of the lattice. Sixteen greys, black and white are in it: atan2(0, 0), delta == 0, cbrt(0).
  stretched  float forms: second and third fields times 1.5 (a grey: 1.5 y - 0.25), hue fields +400 / -400 on alternate rows, and in the
             last row one pixel each of NaN, +inf, -inf and -0.0: the clamps, cs_mod's wrap, sat == 0, l == 0 || l == 1. NaN counts as one
             class (assert_bits_equal_nan_class).
Pairs with (i + j) % 3 == 0 run a second time with source and destination as views one row and three columns into parents filled with a
sentinel; the parents' other bytes must keep it. The pairs the oracle refuses must be the pairs the device refuses."""
import functools

import numpy as np
import pytest

import zignal_amd as zg
from tests import color_routes as R
from tests.util import assert_bits_equal_nan_class

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS, COLS = 37, 259
DTYPE = {"u8": np.uint8, "f32": np.float32}
TORCH_DTYPE = {"u8": torch.uint8, "f32": torch.float32}
SENTINEL = 0xA5


def cs(space):
    return getattr(zg, "CS_" + space)


def name(form):
    return f"{form[0].capitalize()}({form[1]})"


@functools.lru_cache(maxsize=None)
def source(oracle, form, kind):
    """The pair tests' input in `form`: computed once, shared, never written."""
    space, t = form
    rgb = R.lattice_frame(ROWS, COLS)
    moving = (np.arange(ROWS * COLS) * 37 % 256).astype(np.uint8).reshape(ROWS, COLS)
    if t == "u8":
        assert kind == "in gamut"
        out = {1: moving, 3: rgb, 4: np.concatenate([rgb, moving[..., None]], -1)}[R.channels(space)]
    else:
        out = oracle.convert(rgb, zg.CS_RGB, cs(space), np.float32, R.channels(space))
        if space == "RGBA":
            out[..., 3] = moving.astype(np.float32) / np.float32(255)
        if kind == "stretched":
            if space == "GRAY":
                out = out * np.float32(1.5) - np.float32(0.25)
            else:
                out[..., 1:3] *= np.float32(1.5)
            if space in R.HUE_FIELD:
                out[0::2, :, R.HUE_FIELD[space]] += np.float32(400)
                out[1::2, :, R.HUE_FIELD[space]] -= np.float32(400)
            for i, v in enumerate((np.nan, np.inf, -np.inf, -0.0)):
                out[-1, 7 + 5 * i] = np.float32(v)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def parent_and_view(form, fill=None):
    """A (ROWS + 2) x (COLS + 6) parent whose every byte is the sentinel, and the ROWS x COLS view one row and three columns into it."""
    ch, esize = R.channels(form[0]), 1 if form[1] == "u8" else 4
    flat = torch.full(((ROWS + 2) * (COLS + 6) * ch * esize,), SENTINEL, dtype=torch.uint8, device="cuda")
    typed = flat.view(TORCH_DTYPE[form[1]]).view((ROWS + 2, COLS + 6) + ((ch,) if ch > 1 else ()))
    view = typed[1:ROWS + 1, 3:COLS + 3]
    if fill is not None:
        view.copy_(fill)
    return flat, view


def untouched(flat, form):
    p = R.channels(form[0]) * (1 if form[1] == "u8" else 4)
    bad = (flat != SENTINEL).view(ROWS + 2, (COLS + 6) * p)
    bad[1:ROWS + 1, 3 * p:(COLS + 3) * p] = False
    return not bool(bad.any())


@pytest.mark.parametrize("i", range(len(R.FORMS)), ids=[f"{s}_{t}" for s, t in R.FORMS])
def test_every_destination_from(oracle, i):
    src_form = R.FORMS[i]
    oracle_refuses, device_refuses, differ = [], [], []

    def check(got, want, what):  # every pair is looked at before the test fails, so one run names them all
        try:
            assert_bits_equal_nan_class(got, want, what)
        except AssertionError as e:
            differ.append(str(e))

    for kind in ("in gamut", "stretched") if src_form[1] == "f32" else ("in gamut",):
        host = source(oracle, src_form, kind)
        dev_src = torch.from_numpy(np.array(host, order="C")).cuda()
        for j, dst_form in enumerate(R.FORMS):
            what = f"{name(src_form)} -> {name(dst_form)}, {kind}, route {[name(f) for f in R.form_route(src_form, dst_form)]}"
            args = (cs(dst_form[0]), DTYPE[dst_form[1]])
            try:
                with np.errstate(all="ignore"):
                    want = oracle.convert(host, cs(src_form[0]), *args, R.channels(dst_form[0]))
            except RuntimeError:
                oracle_refuses.append((kind, dst_form))
                want = None
            try:
                got = zg.Image(dev_src).convert(*args, src_space=cs(src_form[0]))
                torch.cuda.synchronize()
            except zg.ZignalError as e:
                assert want is None, f"{what}: the device refuses a pair the oracle takes: {e}"
                device_refuses.append((kind, dst_form))
                got = None
            if want is None or got is None:
                continue
            check(got.to_numpy(), want, what)
            if (i + j) % 3 == 0:
                src_flat, src_view = parent_and_view(src_form, dev_src)
                dst_flat, dst_view = parent_and_view(dst_form)
                zg.Image(src_view).convert(*args, src_space=cs(src_form[0]), out=zg.Image(dst_view))
                torch.cuda.synchronize()
                check(dst_view.cpu().numpy(), want, what + ", views")
                assert untouched(dst_flat, dst_form), what + ": a byte outside the destination view was written"
                assert untouched(src_flat, src_form), what + ": the source's parent was written"
    assert not differ, f"{len(differ)} differences:\n" + "\n".join(differ)
    assert device_refuses == oracle_refuses, f"from {name(src_form)}: the device refuses {device_refuses}, the oracle {oracle_refuses}"

"""The oracle's colour routing against tests/color_routes.py, the hand transcription of the reference's `.to()` tables: the oracle's one-call
convert must equal the conversion functions applied one at a time along the transcribed route, with the value rounded to f32 (or to bytes)
between them. No GPU: this pins the checker, so that tests/test_gpu_color_pairs.py compares the kernels with a route that two independent
readings of src/color.zig agree on."""
import numpy as np
import pytest

import zignal_amd as zg
from tests import color_routes as R
from tests.util import assert_bits_equal

DTYPE = {"u8": np.uint8, "f32": np.float32}


def cs(space):
    return getattr(zg, "CS_" + space)


def one_step(oracle, img, src, dst, last):
    """One conversion function, or one `.as()`, through the oracle's own entry. Gray(f32).as(u8) inside a longer chain is
    @round(255 * clamp(y, 0, 1)) in f32 (color.zig:554) while the oracle's scalar -> scalar call is convertColor's f64 form (:114-118): the
    chain's step is written out here, the one-call pair Gray(f32) -> Gray(u8) keeps the oracle's."""
    if src == ("GRAY", "f32") and dst == ("GRAY", "u8") and not last:
        y = np.where(np.isnan(img), np.float32(1), np.clip(img, np.float32(0), np.float32(1))) * np.float32(255)
        return (np.trunc(np.abs(y) + np.float32(0.5))).astype(np.uint8)  # @round: halves away from zero, y >= 0 here
    return oracle.convert(img, cs(src[0]), cs(dst[0]), DTYPE[dst[1]], R.channels(dst[0]))


def in_form(oracle, rgb, form):
    return rgb if form == ("RGB", "u8") else oracle.convert(rgb, zg.CS_RGB, cs(form[0]), DTYPE[form[1]], R.channels(form[0]))


def test_table_covers_every_exported_space():
    exported = {n[3:]: getattr(zg, n) for n in dir(zg) if n.startswith("CS_")}
    assert set(exported) == set(R.SPACES) == set(R.NEXT_HOP), sorted(set(exported) ^ set(R.SPACES))
    assert sorted(exported.values()) == list(range(len(R.SPACES)))
    for cur in R.SPACES:
        assert set(R.NEXT_HOP[cur]) == set(R.SPACES) - {cur}
    assert len(R.FORMS) == 17 and len(set(R.FORMS)) == 17
    assert {s for s, t in R.FORMS if t == "u8"} == set(R.U8_SPACES) and {s for s, t in R.FORMS if t == "f32"} == set(R.SPACES)


def test_every_route_ends():
    longest = max(((a, b) for a in R.SPACES for b in R.SPACES), key=lambda p: len(R.route(*p)))
    for a in R.SPACES:
        for b in R.SPACES:
            hops = R.route(a, b)
            assert len(hops) <= 8 and (hops[-1] if hops else a) == b and len(set(hops)) == len(hops), (a, b, hops)
    # colorspaces.hip, cs_to_f32: "longest route: Lch -> Lab -> Xyz -> Rgb -> Hsl"
    assert R.route("LCH", "HSL") == ["LAB", "XYZ", "RGB", "HSL"]
    assert len(R.route(*longest)) == len(R.route("LCH", "HSL")) == 4, longest
    for src in R.FORMS:
        for dst in R.FORMS:
            steps = R.form_route(src, dst)
            assert (steps[-1] if steps else src) == dst and all(f in R.FORMS for f in steps), (src, dst, steps)


@pytest.mark.parametrize("src", R.FORMS, ids=lambda f: f"{f[0]}_{f[1]}")
def test_oracle_one_call_equals_the_route_walked(oracle, src):
    rgb = R.lattice_frame(64, 259)
    start = in_form(oracle, rgb, src)
    for dst in R.FORMS:
        try:
            want = oracle.convert(start, cs(src[0]), cs(dst[0]), DTYPE[dst[1]], R.channels(dst[0]))
        except RuntimeError:
            continue  # a pair the library does not take: tests/test_gpu_color_pairs.py holds the device to the same list
        steps = R.form_route(src, dst)
        img, cur = start, src
        for nxt in steps:
            img, cur = one_step(oracle, img, cur, nxt, last=len(steps) == 1), nxt
        assert_bits_equal(img, want, f"{src} -> {dst} along {steps}")

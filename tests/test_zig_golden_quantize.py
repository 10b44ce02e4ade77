"""The `quantize` section of tests/golden/zig_golden.json (made by tools/zig_golden.zig with a real Zig toolchain and the zignal module;
absent here, so this file is skipped): the reference's own medianCut on frames with many equal keys per dimension, and its own dither
modes, inputs included, against the restatements of tests/quantize_ref.py, which the library equals byte for byte
(tests/test_quantize_oracle.py, tests/test_gpu_quantize.py). What only the real thing can pin: the order Zig's std.sort.heap, which is
unstable, leaves among equal keys; the adaptive palette rests on a restatement of it."""
import json
import os

import numpy as np
import pytest

from tests import quantize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "zig_golden.json")

pytestmark = pytest.mark.skipif(not os.path.exists(PATH), reason="tests/golden/zig_golden.json absent: run tools/zig_golden.zig with a Zig >= 0.17-dev toolchain")


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        g = json.load(f)
    if "quantize" not in g:
        pytest.skip("zig_golden.json predates the quantize section: run tools/zig_golden.zig again")
    return g["quantize"]


def _frame(c):
    return np.asarray(c["data"], np.uint8).reshape(c["rows"], c["cols"], 3)


def test_the_reference_cuts_the_palettes_the_restatement_cuts(golden):
    assert len(golden["median_cut"]) == 3
    for c in golden["median_cut"]:
        img = _frame(c)
        for p in c["palettes"]:
            want = np.asarray(p["palette"], np.uint8).reshape(-1, 3)
            assert R.median_cut(img, p["max_colors"]).tobytes() == want.tobytes(), (c["rows"], c["cols"], p["max_colors"])


def test_the_reference_dithers_what_the_restatements_dither(golden):
    palette = np.array([[64, 64, 64], [192, 192, 192]], np.uint8)
    lut = R.palette_lut(palette)
    assert {c["mode"] for c in golden["dither"]} == {R.FLOYD_STEINBERG, R.ATKINSON, R.ORDERED}
    for c in golden["dither"]:
        img = _frame(c)
        want = np.asarray(c["out"], np.uint8).reshape(img.shape)
        assert R.dither(img, palette, lut, c["mode"]).tobytes() == want.tobytes(), c["mode"]
        if c["mode"] != R.ORDERED:
            assert R.dither_literal(img, palette, lut, c["mode"]).tobytes() == want.tobytes(), c["mode"]

"""The `flood_fill` section of tests/golden/zig_golden.json (made by tools/zig_golden.zig with a real Zig toolchain and the zignal module;
absent here, so this file is skipped): Image(T).floodFill of the reference itself, inputs included, against the restatements of
tests/flood_ref.py, which the device equals byte for byte (tests/test_gpu_flood.py). What only the real thing can pin: that the
reference's traversal leaves the connected component the restatements derive, and its f64 square root at the thresholds on a boundary."""
import json
import os

import numpy as np
import pytest

from tests import flood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "zig_golden.json")

pytestmark = pytest.mark.skipif(not os.path.exists(PATH), reason="tests/golden/zig_golden.json absent: run tools/zig_golden.zig with a Zig >= 0.17-dev toolchain")

LAYOUT = {"u8": (np.uint8, 1), "f32": (np.float32, 1), "rgb_u8": (np.uint8, 3), "rgba_f32": (np.float32, 4)}


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        g = json.load(f)
    if "flood_fill" not in g:
        pytest.skip("zig_golden.json predates the flood_fill section: run tools/zig_golden.zig again")
    return g["flood_fill"]


def _image(data, rows, cols, pixel):
    dtype, ch = LAYOUT[pixel]
    a = np.asarray(data, np.uint8).view(dtype)
    return a.reshape(rows, cols) if ch == 1 else a.reshape(rows, cols, ch)


def test_the_reference_fills_what_the_restatements_fill(golden):
    assert {c["pixel"] for c in golden} == set(LAYOUT)
    for c in golden:
        src = _image(c["data"], c["rows"], c["cols"], c["pixel"])
        fill = _image(c["fill"], 1, 1, c["pixel"])[0, 0]
        changed = 0
        for f in c["fills"]:
            threshold = float(np.array([f["threshold_bits"]], np.uint64).view(np.float64)[0])
            want = _image(f["out"], c["rows"], c["cols"], c["pixel"])
            for fn in (R.flood_fill_fast, R.flood_fill_literal):
                got, n = fn(src, f["row"], f["col"], fill, threshold, f["connectivity"], ("seed", "neighbor")[f["mode"]])
                assert got.tobytes() == want.tobytes(), (c["pixel"], f["threshold_bits"], f["connectivity"], f["mode"], fn.__name__)
            changed += n > 1
        assert changed > 0

"""The `hough` section of tests/golden/zig_golden.json (made by tools/zig_golden.zig with a real Zig toolchain and the zignal module;
absent here, so this file is skipped): the tables of HoughTransform.init, compute and findLines of the reference itself, inputs
included, against the restatements of tests/hough_ref.py, which the library and the device equal bit for bit
(tests/test_hough_oracle.py, tests/test_gpu_hough.py). What only the real thing can pin: the table entries at the quarter points,
which rest on the last bit of Zig's f64 @cos / @sin, and the order std.mem.sort leaves equal scores in."""
import json
import os

import numpy as np
import pytest

import zignal_amd as zg
from tests import hough_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "zig_golden.json")

pytestmark = pytest.mark.skipif(not os.path.exists(PATH), reason="tests/golden/zig_golden.json absent: run tools/zig_golden.zig with a Zig >= 0.17-dev toolchain")


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        g = json.load(f)
    if "hough" not in g:
        pytest.skip("zig_golden.json predates the hough section: run tools/zig_golden.zig again")
    return g["hough"]


def _f32(bits: int) -> float:
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def _lines(rows) -> np.ndarray:
    out = np.zeros(len(rows), zg.HOUGH_LINE_DTYPE)
    for i, (angle, radius, score, x1, y1, x2, y2) in enumerate(rows):
        out[i] = (_f32(angle), _f32(radius), score, (_f32(x1), _f32(y1)), (_f32(x2), _f32(y2)))
    return out


def test_tables_quarter_points_included(golden):
    quarter = 0
    for t in golden["tables"]:
        size = t["size"]
        for got in (R.tables(size), zg.HoughTransform.tables(size)):
            assert got[0].tolist() == t["cos"] and got[1].tolist() == t["sin"], size
        e = R.even_size(size)
        quarter += e % 4 == 0
    assert quarter > 0


def test_compute_and_find_lines(golden):
    ties = 0
    for c in golden["cases"]:
        size = c["size"]
        edges = np.asarray(c["edges"], np.uint8).reshape(c["rows"], c["cols"])
        want = np.asarray(c["accumulator"], np.uint32).reshape(size, size)
        for fn in (R.compute, R.compute_fast):
            assert np.array_equal(fn(edges, tuple(c["box"]), np.zeros((size, size), np.uint32), size), want), (size, fn.__name__)
        for f in c["finds"]:
            _, got = R.find_lines(want, size, f["threshold"], _f32(f["angle_bits"]), _f32(f["radius_bits"]))
            assert got.tobytes() == _lines(f["lines"]).tobytes(), (size, f["threshold"], _f32(f["angle_bits"]), _f32(f["radius_bits"]))
            ties += sum(1 for a, b in zip(f["lines"], f["lines"][1:]) if a[2] == b[2])
    assert ties > 0  # the inputs do put the sort's stability to the test

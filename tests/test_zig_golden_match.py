"""The `matcher` section of tests/golden/zig_golden.json (made by tools/zig_golden.zig with a real Zig toolchain and the zignal module;
absent here, so this file is skipped): BruteForceMatcher.match / knnMatch / radiusMatch of the reference itself on clustered
descriptors, inputs included, against the restatements of tests/match_ref.py, which the device equals bit for bit
(tests/test_gpu_match.py). What only the real thing can pin is the order of equal distances out of std.mem.sort."""
import json
import os

import numpy as np
import pytest

from tests import match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "zig_golden.json")

pytestmark = pytest.mark.skipif(not os.path.exists(PATH), reason="tests/golden/zig_golden.json absent: run tools/zig_golden.zig with a Zig >= 0.17-dev toolchain")


@pytest.fixture(scope="module")
def cases():
    with open(PATH) as f:
        g = json.load(f)
    if "matcher" not in g:
        pytest.skip("zig_golden.json predates the matcher section: run tools/zig_golden.zig again")
    out = []
    for c in g["matcher"]:
        q = R.as_descriptors(np.asarray(c["query"], np.uint8).reshape(c["nq"], 32))
        t = R.as_descriptors(np.asarray(c["train"], np.uint8).reshape(c["nt"], 32))
        out.append((q, t, c))
    return out


def _f32(bits: int) -> float:
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def _matches(rows) -> np.ndarray:
    out = np.zeros(len(rows), R.MATCH_DTYPE)
    for i, (q, t, d) in enumerate(rows):
        out[i] = (q, t, np.float32(_f32(d)))
    return out


def _same_rows(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == _matches(w).tobytes(), f"{what}: row {i}: {g} here, {w} from Zig"


def test_match(cases):
    for q, t, c in cases:
        for m in c["match"]:
            p = R.Params(bool(m["cross_check"]), m["max_distance"], _f32(m["ratio_bits"]))
            for fn in (R.match_fast, R.match_loops):
                assert fn(q, t, p)[0].tobytes() == _matches(m["matches"]).tobytes(), (c["nq"], c["nt"], p, fn.__name__)


def test_knn_keeps_equal_distances_in_train_order(cases):
    ties = 0
    for q, t, c in cases:
        for m in c["knn"]:
            p = R.Params(max_distance=m["max_distance"])
            _same_rows(R.knn_fast(q, t, p, m["k"]), m["rows"], f"knn {c['nq']}x{c['nt']} k={m['k']} max_distance={m['max_distance']}")
            ties += sum(1 for row in m["rows"] for a, b in zip(row, row[1:]) if a[2] == b[2])
    assert ties > 0  # the inputs do put the sort's stability to the test


def test_radius(cases):
    for q, t, c in cases:
        for m in c["radius"]:
            r = _f32(m["max_dist_bits"])
            _same_rows(R.radius_fast(q, t, r), m["rows"], f"radius {c['nq']}x{c['nt']} r={r}")

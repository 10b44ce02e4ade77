"""The `orb` section of tests/golden/zig_golden.json (made by tools/zig_golden.zig with a real Zig toolchain; absent here, so this
file is skipped): ORB's comptime orientation weight table, radiansToDegrees(atan2) and @cos / @sin of degreesToRadians against
the restatements of tests/orb_ref.py, which the device equals bit for bit (tests/test_gpu_orb.py). Whether Zig's comptime @exp and
its degree / radian conversions equal `exp`, `ang * f32(180 / pi)` and `ang * f32(pi / 180)` at the last ulp is what this pins."""
import json
import os

import numpy as np
import pytest

from tests import orb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "zig_golden.json")

pytestmark = pytest.mark.skipif(not os.path.exists(PATH), reason="tests/golden/zig_golden.json absent: run tools/zig_golden.zig with a Zig >= 0.17-dev toolchain")


@pytest.fixture(scope="module")
def orb():
    with open(PATH) as f:
        g = json.load(f)
    if "orb" not in g:
        pytest.skip("zig_golden.json predates the orb section: run tools/zig_golden.zig again")
    return g["orb"]


def _differences(got, want_bits, what):
    g = np.ascontiguousarray(got, np.float32).view(np.uint32).ravel()
    w = np.asarray(want_bits, np.uint32).ravel()
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} values differ from Zig's; first at {int(bad[0])}: {g[bad[0]]:#010x} here, {w[bad[0]]:#010x} from Zig"


def test_orientation_weights(orb):
    _differences(R.orientation_weights(), orb["weights"], "orientation_weights (comptime @exp)")


def test_atan2_in_degrees(orb):
    t = np.asarray(orb["atan2_degrees"], np.uint32)
    y, x = t[:, 0].copy().view(np.float32), t[:, 1].copy().view(np.float32)
    got = np.array([R.atan2f(a, b) * R.DEG for a, b in zip(y, x)], np.float32)
    _differences(got, t[:, 2], "radiansToDegrees(atan2(y, x))")


def test_cos_and_sin_of_degrees(orb):
    t = np.asarray(orb["cos_sin_of_degrees"], np.uint32)
    a = t[:, 0].copy().view(np.float32)
    rad = (a * R.RAD).astype(np.float32)
    _differences(np.array([R.cosf(r) for r in rad], np.float32), t[:, 1], "@cos(degreesToRadians(a))")
    _differences(np.array([R.sinf(r) for r in rad], np.float32), t[:, 2], "@sin(degreesToRadians(a))")

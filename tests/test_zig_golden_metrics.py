"""The `metrics` section of tests/golden/zig_golden.json (made by tools/zig_golden.zig with a real Zig toolchain; absent here, so this file
is skipped): generateSsimWindow's weights, @exp at the window's arguments and std.math.log10 on a sweep, in f64 bit patterns, against
zg_ssim_window_host, zg_exp_f64_host and zg_log10_f64_host. What only the real thing can pin: the last ulp of the two restated functions."""
import json
import os

import numpy as np
import pytest

import zignal_amd as zg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "zig_golden.json")

pytestmark = pytest.mark.skipif(not os.path.exists(PATH), reason="tests/golden/zig_golden.json absent: run tools/zig_golden.zig with a Zig >= 0.17-dev toolchain")


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        g = json.load(f)
    if "metrics" not in g:
        pytest.skip("zig_golden.json predates the metrics section: run tools/zig_golden.zig again")
    return g["metrics"]


def _f64(values):
    return np.asarray(values, np.uint64).view(np.float64)


def test_the_window_has_zigs_bits(golden):
    mine = zg.ssim_window().ravel().view(np.uint64)
    assert np.array_equal(mine, np.asarray(golden["ssim_window_comptime"], np.uint64))
    assert golden["ssim_window_comptime"] == golden["ssim_window_runtime"]


def test_exp_and_log10_have_zigs_bits(golden):
    lib = zg.lib()
    for name, fn in (("exp", lib.zg_exp_f64_host), ("log10", lib.zg_log10_f64_host)):
        pairs = np.asarray(golden[name], np.uint64)
        got = np.array([fn(float(x)) for x in _f64(pairs[:, 0])])
        assert np.array_equal(got.view(np.uint64), pairs[:, 1]), name

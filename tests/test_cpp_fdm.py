"""The C++ mirror of feature distribution matching (zignal::FeatureDistributionMatching<T> in zignal_amd/cpp/zignal_hip.hpp): compiles
against the C ABI on the CPU; tests/cpp/test_fdm.cpp runs on the GPU as a bare process and compares the host and device forms with a result
recorded from tests/fdm_ref.py (tests/golden/fdm_cpp_rgb.rgb — written by the restatement, not by the device), which the second test here
holds to the restatement as it is now, together with the guards that make byte equality the right check for it."""
import os
import subprocess

import numpy as np
import pytest

from tests import fdm_cases as K
from tests import fdm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(CPP, "test_fdm")
DELTA = 100 * 5.4e-13  # tests/test_gpu_fdm.py


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_fdm.cpp"), "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir],
                   check=True)


def noise(s, shift):
    """test_fdm.cpp's noise(): three mixed bytes of an LCG a pixel, 40 x 48."""
    out = np.zeros((40 * 48, 3), np.uint8)
    for i in range(40 * 48):
        v = []
        for _ in range(3):
            s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
            v.append(s >> 24)
        out[i] = (v[0] // 2 + 60 - shift, v[0] // 4 + v[1] // 2 + 30, v[1] // 4 + v[2] // 2 + v[0] // 8 + shift)
    return out.reshape(40, 48, 3)


def patterns():
    return noise(5, 0), noise(77, 20)


def test_cpp_fdm_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


def test_recording_is_the_restatement_of_today_and_is_guarded():
    src, tgt = patterns()
    target = R.prepare_target(tgt)
    x = R.source_transform(src, target)
    want, pre = R.apply(src, x, return_pre=True)
    with open(os.path.join(GOLDEN, "fdm_cpp_rgb.rgb"), "rb") as f:
        assert f.read() == want.tobytes()
    assert float(np.min(np.abs((pre - np.floor(pre)) - 0.5))) > DELTA
    assert all(v == 0.0 or not (1e-11 < v < 1e-9) for v in list(target["s"]) + list(x["source_s"]))
    assert not np.array_equal(want, src)
    # and the restatement fed the exact-moment statistics gives the same bytes: no sign of the SVD hangs on Welford's rounding noise here
    # (on fdm.zig's own 50 x 50 pattern one does: cov(r, g) is exactly 0 there and 1.6e-19 after the recurrence)
    assert np.array_equal(K.match_with_exact_statistics(src, tgt), want)


@pytest.mark.gpu
def test_cpp_fdm_against_the_recorded_restatement():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp fdm ok" in out.stdout, out.stdout + out.stderr

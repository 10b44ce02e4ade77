"""The C++ mirror of geometry fitting (zignal_amd/cpp/zignal_hip_transform.hpp): compiles against the C ABI on the CPU;
tests/cpp/test_transform.cpp runs on the GPU as a bare process and compares zignal::fit and zignal::DeviceFit with records written by
tests/transform_ref.py (tests/golden/transform_cpp_records.bin: written by the restatement, not by the device), which the second test here
holds to the restatement as it is now."""
import os
import subprocess

import numpy as np
import pytest

from tests import transform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(CPP, "test_transform")
N = 12


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_transform.cpp"), "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir],
                   check=True)


def points():
    """test_transform.cpp's points(): integers from an LCG, and their image under an integer affine map plus 0 .. 3 of noise."""
    state = [2024]

    def nxt():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        return state[0] >> 16
    f, t = [], []
    for _ in range(N):
        x, y = nxt() % 320, nxt() % 240
        tx = 2 * x - y + 7 + nxt() % 4
        ty = x + 2 * y - 5 + nxt() % 4
        f.append((x, y))
        t.append((tx, ty))
    return f, t


def records():
    """status and the nine coefficients as f64 for kind 0 .. 2 and scalar f32, f64: 60 doubles."""
    f, t = points()
    out = []
    with np.errstate(all="ignore"):
        for kind in (R.SIMILARITY, R.AFFINE, R.PROJECTIVE):
            for T in (R.F32, R.F64):
                status, m = R.fit(T, kind, [(T(a), T(b)) for a, b in f], [(T(a), T(b)) for a, b in t])
                out += [float(status)] + [float(v) for v in m]
    return np.array(out, np.float64)


def test_cpp_transform_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


def test_recording_is_the_restatement_of_today():
    want = records()
    with open(os.path.join(GOLDEN, "transform_cpp_records.bin"), "rb") as fh:
        assert fh.read() == want.tobytes()
    statuses = want.reshape(6, 10)[:, 0]
    assert (statuses == R.OK).sum() >= 5  # a recording of failures would pin nothing


@pytest.mark.gpu
def test_cpp_transform_against_the_recorded_restatement():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp transform ok" in out.stdout, out.stdout + out.stderr

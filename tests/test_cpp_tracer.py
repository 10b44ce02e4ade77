"""The C++ mirror of the tracer (zignal::Tracer in zignal_amd/cpp/zignal_hip.hpp): compiles against the C ABI on the CPU;
tests/cpp/test_tracer.cpp runs on the GPU as a bare process and compares the host and device forms with
tests/golden/tracer_cpp_paths.bin, which tests/tracer_ref.py wrote."""
import os
import subprocess

import numpy as np
import pytest

from tests import tracer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_tracer")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tracer_cpp_paths.bin")


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_tracer.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def test_cpp_tracer_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


def test_the_fixture_is_what_the_restatement_gives():
    e = R.cpp_frame()
    counts, offsets, points = R.pack(R.trace(e))
    want = np.array(e.shape, "<u4").tobytes() + e.tobytes() + counts.astype("<u4").tobytes() + offsets.astype("<u4").tobytes() + points.astype("<f4").tobytes()
    with open(GOLDEN, "rb") as f:
        assert f.read() == want
    assert counts[0] >= 4 and len(want) < 8192


@pytest.mark.gpu
def test_cpp_tracer_against_the_fixture():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp tracer ok" in out.stdout, out.stdout + out.stderr

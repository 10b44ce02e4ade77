"""The C++ mirror of seam carving (Image<T>::seamCarve and DeviceImage<T>::seamCarve in zignal_amd/cpp/zignal_hip.hpp): compiles against
the C ABI on the CPU; tests/cpp/test_seam.cpp runs on the GPU as a bare process and compares the staged entry points and the host and
device forms of the iteration with the example's loops written out in C++."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_seam")


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_seam.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def test_cpp_seam_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_seam_against_the_examples_loops():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp seam ok" in out.stdout, out.stdout + out.stderr

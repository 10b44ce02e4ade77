"""The C++ mirror of the quantisation module (DeviceImage<T>::colorHistogram, medianCut, dither, mapToPalette and Palette in
zignal_amd/cpp/zignal_hip.hpp): compiles against the C ABI on the CPU; tests/cpp/test_quantize.cpp runs on the GPU as a bare process
and compares the device forms with the reference's loops written out in C++."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_quantize")


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_quantize.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def test_cpp_quantize_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_quantize_against_the_reference_loops():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp quantize ok" in out.stdout, out.stdout + out.stderr

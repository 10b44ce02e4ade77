"""The C++ mirror of the order-statistic blurs (Image<T> and DeviceImage<T>::percentileBlur, minBlur, maxBlur, midpointBlur,
alphaTrimmedMeanBlur in zignal_amd/cpp/zignal_hip.hpp): compiles against the C ABI on the CPU; tests/cpp/test_order_stat.cpp runs on the GPU
as a bare process and compares the host and device forms, at radius 2 and 16, with a sort of every window written out in C++."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_order_stat")


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", BIN, os.path.join(CPP, "test_order_stat.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def test_cpp_order_stat_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_order_stat_against_a_window_sort():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp order-stat ok" in out.stdout, out.stdout + out.stderr

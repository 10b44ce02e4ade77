"""The C++ mirror of the QR detector (zignal::QrDetector in zignal_amd/cpp/zignal_hip.hpp): compiles against the C ABI on the CPU;
tests/cpp/test_qr.cpp runs on the GPU as a bare process and compares the host and device forms with tests/golden/qr_cpp_case.bin,
which tests/qr_ref.py wrote."""
import os
import subprocess

import numpy as np
import pytest

from tests import qr_cases as K
from tests import qr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_qr")
GOLDEN = os.path.join(ROOT, "tests", "golden", "qr_cpp_case.bin")


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_qr.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def fixture_bytes():
    binary = K.binary("v2_axis")
    det, grids, modules = R.pack(K.want("v2_axis"))
    return np.array(binary.shape, "<u4").tobytes() + binary.tobytes() + det.tobytes() + np.array([len(grids)], "<u4").tobytes() + grids.tobytes() + modules.tobytes()


def test_cpp_qr_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


def test_the_fixture_is_what_the_restatement_gives():
    want = fixture_bytes()
    with open(GOLDEN, "rb") as f:
        assert f.read() == want
    assert len(K.want("v2_axis")["grids"]) >= 2 and len(want) < 32768 and R.UNDEFINED_CASTS[0] == 0


@pytest.mark.gpu
def test_cpp_qr_against_the_fixture():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp qr ok" in out.stdout, out.stdout + out.stderr

"""The C++ mirror of the Canvas arcs (Canvas<T>::drawArc and fillArc in zignal_amd/cpp/zignal_hip.hpp): compiles against the C ABI on the
CPU; tests/cpp/test_canvas_arcs.cpp runs on the GPU as a bare process and compares the host and device forms with results recorded from
tests/canvas_arcs_ref.py (tests/golden/canvas_arcs_cpp_*.rgba), which the second test here holds to the restatement as it is now."""
import os
import subprocess

import pytest

from tests import canvas_arcs_ref as AR
from tests import canvas_cases as K
from tests.test_cpp_canvas_curves import frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(CPP, "test_canvas_arcs")


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_canvas_arcs.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def arcs(width, mode, color):
    """test_canvas_arcs.cpp's arcs()."""
    return [AR.fill_arc((30.0, 24.0), 20.0, 0.5, 4.0, color, mode), K.line(2.0, 3.0, 60.0, 40.0, color, 2, mode),
            AR.arc((32.0, 22.5), 18.0, 4.0, 1.0, color, width, mode), AR.arc((16.0, 16.0), 12.0, -2.5, -0.5, color, 1, mode),
            AR.fill_arc((44.25, 30.5), 11.0, 5.5, 8.0, color, mode), AR.arc((40.0, 24.0), 9.0, 0.25, 7.0, color, width, mode)]


RECORDINGS = {"canvas_arcs_cpp_soft.rgba": (2, AR.SOFT, (250, 20, 60, 128)), "canvas_arcs_cpp_fast.rgba": (3, AR.FAST, (10, 200, 90, 255))}


def test_cpp_canvas_arcs_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.parametrize("name", sorted(RECORDINGS))
def test_recordings_are_the_restatement_of_today(name):
    want = AR.run(frame(), arcs(*RECORDINGS[name]))
    with open(os.path.join(GOLDEN, name), "rb") as f:
        assert f.read() == want.tobytes()
    assert want.tobytes() != frame().tobytes()


@pytest.mark.gpu
def test_cpp_canvas_arcs_against_the_recorded_restatement():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp canvas arcs ok" in out.stdout, out.stdout + out.stderr

"""The C++ mirror of the Canvas curves (Canvas<T>::drawQuadraticBezier, drawCubicBezier, drawSplinePolygon, fillSplinePolygon in zignal_amd/cpp/zignal_hip.hpp): compiles against the C ABI on the CPU; tests/cpp/test_canvas_curves.cpp runs on the
GPU as a bare process and compares the host and device forms with results recorded from tests/canvas_curves_ref.py
(tests/golden/canvas_curves_cpp_*.rgba), which the second test here holds to the restatement as it is now."""
import os
import subprocess

import numpy as np
import pytest

from tests import canvas_curves_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(CPP, "test_canvas_curves")
ROWS, COLS = 48, 64


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_canvas_curves.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def frame():
    """test_canvas_curves.cpp's frame(): an LCG over the pixels, alpha 0, 140 or 255."""
    img = np.zeros((ROWS, COLS, 4), np.uint8)
    s = 99
    for r in range(ROWS):
        for c in range(COLS):
            s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
            img[r, c] = ((s >> 24) & 255, (s >> 16) & 255, (s >> 8) & 255, 0 if s & 3 == 0 else (140 if s & 3 == 1 else 255))
    return img


def curves(width, mode, color):
    """test_canvas_curves.cpp's curves()."""
    return [CR.quad_bezier((5.0, 42.0), (32.25, -10.0), (60.0, 40.0), color, width, mode),
            CR.cubic_bezier((3.0, 24.0), (20.0, 1.0), (45.0, 47.0), (61.0, 22.5), color, width, mode),
            CR.spline_polygon([(20, 10), (52, 12), (45, 40), (12, 36)], color, width, 0.3, mode),
            CR.fill_spline_polygon([(32, 6), (55, 15), (58, 34), (32, 44), (10, 35), (6, 14)], color, 0.5, mode)]


RECORDINGS = {"canvas_curves_cpp_soft.rgba": (2, CR.SOFT, (250, 20, 60, 128)), "canvas_curves_cpp_fast.rgba": (3, CR.FAST, (10, 200, 90, 255))}


def test_cpp_canvas_curves_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.parametrize("name", sorted(RECORDINGS))
def test_recordings_are_the_restatement_of_today(name):
    want = CR.run(frame(), curves(*RECORDINGS[name]))
    with open(os.path.join(GOLDEN, name), "rb") as f:
        assert f.read() == want.tobytes()
    assert want.tobytes() != frame().tobytes()


@pytest.mark.gpu
def test_cpp_canvas_curves_against_the_recorded_restatement():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp canvas curves ok" in out.stdout, out.stdout + out.stderr

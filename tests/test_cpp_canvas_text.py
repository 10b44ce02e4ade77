"""The C++ mirror of drawText (BitmapFont and Canvas<T>::drawText in zignal_amd/cpp/zignal_hip.hpp): compiles against the C ABI on the CPU;
tests/cpp/test_canvas_text.cpp runs on the GPU as a bare process and compares the host and device forms with results recorded from
tests/canvas_text_ref.py (tests/golden/canvas_text_cpp_*.rgba — written by the restatement, not by the device), which the second test
here holds to the restatement as it is now. The two fonts are made here as the C++ file makes them."""
import os
import subprocess

import pytest

from tests import canvas_cases as K
from tests import canvas_curves_ref as CR
from tests import canvas_text_ref as TR
from tests.test_cpp_canvas_curves import frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(CPP, "test_canvas_text")


def _build():
    lib_dir = os.path.join(ROOT, "zignal_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, os.path.join(CPP, "test_canvas_text.cpp"),
                    "-L" + lib_dir, "-lzignal_hip", "-Wl,-rpath," + lib_dir], check=True)


def noise(s, count):
    """test_canvas_text.cpp's noise(): the top byte of the frame's LCG."""
    out = bytearray()
    for _ in range(count):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(s >> 24)
    return out


def fixed_font():
    data = noise(7, 64)
    data[0:8] = bytes([0x81, 0x81, 0x81, 0x81, 0xFF, 0x81, 0x81, 0x81])
    data[8:16] = bytes([0x7E, 0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x7E])
    data[56:64] = bytes([0xFF, 0x81, 0x81, 0x81, 0x81, 0x81, 0x81, 0xFF])
    return TR.Font(8, 8, ord("H"), ord("O"), bytes(data))


def table_font():
    glyphs = [TR.Glyph(0x2192, 7, 5, 0, 3, 0, 40), TR.Glyph(ord("j"), 6, 12, -2, 1, 5, 0), TR.Glyph(0x3A9, 11, 14, -1, -2, 12, 12)]
    return TR.Font(9, 10, 0, 0, bytes(noise(11, 45)), glyphs)


def scene(scale, mode, color):
    """test_canvas_text.cpp's scene(), as the reference's calls in order."""
    out = CR.run(frame(), [K.fill_rect(4.0, 3.0, 56.0, 40.0, (20, 30, 200, 160), TR.SOFT)])
    out = TR.run(out, fixed_font(), [TR.text("HI\nOK", (6.5, 5.25), color, scale, mode)])
    out = CR.run(out, [K.line(2.0, 8.0, 60.0, 30.0, (250, 250, 10, 128), 3, TR.SOFT)])
    out = TR.run(out, fixed_font(), [TR.text("NO", (-3.0, 20.5), color, 1.0, mode)])
    return TR.run(out, table_font(), [TR.text("jΩ→j", (30.0, 28.0), color, scale, mode)])


RECORDINGS = {"canvas_text_cpp_soft.rgba": (2.5, TR.SOFT, (250, 20, 60, 128)), "canvas_text_cpp_fast.rgba": (1.5, TR.FAST, (10, 200, 90, 255))}


def test_cpp_canvas_text_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.parametrize("name", sorted(RECORDINGS))
def test_recordings_are_the_restatement_of_today(name):
    want = scene(*RECORDINGS[name])
    with open(os.path.join(GOLDEN, name), "rb") as f:
        assert f.read() == want.tobytes()
    assert want.tobytes() != frame().tobytes()
    assert fixed_font().get_text_bounds("HI\nOK", 2.5)[2:] == (40.0, 40.0) and table_font().get_text_bounds("jΩ→j", 1.0)[2:] == (22.0, 10.0)


@pytest.mark.gpu
def test_cpp_canvas_text_against_the_recorded_restatement():
    if not os.path.exists(BIN):
        _build()
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)  # one attempt: a failure is a failure
    assert out.returncode == 0 and "cpp canvas text ok" in out.stdout, out.stdout + out.stderr

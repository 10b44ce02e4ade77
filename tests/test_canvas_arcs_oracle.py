"""tests/canvas_arcs_ref.py, the yardstick of the device's drawArc and fillArc, against the reference itself: the MD5 sums it records for its
own arc renderings (src/canvas/tests/regression.zig) and the behaviour its own arc tests assert (src/canvas/tests/arcs.zig); the two ways
@mod may be lowered agree on every angle the suites use; the device's per-pixel form of fillArcFast equals the literal loops; packing, the
declarations in every binding, and the host form's contract check, which runs before any device is asked for."""
from __future__ import annotations

import hashlib
import math
import os
import re

import numpy as np
import pytest

from tests import canvas_arcs_ref as AR
from tests.canvas_arcs_ref import F, FAST, SOFT

_DOC, _GOLDEN = AR.golden_cases()
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi

# Every (start, end) pair tests/test_gpu_canvas_arcs.py draws with, beside the goldens': exact multiples of pi / 2, wraps, negative
# angles, both above 2 pi, spans just below and above pi, start == end, spans at and above 2 pi. None lies in (-1e-6, 0) modulo 2 pi.
ANGLE_PAIRS = [(0.0, PI / 2), (PI / 2, PI), (PI, 3 * PI / 2), (3 * PI / 2, 2 * PI), (0.0, PI), (-PI / 2, PI / 2), (3 * PI / 2, PI / 2), (5.5, 0.7),
               (-2.5, -0.4), (-7.0, -5.2), (7.0, 9.5), (4 * PI + 0.3, 4 * PI + 2.9), (0.3, 0.3 + 3.1415), (0.3, 0.3 + 3.1417), (1.0, 4.5), (2.0, 2.0),
               (0.25, 0.25 + 2 * PI), (-1.0, 6.5), (0.1, 6.2), (PI / 4, 3 * PI / 2)]


def _white():
    img = np.empty((_DOC["rows"], _DOC["cols"], 4), np.uint8)
    img[:] = _DOC["background"]
    return img


def test_fixture_is_the_seven_recorded_arc_cases():
    names = [n for n, _, _ in _GOLDEN]
    assert sorted(names) == sorted(["drawArcQuarter", "drawArcHalf", "drawArcThick", "fillArcQuarter", "fillArcHalf", "fillArcFull", "drawArcSoftThick"])
    assert (_DOC["rows"], _DOC["cols"], _DOC["background"]) == (100, 100, [255, 255, 255, 255])


@pytest.mark.parametrize("name,md5,cmd", _GOLDEN, ids=[n for n, _, _ in _GOLDEN])
def test_restatement_reproduces_reference_md5(name, md5, cmd):
    out = AR.run(_white(), [cmd])
    assert hashlib.md5(out.tobytes()).hexdigest() == md5


def test_both_lowerings_of_mod_agree_on_every_angle_the_suites_use():
    angles = {a for pair in ANGLE_PAIRS for a in pair} | {a for _, _, c in _GOLDEN for a in c["pts"][0]}
    for a in sorted(angles):
        r = float(np.fmod(F(a), AR.TWO_PI))
        assert not (-1e-6 < r < 0), a  # the one interval on which the forms differ
        n0, n1 = AR.normalize(a, form=0), AR.normalize(a, form=1)
        assert n0 == n1 and 0 <= n1 < AR.TWO_PI, (a, n0, n1)
    # and where they do differ, so that the exclusion above is known to matter
    tiny = F(-1e-7)
    assert AR.normalize(tiny, form=0) == AR.TWO_PI and AR.normalize(tiny, form=1) == 0


def test_arc_range_and_segment_counts():
    arc = AR.ArcRange(F(3 * PI / 2), F(PI / 2))  # wraps: end moves up by 2 pi
    assert arc.start < arc.end and abs(float(arc.span()) - PI) < 1e-6
    assert AR.ArcRange(F(0.3), F(0.3 + 3.1417)).is_long() and not AR.ArcRange(F(0.3), F(0.3 + 3.1415)).is_long()
    assert AR.ArcRange(F(2.0), F(2.0)).span() == 0
    quarter = AR.ArcRange(F(0), F(PI / 2))
    assert AR.arc_segments(quarter, F(1.0))[0] == 8 and AR.arc_segments(quarter, F(35.0))[0] == 11  # ceil(54.98 / 5)
    assert AR.arc_segments(AR.ArcRange(F(0), F(PI)), F(400.0))[0] == 200
    # atan2 of the signed zeros decides the axis points of a width-1 fast arc
    assert AR.atan2(F(0.0), -F(0.0)) == AR.PI and AR.atan2(-F(0.0), -F(0.0)) == -AR.PI and AR.atan2(-F(0.0), F(0.0)) == 0


def test_behaviour_the_reference_asserts_for_arcs():
    """src/canvas/tests/arcs.zig: zero and negative radius, NaN and infinite angles draw nothing; the wrap 3 pi / 2 -> pi / 2 is the arc
    -pi / 2 -> pi / 2 on the pixels that test compares (the right side drawn, the left side not)."""
    frame = np.zeros((64, 64, 4), np.uint8)
    red = (255, 0, 0, 255)
    nan, inf = float("nan"), float("inf")
    nothing = [AR.arc((32, 32), 0, 0, PI, red, 1, FAST), AR.arc((32, 32), -5, 0, PI, red, 2, SOFT), AR.fill_arc((32, 32), 0, 0, PI, red, FAST),
               AR.fill_arc((32, 32), -5, 0, PI, red, SOFT), AR.arc((32, 32), 10, 0, PI, red, 0, SOFT)]
    for mode in (FAST, SOFT):
        for a0, a1 in ((nan, PI), (0, nan), (inf, PI), (0, -inf)):
            nothing += [AR.arc((32, 32), 10, a0, a1, red, 1, mode), AR.arc((32, 32), 10, a0, a1, red, 3, mode), AR.fill_arc((32, 32), 10, a0, a1, red, mode)]
    nothing.append(AR.fill_arc((32, 32), 10, 2.0, 2.0, red, FAST))  # fillArcFast: span <= 0
    for cmd in nothing:
        assert AR.run(frame, [cmd]).tobytes() == frame.tobytes(), cmd
    # "arc drawing - angle wrapping": width 2, fast, black on a white Rgb frame; the counts of black pixels differ by less than a tenth
    white = np.full((64, 64, 3), 255, np.uint8)
    black = (0, 0, 0, 255)
    count = lambda a0, a1: int((AR.run(white, [AR.arc((32, 32), 25, a0, a1, black, 2, FAST)]) == 0).all(axis=2).sum())
    n_wrapped, n_plain = count(3 * PI / 2, PI / 2), count(-PI / 2, PI / 2)
    assert n_plain > 100 and abs(n_wrapped - n_plain) < max(n_wrapped, n_plain) // 10
    for mode in (FAST, SOFT):
        wrapped = AR.run(frame, [AR.fill_arc((32, 32), 20, 3 * PI / 2, PI / 2, red, mode)])
        plain = AR.run(frame, [AR.fill_arc((32, 32), 20, -PI / 2, PI / 2, red, mode)])
        for out in (wrapped, plain):
            assert out[32, 42, 0] == 255 and out[32, 22, 0] == 0  # right of the centre drawn, left of it not
        assert wrapped[32, 42].tobytes() == plain[32, 42].tobytes() and wrapped[22, 36].tobytes() == plain[22, 36].tobytes()
    # a span of 2 pi or more is the circle
    full = [AR.arc((32, 32), 12, 0.25, 0.25 + 2 * PI, red, 3, SOFT), AR.fill_arc((32, 32), 12, -1.0, 6.5, red, FAST)]
    assert AR.run(frame, full[:1]).tobytes() == AR.cref.run(frame, [{"kind": 3, "mode": SOFT, "width": 3, "color": red, "p": [32, 32, 12]}]).tobytes()
    assert AR.run(frame, full[1:]).tobytes() == AR.cref.run(frame, [{"kind": 4, "mode": FAST, "width": 1, "color": red, "p": [32, 32, 12]}]).tobytes()


@pytest.mark.parametrize("center,radius", [((16.0, 16.0), 22.0), ((15.5, 16.25), 7.3), ((-6.0, 20.0), 22.0), ((-380.0, 20.0), 400.0), ((20.0, 20.0), 0.4),
                                           ((31.75, 9.5), 1.0)], ids=["corner", "fractional", "off", "far", "r0.4", "r1"])
def test_per_pixel_form_of_fill_arc_fast_equals_the_literal_loops(center, radius):
    """The device does not walk fillArcFast's spans; it asks, per pixel, whether a value of the row's x sequence that belongs to a span lies
    within one pixel (canvas.hip: arc_fill_fast). Restated in AR.arc_fill_fast_gather and held here to the literal loops; the frame's 48
    columns take the x walk across the binades at 1, 2, 4, 8, 16 and 32, where `x += 1` rounds."""
    frame = np.zeros((40, 48), np.uint8)
    white = (255, 255, 255, 255)
    drawn = 0
    for a0, a1 in ANGLE_PAIRS:
        if abs(F(a1) - F(a0)) >= AR.TWO_PI:
            continue
        want = AR.run(frame, [AR.fill_arc(center, radius, a0, a1, white, FAST)])
        got = AR.arc_fill_fast_gather(frame, center, radius, a0, a1, white)
        assert got.tobytes() == want.tobytes(), (a0, a1, int((got != want).sum()))
        drawn += int(want.any())
    assert drawn > 0


def test_walk_to_equals_the_literal_walk():
    for start in (0.0, 0.3, 0.9999999, 1.5, 6.2000003, 15.999999, 31.4, 1000.75):
        v, seq = F(start), []
        while v < 2100:
            seq.append(v)
            v = F(v + F(1.0))
        for target in (-1, 0, 1, 2, 7, 16, 17, 32, 33, 1024, 2049):
            want = next(((x, seq[i - 1] if i else None) for i, x in enumerate(seq) if int(np.trunc(x)) >= target))
            assert AR.walk_to(start, target) == want, (start, target)


def test_packing_round_trips_angles_and_parameters():
    from zignal_amd import _lib as L
    from zignal_amd import canvas

    assert (L.DRAW_ARC, L.DRAW_FILL_ARC) == AR.ARC_KINDS == (16, 17)
    commands = [AR.arc((10.5, 20), 7.25, -PI / 2, 3 * PI, AR.TRANSLUCENT, 3, SOFT), {"kind": 0, "color": (1, 2, 3), "p": [1, 2, 3, 4]},
                AR.cref.quad_bezier((1, 2), (3, 4), (5, 6)), AR.fill_arc((1, 2), 3, 0.5, 0.25, AR.OPAQUE, FAST)]
    cmds, vertices = canvas.pack_commands(commands)
    assert cmds.dtype.itemsize == 40 and vertices.shape == (5, 2) and vertices.dtype == np.float32
    assert list(cmds["kind"]) == [16, 0, 18, 17] and list(cmds["first_vertex"]) == [0, 0, 1, 4] and list(cmds["n_vertices"]) == [1, 0, 3, 1]
    assert list(cmds[0]["p"]) == [10.5, 20, 7.25, 0] and list(cmds[3]["p"]) == [1, 2, 3, 0] and list(cmds["width"]) == [3, 1, 1, 1]
    assert tuple(vertices[0]) == (np.float32(-PI / 2), np.float32(3 * PI)) and tuple(vertices[4]) == (np.float32(0.5), np.float32(0.25))
    assert canvas.has_arcs(cmds) and canvas.has_arcs(commands) and not canvas.has_arcs(cmds[1:3]) and not canvas.has_arcs(commands[1:3])
    cv = canvas.Canvas(np.zeros((4, 4), np.uint8))
    cv.draw_arc((10.5, 20), 7.25, -PI / 2, 3 * PI, AR.TRANSLUCENT, 3, "soft").draw_line((1, 2), (3, 4), (1, 2, 3))
    cv.draw_quadratic_bezier((1, 2), (3, 4), (5, 6), AR.OPAQUE).fill_arc((1, 2), 3, 0.5, 0.25, AR.OPAQUE)
    again, vertices_again = canvas.pack_commands(cv.commands)
    assert again.tobytes() == cmds.tobytes() and vertices_again.tobytes() == vertices.tobytes()


def test_declarations_of_the_arc_kinds_agree():
    """The C header, the ctypes module, the C++ wrapper, the Zig shim and this suite's restatement; the new entry point is declared, bound
    and exported, and the ABI has not moved."""
    from zignal_amd import _lib as L
    import zignal_amd as zg

    header = open(os.path.join(_ROOT, "include", "zignal_hip_canvas.h")).read()
    define = lambda name: int(re.search(r"#define %s\s+(\d+)" % name, header).group(1))
    assert (define("ZG_DRAW_ARC"), define("ZG_DRAW_FILL_ARC")) == (16, 17) == AR.ARC_KINDS == (L.DRAW_ARC, L.DRAW_FILL_ARC)
    assert define("ZG_CANVAS_MAX_CURVE_POINTS") >= 2 * (AR.ARC_MAX_SEGMENTS + 1)  # the soft outline's polygon fits the tables
    assert re.search(r"ZG_API int zg_canvas_draw_arcs\(", header)
    zig = open(os.path.join(_ROOT, "zig", "zignal_hip_canvas.zig")).read()
    for name, value in (("arc", 16), ("fill_arc", 17)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), zig), name
    for name in ("zg_canvas_draw_arcs", "pub fn drawArc", "pub fn fillArc"):
        assert name in zig, name
    hpp = open(os.path.join(_ROOT, "zignal_amd", "cpp", "zignal_hip.hpp")).read()
    for name in ("ZG_DRAW_ARC", "ZG_DRAW_FILL_ARC", "zg_canvas_draw_arcs", "Canvas &drawArc(", "Canvas &fillArc("):
        assert name in hpp, name
    assert zg.lib().zg_canvas_draw_arcs is not None
    assert zg.lib().zg_sizeof_draw_cmd() == 40 and zg.canvas_tile() == 16


def test_host_form_contract_for_arcs_is_checked_before_any_device():
    """An arc carries exactly one vertex, the angle pair; its centre and radius obey the rule for float parameters, its angles do not (the
    non-finite ones draw nothing). What passes goes on to the device, and only a machine without one then answers ZG_ERR_HIP."""
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import canvas

    frame = np.full((20, 20, 4), 7, np.uint8)
    nan, inf = float("nan"), float("inf")
    good = AR.arc((10, 10), 6, 0.5, 2.5, AR.OPAQUE, 2, SOFT)
    fill = AR.fill_arc((10, 10), 6, 0.5, 2.5)
    refused = [dict(good, pts=[]), dict(good, pts=[(0.5, 2.5), (1, 1)]), dict(fill, pts=[]), dict(fill, pts=[(0.5, 2.5), (1, 1)]),
               dict(good, p=[nan, 10, 6]), dict(good, p=[10, inf, 6]), dict(fill, p=[10, 10, nan]), dict(fill, p=[10, 10, inf]), dict(good, p=[10, 10, 70000.0]),
               dict(fill, p=[-70000.0, 10, 6]), dict(good, mode=2), dict(good, width=70000)]
    for bad in refused:
        out = frame.copy()
        with pytest.raises(zg.InvalidArgument):
            canvas.draw_host(out, *canvas.pack_commands([bad]))
        assert out.tobytes() == frame.tobytes(), bad
    cmds, vertices = canvas.pack_commands([good])
    cmds[0]["first_vertex"] = 1  # the angle pair lies outside the array
    with pytest.raises(zg.InvalidArgument):
        canvas.draw_host(frame.copy(), cmds, vertices)
    passes = [good, fill, dict(good, pts=[(nan, 1.0)]), dict(fill, pts=[(0.0, inf)]), dict(good, pts=[(1e30, -1e30)]), dict(fill, pts=[(-70000.0, 70001.0)]),
              dict(good, p=[10, 10, 6, nan]), dict(good, p=[10, 10, -3.0]), dict(good, width=0)]
    for ok in passes:
        try:
            canvas.draw_host(frame.copy(), *canvas.pack_commands([ok]))
        except zg.ZignalError as e:
            assert e.status == L.ERR_HIP, (ok, e)

"""The yardstick of the Canvas curves: tests/canvas_curves_ref.py reproduces the MD5 sums the reference records for its own Bézier and
spline-polygon renderings (src/canvas/tests/regression.zig, kept as data in tests/golden/canvas_curves_md5.json); the packing of a command
that carries points and a parameter round-trips; the declarations of the new constants agree; and the host form's contract check, which
runs before any device is touched, refuses what the header says it refuses."""
from __future__ import annotations

import hashlib
import os
import re

import numpy as np
import pytest

from tests import canvas_curves_ref as CR

_DOC, _GOLDEN = CR.golden_cases()
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _white():
    img = np.empty((_DOC["rows"], _DOC["cols"], 4), np.uint8)
    img[:] = _DOC["background"]
    return img


def test_fixture_is_the_eight_recorded_curve_cases():
    names = [n for n, _, _ in _GOLDEN]
    assert sorted(names) == sorted(["drawBezierCubic", "drawBezierQuadratic", "drawCubicBezierFast", "drawQuadraticBezierFast", "drawSplinePolygon",
                                    "drawSplinePolygonFast", "fillSplinePolygonSoft", "fillSplinePolygonFast"])
    assert (_DOC["rows"], _DOC["cols"], _DOC["background"]) == (100, 100, [255, 255, 255, 255])


@pytest.mark.parametrize("name,md5,cmd", _GOLDEN, ids=[n for n, _, _ in _GOLDEN])
def test_restatement_reproduces_reference_md5(name, md5, cmd):
    out = CR.run(_white(), [cmd])
    assert hashlib.md5(out.tobytes()).hexdigest() == md5


def test_tessellation_counts_at_their_limits():
    """segments = max(min, min(max, trunc(length / pixels per segment))): the clamps and the three per-segment constants."""
    assert CR.segment_count(CR.F(0.0), CR.PPS_QUADRATIC, 3, 200) == 3
    assert CR.segment_count(CR.F(7.99), CR.PPS_QUADRATIC, 3, 200) == 3 and CR.segment_count(CR.F(8.0), CR.PPS_QUADRATIC, 3, 200) == 4
    assert CR.segment_count(CR.F(299.9), CR.PPS_SOFT, 4, 200) == 199 and CR.segment_count(CR.F(300.0), CR.PPS_SOFT, 4, 200) == 200
    assert CR.segment_count(CR.F(1e6), CR.PPS_FAST, 4, 50) == 50
    pts = CR.tessellate(CR.F(30.0), CR.PPS_FAST, 4, 50, CR.eval_cubic, ((CR.F(0), CR.F(0)), (CR.F(10), CR.F(0)), (CR.F(20), CR.F(0)), (CR.F(30), CR.F(0))))
    assert len(pts) == 10 and pts[0] == (0.0, 0.0) and pts[-1] == (30.0, 0.0)  # `segments` points, both ends included


def test_packing_round_trips_points_and_parameters():
    from zignal_amd import _lib as L
    from zignal_amd import canvas

    assert (L.DRAW_QUAD_BEZIER, L.DRAW_CUBIC_BEZIER, L.DRAW_SPLINE_POLYGON, L.DRAW_FILL_SPLINE_POLYGON) == CR.CURVE_KINDS
    commands = [CR.quad_bezier((1, 2), (3.5, 4), (5, 6.25), CR.TRANSLUCENT, 3, CR.SOFT), {"kind": 0, "color": (1, 2, 3), "p": [1, 2, 3, 4]},
                CR.spline_polygon([(1, 1), (9, 2), (5, 8), (2, 6)], CR.OPAQUE, 2, 0.25, CR.FAST), CR.cubic_bezier((0, 0), (1, 5), (6, 5), (7, 0)),
                CR.fill_spline_polygon([(1, 1), (9, 2), (5, 8)], CR.OPAQUE, 1.5, CR.SOFT)]
    cmds, vertices = canvas.pack_commands(commands)
    assert cmds.dtype.itemsize == 40 and vertices.shape == (14, 2) and vertices.dtype == np.float32
    assert list(cmds["kind"]) == [18, 0, 20, 19, 21] and list(cmds["first_vertex"]) == [0, 0, 3, 7, 11] and list(cmds["n_vertices"]) == [3, 0, 4, 4, 3]
    assert list(cmds["mode"]) == [1, 0, 0, 0, 1] and list(cmds["width"]) == [3, 1, 2, 1, 1]
    assert tuple(cmds[0]["color"]) == CR.TRANSLUCENT and tuple(cmds[1]["color"]) == (1, 2, 3, 255)
    assert list(cmds[1]["p"]) == [1, 2, 3, 4] and cmds[2]["p"][0] == np.float32(0.25) and cmds[4]["p"][0] == np.float32(1.5) and list(cmds[0]["p"]) == [0, 0, 0, 0]
    for c, k in zip(commands, range(5)):
        if "pts" in c:
            f, n = int(cmds[k]["first_vertex"]), int(cmds[k]["n_vertices"])
            assert [tuple(v) for v in vertices[f:f + n]] == [tuple(np.float32(q) for q in p) for p in c["pts"]]
    # the Canvas class appends the same commands
    cv = canvas.Canvas(np.zeros((4, 4), np.uint8))
    cv.draw_quadratic_bezier((1, 2), (3.5, 4), (5, 6.25), CR.TRANSLUCENT, 3, "soft").draw_line((1, 2), (3, 4), (1, 2, 3))
    cv.draw_spline_polygon([(1, 1), (9, 2), (5, 8), (2, 6)], CR.OPAQUE, 2, 0.25, "fast").draw_cubic_bezier((0, 0), (1, 5), (6, 5), (7, 0), CR.OPAQUE)
    cv.fill_spline_polygon([(1, 1), (9, 2), (5, 8)], CR.OPAQUE, 1.5, "soft")
    again, vertices_again = canvas.pack_commands(cv.commands)
    assert again.tobytes() == cmds.tobytes() and vertices_again.tobytes() == vertices.tobytes()


def test_declarations_of_the_new_constants_agree():
    """The C header, the ctypes module, the C++ wrapper's use of the header's names, the Zig shim and this suite's restatement."""
    from zignal_amd import _lib as L

    header = open(os.path.join(_ROOT, "include", "zignal_hip_canvas.h")).read()
    define = lambda name: re.search(r"#define %s\s+(\d+)" % name, header).group(1)
    c_kinds = tuple(int(define(n)) for n in ("ZG_DRAW_QUAD_BEZIER", "ZG_DRAW_CUBIC_BEZIER", "ZG_DRAW_SPLINE_POLYGON", "ZG_DRAW_FILL_SPLINE_POLYGON"))
    assert c_kinds == (18, 19, 20, 21) == CR.CURVE_KINDS == (L.DRAW_QUAD_BEZIER, L.DRAW_CUBIC_BEZIER, L.DRAW_SPLINE_POLYGON, L.DRAW_FILL_SPLINE_POLYGON)
    assert int(define("ZG_CANVAS_MAX_CURVE_POINTS")) == 512 == L.CANVAS_MAX_CURVE_POINTS == CR.MAX_CURVE_POINTS
    assert int(define("ZG_CANVAS_MAX_VERTICES")) == 64 == L.CANVAS_MAX_VERTICES
    zig = open(os.path.join(_ROOT, "zig", "zignal_hip_canvas.zig")).read()
    for name, value in (("quad_bezier", 18), ("cubic_bezier", 19), ("spline_polygon", 20), ("fill_spline_polygon", 21)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), zig), name
    assert re.search(r"max_curve_points[^=\n]*=\s*512\b", zig)
    hpp = open(os.path.join(_ROOT, "zignal_amd", "cpp", "zignal_hip.hpp")).read()
    for name in ("ZG_DRAW_QUAD_BEZIER", "ZG_DRAW_CUBIC_BEZIER", "ZG_DRAW_SPLINE_POLYGON", "ZG_DRAW_FILL_SPLINE_POLYGON"):
        assert name in hpp, name
    import zignal_amd as zg
    assert zg.lib().zg_sizeof_draw_cmd() == 40 and zg.canvas_tile() == 16  # the ABI has not moved


def _ring(n, radius, cx=40.0, cy=40.0):
    return [(cx + radius * np.cos(2 * np.pi * k / n), cy + radius * np.sin(2 * np.pi * k / n)) for k in range(n)]


def spline_fill_at_the_bound():
    """(a polygon of 11 long edges whose filled spline is the largest that fits ZG_CANVAS_MAX_CURVE_POINTS, the smallest that does not)."""
    inside = outside = None
    for radius in np.arange(200.0, 320.0, 0.5):
        total = CR.spline_fill_points(_ring(11, radius), 0.5)
        if total <= CR.MAX_CURVE_POINTS:
            inside = (_ring(11, radius), total)
        elif outside is None:
            outside = (_ring(11, radius), total)
    return inside, outside


def test_host_form_contract_is_checked_before_any_device():
    """zg_canvas_draw_host runs cv_check over the whole list first: what is outside the contract is refused here, on a machine with or
    without a device, and the frame is untouched. (What passes the check goes on to the device: tests/test_gpu_canvas_curves.py.)"""
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import canvas

    frame = np.full((20, 20, 4), 7, np.uint8)
    good = CR.cubic_bezier((1, 1), (5, 9), (9, 1), (15, 15))
    nan = float("nan")
    refused = [dict(good, kind=7), dict(good, kind=15), dict(good, kind=16), dict(good, kind=17), dict(good, kind=22), dict(good, mode=2), dict(good, width=70000),
               dict(good, pts=good["pts"][:3]), dict(CR.quad_bezier((1, 1), (5, 9), (9, 1)), pts=good["pts"]), dict(good, pts=[]),
               CR.cubic_bezier((1, 1), (5, nan), (9, 1), (15, 15)), CR.quad_bezier((1, 1), (5, 9), (70000.0, 1)), CR.quad_bezier((1, 1), (float("inf"), 9), (3, 1)),
               CR.spline_polygon([(1, 1), (9, 2), (5, 8)], tension=nan), CR.fill_spline_polygon([(1, 1), (9, 2), (5, 8)], tension=float("inf")),
               CR.fill_spline_polygon([(1, 1), (9, 2), (5, 1e9)]), CR.spline_polygon([(1, 1), (nan, 2), (5, 8)])]
    for bad in refused:
        out = frame.copy()
        with pytest.raises(zg.InvalidArgument):
            canvas.draw_host(out, *canvas.pack_commands([bad]))
        assert out.tobytes() == frame.tobytes(), bad
    cmds, vertices = canvas.pack_commands([good])
    cmds[0]["first_vertex"] = 1  # the range leaves the array
    with pytest.raises(zg.InvalidArgument):
        canvas.draw_host(frame.copy(), cmds, vertices)
    inside, outside = spline_fill_at_the_bound()
    assert inside[1] <= 512 < outside[1] and inside[1] > 500 and outside[1] < 524
    unsupported = [CR.fill_spline_polygon(outside[0]), CR.spline_polygon(_ring(65, 30.0)), CR.fill_spline_polygon(_ring(65, 3.0))]
    for bad in unsupported:
        out = frame.copy()
        with pytest.raises(zg.ZignalError) as e:
            canvas.draw_host(out, *canvas.pack_commands([bad]))
        assert e.value.status == L.ERR_UNSUPPORTED and out.tobytes() == frame.tobytes()
    # inside the contract: the check lets them through (and only a machine without a device then answers ZG_ERR_HIP)
    passes = [good, CR.fill_spline_polygon(inside[0]), CR.spline_polygon(_ring(64, 30.0), width=0), CR.fill_spline_polygon([(1, 1), (2, 2)]),
              CR.spline_polygon([(1, 1), (9, 2), (5, 8)], tension=-3.0), CR.fill_spline_polygon([(1, 1), (9, 2), (5, 8)], tension=65536.0)]
    for ok in passes:
        try:
            canvas.draw_host(frame.copy(), *canvas.pack_commands([ok]))
        except zg.ZignalError as e:
            assert e.status == L.ERR_HIP, (ok, e)

"""The Canvas yardstick itself: tests/canvas_ref.py reproduces the MD5 sums the reference records for its own renderings
(src/canvas/tests/regression.zig, kept as data in tests/golden/canvas_md5.json), and the closed forms the device uses in place of two
sequential recurrences equal the literal walks. The last test runs the same eighteen cases through zg_canvas_draw_host."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

from tests import canvas_cases as cases
from tests import canvas_ref as ref

_DOC, _GOLDEN = cases.golden_cases()


def _white():
    img = np.empty((_DOC["rows"], _DOC["cols"], 4), np.uint8)
    img[:] = _DOC["background"]
    return img


def test_fixture_is_the_eighteen_in_scope_cases():
    names = [n for n, _, _ in _GOLDEN]
    assert len(names) == 18 and len(set(names)) == 18
    assert (_DOC["rows"], _DOC["cols"], _DOC["background"]) == (100, 100, [255, 255, 255, 255])


@pytest.mark.parametrize("name,md5,cmd", _GOLDEN, ids=[n for n, _, _ in _GOLDEN])
def test_restatement_reproduces_reference_md5(name, md5, cmd):
    out = ref.run(_white(), [cmd])
    assert hashlib.md5(out.tobytes()).hexdigest() == md5


def test_bresenham_closed_form_equals_literal_walk():
    """Every (dx, dy) up to 64 in all octants (the horizontal and vertical special cases never reach the general walk), from an origin
    that makes coordinates negative too, and a few long lines."""
    for dx in range(1, 65):
        for dy in range(1, 65):
            for sx in (1, -1):
                for sy in (1, -1):
                    a = (3, -5, 3 + sx * dx, -5 + sy * dy)
                    assert ref.bresenham_line_pixels(*a) == ref.bresenham_line_walk(*a), a
    rng = np.random.default_rng(7)
    for _ in range(40):
        a = tuple(int(v) for v in rng.integers(-70000, 70000, 4))
        if a[0] != a[2] and a[1] != a[3]:
            assert ref.bresenham_line_pixels(*a) == ref.bresenham_line_walk(*a), a


def test_disc_row_closed_form_equals_literal_walk():
    """fillCircleFast's y = top; y += 1 in f32: the binade-at-a-time replay gives the walk's y for every row, None for a row it steps over."""
    F = np.float32
    tops = [F(0), F(0.25), F(0.99999994), F(1.0000001), F(3.7), F(15.999999), F(0.3), F(127.99999), F(1023.4567), F(0.6), F(8191.9995), F(1e-3)]
    rng = np.random.default_rng(11)
    tops += [F(v) for v in rng.uniform(0, 70, 60)] + [F(v) for v in rng.uniform(0, 33000, 20)]
    for top in tops:
        walk, y = {}, F(top)
        for _ in range(300):
            walk[int(np.trunc(y))] = y
            y = F(y + F(1))
        first, last = int(np.trunc(top)), max(walk)
        for row in range(max(0, first - 1), last + 1):
            got = ref.disc_row_y(top, row)
            want = walk.get(row)
            assert (got is None and want is None) or (got is not None and want is not None and F(got) == F(want)), (top, row, got, want)


def test_module_header_bindings_and_struct_size():
    """The Canvas module's header is pulled in by zignal_hip.h after the quantisation module's, the library exports every symbol the
    binding table names, and the three declarations of zg_draw_cmd (C, ctypes, numpy) have one size."""
    import ctypes as C
    import os
    import re

    import zignal_amd as zg
    from zignal_amd import _lib as L

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_quantize.h"') < main.index('#include "zignal_hip_canvas.h"')
    header = open(os.path.join(root, "include", "zignal_hip_canvas.h")).read()
    declared = set(re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(", header))
    assert declared == set(L.CANVAS_EXPORTED_SYMBOLS)
    lib = zg.lib()
    for name in L.CANVAS_EXPORTED_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.zg_sizeof_draw_cmd() == C.sizeof(L.ZgDrawCmd) == zg.DRAW_CMD_DTYPE.itemsize == 40
    assert zg.canvas_tile() == 16


@pytest.mark.gpu
@pytest.mark.parametrize("name,md5,cmd", _GOLDEN, ids=[n for n, _, _ in _GOLDEN])
def test_host_form_reproduces_reference_md5(name, md5, cmd):
    import zignal_amd as zg
    from zignal_amd import canvas

    out = _white()
    cmds, vertices = canvas.pack_commands([cmd])
    canvas.draw_host(out, cmds, vertices)
    assert hashlib.md5(out.tobytes()).hexdigest() == md5
    assert zg is not None

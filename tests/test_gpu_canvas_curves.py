"""The Canvas curves on the device — quadratic and cubic Béziers, spline polygons drawn and filled — against tests/canvas_curves_ref.py (the
reference's calls made one after another), byte for byte: the reference's own recorded MD5 sums through both forms, every new kind, mode,
width, colour and pixel type, frames where tiling and clipping can go wrong, the tessellation limits and the bound on a filled spline
polygon, order against the old kinds, a seeded random list over all kinds, views, the contract, the count word and a captured graph."""
import hashlib

import numpy as np
import pytest

import zignal_amd as zg
from tests import canvas_cases as K
from tests import canvas_curves_ref as CR
from tests.test_canvas_curves_oracle import _ring, spline_fill_at_the_bound
from tests.test_gpu_canvas import PIXELS, T, background, on_device, same_bytes
from zignal_amd import canvas

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FAST, SOFT = CR.FAST, CR.SOFT
_DOC, _GOLDEN = CR.golden_cases()


def check(host, commands, what):
    want = CR.run(host, commands)
    got = on_device(host, commands)
    if not same_bytes(got, want):
        bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first (row, col) {tuple(bad[0])}: device {got[tuple(bad[0])]}, reference {want[tuple(bad[0])]}")
    return want


def every_curve(width, mode, color, rows, cols):
    """One command of every new kind, sized to the frame: each crosses several tile borders and the others."""
    w, h = float(cols), float(rows)
    hexagon = [(0.5 * w, 0.12 * h), (0.86 * w, 0.3 * h), (0.9 * w, 0.7 * h), (0.5 * w, 0.9 * h), (0.15 * w, 0.72 * h), (0.1 * w, 0.3 * h)]
    return [CR.fill_spline_polygon(hexagon, color, 0.5, mode),
            CR.quad_bezier((0.1 * w, 0.85 * h), (0.5 * w + 0.25, -0.2 * h), (0.92 * w, 0.8 * h), color, width, mode),
            CR.cubic_bezier((0.05 * w, 0.5 * h), (0.3 * w, 0.02 * h), (0.7 * w, 0.98 * h), (0.95 * w, 0.45 * h + 0.5), color, width, mode),
            CR.spline_polygon([(0.3 * w, 0.2 * h), (0.8 * w, 0.25 * h), (0.7 * w, 0.8 * h), (0.2 * w, 0.75 * h)], color, width, 0.3, mode)]


# ---- the reference's own renderings ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,md5,cmd", _GOLDEN, ids=[n for n, _, _ in _GOLDEN])
def test_host_and_device_forms_reproduce_reference_md5(name, md5, cmd):
    white = np.empty((_DOC["rows"], _DOC["cols"], 4), np.uint8)
    white[:] = _DOC["background"]
    out = white.copy()
    canvas.draw_host(out, *canvas.pack_commands([cmd]))
    assert hashlib.md5(out.tobytes()).hexdigest() == md5
    assert hashlib.md5(on_device(white, [cmd]).tobytes()).hexdigest() == md5


# ---- every new kind x mode x width x colour x pixel type --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("color", [CR.OPAQUE, CR.TRANSLUCENT], ids=["opaque", "a128"])
@pytest.mark.parametrize("width", [1, 2, 5])
@pytest.mark.parametrize("mode", [FAST, SOFT], ids=["fast", "soft"])
def test_every_curve_kind_equals_the_reference(mode, width, color):
    commands = every_curve(width, mode, color, 40, 48)
    for pixel in PIXELS:
        host = background(40, 48, pixel)
        for k, cmd in enumerate(commands):
            want = check(host, [cmd], (pixel, k, mode, width))
            assert not same_bytes(want, host), (pixel, k)
        check(host, commands, (pixel, mode, width))


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(T + 1, T + 1), (1, 3 * T + 5), (2 * T + 7, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_borders_and_degenerate_frames(shape):
    rows, cols = shape
    w, h = float(cols), float(rows)
    Tr = CR.TRANSLUCENT
    commands = every_curve(2, SOFT, Tr, rows, cols) + every_curve(5, FAST, CR.OPAQUE, rows, cols) + every_curve(1, FAST, Tr, rows, cols) \
        + every_curve(1, SOFT, Tr, rows, cols)
    # a control point on the tile corner, curves that end on it, and a spline polygon round it
    commands += [CR.cubic_bezier((T - 3.0, T - 9.0), (float(T), float(T)), (T + 6.0, T - 2.0), (float(T), T + 7.5), Tr, 1, SOFT),
                 CR.quad_bezier((0.0, 0.0), (T - 0.5, 2.0), (float(T), float(T)), CR.OPAQUE, 1, FAST),
                 CR.fill_spline_polygon([(T - 4.0, T - 5.0), (T + 5.0, T - 3.5), (T + 3.0, T + 6.0), (T - 6.0, T + 4.0)], Tr, 0.5, SOFT)]
    # wholly outside the frame
    commands += [CR.cubic_bezier((w + 20, -30), (w + 60, 5), (w + 35, 40), (w + 90, h + 8), CR.OPAQUE, wd, m) for wd in (1, 3) for m in (FAST, SOFT)]
    commands += [CR.quad_bezier((-50, -10), (-20, -40), (-8, -6), CR.OPAQUE, 2, SOFT), CR.fill_spline_polygon([(-40, -40), (-10, -35), (-20, -8)], CR.OPAQUE, 0.5, FAST),
                 CR.spline_polygon([(w + 9, h + 9), (w + 40, h + 12), (w + 20, h + 50)], CR.OPAQUE, 2, 0.5, SOFT)]
    for pixel in PIXELS:
        check(background(rows, cols, pixel, 2), commands, (shape, pixel))
    # reaching in from 60 000 away: 200 segments of 300 pixels and more each, one or two of which cross the frame
    far = [CR.cubic_bezier((-60000.0, 0.4 * h), (-20000.0, 0.5 * h), (20000.0, 0.6 * h), (60000.0, 0.45 * h), Tr, 1, SOFT),
           CR.quad_bezier((0.5 * w, -60000.0), (0.3 * w, 0.0), (0.6 * w, 60000.0), CR.OPAQUE, 3, FAST),
           CR.fill_spline_polygon([(-60000.0, -100.0), (0.5 * w, 0.25 * h), (60000.0, -90.0), (0.4 * w, 0.8 * h)], Tr, 0.5, SOFT)]
    host = background(rows, cols, "rgba_u8", 2)
    assert not same_bytes(check(host, far, (shape, "far")), host)


# ---- tessellation limits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tessellation_limits():
    host = background(80, 96, "rgba_u8", 7)
    Tr = CR.TRANSLUCENT
    short_quad, short_cubic = ((40.0, 40.0), (41.0, 42.5), (43.0, 40.5)), ((10.0, 10.0), (10.5, 11.0), (11.5, 9.5), (12.0, 10.5))
    long_quad, long_cubic = ((2.0, 70.0), (48.0, -330.0), (93.0, 72.0)), ((3.0, 5.0), (300.0, 60.0), (-200.0, 20.0), (90.0, 75.0))
    P = lambda pts: [tuple(CR.F(v) for v in p) for p in pts]
    assert CR.segment_count(CR.quadratic_length(*P(short_quad)), CR.PPS_QUADRATIC, 3, 200) == 3
    assert CR.segment_count(CR.cubic_length(*P(short_cubic)), CR.PPS_SOFT, 4, 200) == 4
    assert CR.quadratic_length(*P(long_quad)) / CR.PPS_QUADRATIC > 201 and CR.cubic_length(*P(long_cubic)) / CR.PPS_FAST > 201
    for width, mode in ((1, FAST), (1, SOFT), (2, FAST), (3, FAST), (4, SOFT)):  # cubic: 3 pixels a segment for fast widths 1 and 2, else 1.5
        for pts in (short_quad, long_quad):
            check(host, [CR.quad_bezier(*pts, Tr, width, mode)], ("quad", pts, width, mode))
        for pts in (short_cubic, long_cubic):
            check(host, [CR.cubic_bezier(*pts, Tr, width, mode)], ("cubic", pts, width, mode))
    # a cubic whose estimate sits between the two constants' thresholds: 199 segments or 100
    between = ((3.0, 40.0), (60.0, -30.0), (40.0, 110.0), (93.0, 38.0))
    n_soft, n_fast = (CR.segment_count(CR.cubic_length(*P(between)), pps, 4, 200) for pps in (CR.PPS_SOFT, CR.PPS_FAST))
    assert 4 < n_fast < n_soft < 200
    check(host, [CR.cubic_bezier(*between, Tr, 2, FAST), CR.cubic_bezier(*between, Tr, 3, FAST), CR.cubic_bezier(*between, Tr, 2, SOFT)], "between")
    # tension below 0, between 0 and 1, above 1; width 0, two vertices, zero-length edges
    square = [(20.0, 15.0), (75.0, 20.0), (70.0, 65.0), (15.0, 60.0)]
    for tension in (-2.0, 0.0, 0.35, 1.0, 7.5):
        want = check(host, [CR.fill_spline_polygon(square, Tr, tension, SOFT), CR.spline_polygon(square, CR.OPAQUE, 2, tension, FAST)], tension)
        assert not same_bytes(want, host)
    assert same_bytes(check(host, [CR.fill_spline_polygon(square, Tr, -2.0, FAST)], "clamped"), CR.run(host, [CR.fill_spline_polygon(square, Tr, 0.0, FAST)]))
    nothing = [CR.spline_polygon(square, Tr, 0, 0.5, SOFT), CR.spline_polygon(square[:2], Tr, 2, 0.5, SOFT), CR.fill_spline_polygon(square[:2], Tr, 0.5, SOFT),
               CR.quad_bezier((1, 1), (30, 30), (50, 2), Tr, 0, SOFT), CR.cubic_bezier((1, 1), (30, 30), (50, 2), (60, 60), Tr, 0, FAST)]
    assert same_bytes(check(host, nothing, "nothing drawn"), host)
    point = [CR.cubic_bezier((30.5, 30.5), (30.5, 30.5), (30.5, 30.5), (30.5, 30.5), Tr, wd, m) for wd in (1, 3) for m in (FAST, SOFT)] \
        + [CR.fill_spline_polygon([(50.0, 50.0)] * 3, Tr, 0.5, SOFT), CR.spline_polygon([(60.0, 20.0), (60.0, 20.0), (70.0, 30.0)], Tr, 2, 0.5, SOFT)]
    for k, cmd in enumerate(point):
        check(host, [cmd], ("degenerate", k))


@pytest.mark.gpu
def test_filled_spline_polygon_at_the_bound_on_its_points():
    """The largest filled spline polygon that fits ZG_CANVAS_MAX_CURVE_POINTS is drawn and equals the restatement; the smallest that does
    not is skipped on the device and refused as unsupported by the host form. 64 vertices are taken, 65 are not."""
    host = background(80, 80, "rgba_u8", 8)
    (inside, n_inside), (outside, n_outside) = spline_fill_at_the_bound()
    assert 500 < n_inside <= CR.MAX_CURVE_POINTS < n_outside
    for mode in (FAST, SOFT):
        want = check(host, [CR.fill_spline_polygon(inside, CR.TRANSLUCENT, 0.5, mode)], ("inside", mode))
        assert not same_bytes(want, host)
        assert same_bytes(on_device(host, [CR.fill_spline_polygon(outside, CR.TRANSLUCENT, 0.5, mode)]), host)
    out = host.copy()
    with pytest.raises(zg.ZignalError) as e:
        canvas.draw_host(out, *canvas.pack_commands([CR.fill_spline_polygon(outside)]))
    assert e.value.status == 5 and same_bytes(out, host)  # ZG_ERR_UNSUPPORTED
    ring64 = _ring(64, 30.0)
    assert CR.spline_fill_points(ring64, 0.5) == 256  # 64 edges at the minimum of 4 points
    check(host, [CR.fill_spline_polygon(ring64, CR.TRANSLUCENT, 0.5, SOFT), CR.spline_polygon(ring64, CR.OPAQUE, 2, 0.5, SOFT)], "64 vertices")
    for cmd in (CR.fill_spline_polygon(_ring(65, 30.0)), CR.spline_polygon(_ring(65, 30.0))):
        assert same_bytes(on_device(host, [cmd]), host)
        with pytest.raises(zg.ZignalError) as e:
            canvas.draw_host(host.copy(), *canvas.pack_commands([cmd]))
        assert e.value.status == 5
    big = K.fill_polygon([(float(i), float(i * i % 7)) for i in range(65)])  # user polygons keep their bound of 64
    assert same_bytes(on_device(host, [big]), host)


# ---- order --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_curves_and_old_kinds_compose_in_list_order():
    host = background(64, 72, "rgba_u8", 9)
    commands = [CR.fill_spline_polygon([(10, 8), (60, 12), (55, 55), (12, 50)], (255, 0, 0, 128), 0.5, SOFT), K.fill_circle(40, 30, 18, (0, 0, 255, 128), SOFT),
                CR.cubic_bezier((2, 30), (30, -10), (40, 70), (70, 28), (0, 255, 0, 128), 5, SOFT), K.line(5, 5, 66, 58, (255, 255, 0, 128), 4, SOFT),
                CR.quad_bezier((5, 60), (36, -20), (68, 60), (255, 0, 255, 128), 3, SOFT), K.fill_rect(20, 20, 50, 45, (0, 255, 255, 128), SOFT),
                CR.spline_polygon([(20, 10), (60, 30), (30, 58)], (30, 30, 30, 128), 2, 0.2, SOFT),
                K.circle(30, 30, 15, (0, 90, 200, 128), 3, SOFT)]
    forward, backward = check(host, commands, "forward"), check(host, commands[::-1], "backward")
    assert not same_bytes(forward, backward)
    # a Bézier's own segments overlap at their joints and a self-crossing curve crosses itself: blended as often as the reference blends
    loop = CR.cubic_bezier((10, 50), (90, 5), (-20, 5), (60, 50), (200, 40, 40, 128), 4, SOFT)
    check(host, [loop, dict(loop, width=1), dict(loop, width=2, mode=FAST)], "self-crossing")


# ---- a seeded random list -----------------------------------------------------------------------------------------------------------------
def random_commands(n, rows, cols, seed):
    """n commands over the seven old kinds and the four curves with heavy overlap."""
    rng = np.random.default_rng(seed)
    old = K.random_commands(n, rows, cols, seed)
    out = []
    for k in range(n):
        kind = int(rng.integers(0, 11))
        if kind < 7:
            out.append(old[k])
            continue
        mode, width = int(rng.integers(0, 2)), int(rng.choice([1, 1, 2, 3, 5]))
        color = tuple(int(v) for v in rng.integers(0, 256, 3)) + (255 if rng.random() < 0.5 else int(rng.integers(0, 255)),)
        x, y, s = float(rng.uniform(-6, cols + 6)), float(rng.uniform(-6, rows + 6)), float(rng.uniform(4, 30))
        pts = [(float(np.float32(x + dx)), float(np.float32(y + dy))) for dx, dy in rng.uniform(-s, s, (6, 2))]
        tension = float(np.float32(rng.uniform(-0.3, 1.3)))
        out.append([CR.quad_bezier(*pts[:3], color, width, mode), CR.cubic_bezier(*pts[:4], color, width, mode),
                    CR.spline_polygon(pts[:int(rng.integers(3, 7))], color, width, tension, mode),
                    CR.fill_spline_polygon(pts[:int(rng.integers(3, 7))], color, tension, mode)][kind - 7])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", PIXELS)
def test_a_random_list_over_all_kinds_with_heavy_overlap(pixel):
    rows, cols = 80, 96
    commands = random_commands(150, rows, cols, 20261020)
    assert {c["kind"] for c in commands} == set(range(7)) | set(CR.CURVE_KINDS)
    check(background(rows, cols, pixel, 4), commands, pixel)


# ---- views ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_views_of_a_wider_tensor_leave_their_surroundings_alone():
    rows, cols = T + 3, 2 * T + 1
    commands = every_curve(2, SOFT, CR.TRANSLUCENT, rows, cols) + every_curve(3, FAST, CR.OPAQUE, rows, cols)
    cmds, vertices = canvas.pack_commands(commands)
    dcmds, dverts = torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), torch.from_numpy(vertices).cuda()
    for pixel in PIXELS:
        inner = background(rows, cols, pixel, 5)
        wide = np.full((rows + 6, cols + 11) + inner.shape[2:], 0xA5, np.uint8)
        wide[2:2 + rows, 4:4 + cols] = inner
        dev = torch.from_numpy(wide).cuda()
        canvas.draw(dev[2:2 + rows, 4:4 + cols], dcmds, vertices=dverts)
        expect = wide.copy()
        expect[2:2 + rows, 4:4 + cols] = CR.run(inner, commands)
        assert same_bytes(dev.cpu().numpy(), expect), pixel


# ---- the contract and the count word ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_commands_outside_the_contract_are_skipped_on_the_device_and_refused_by_the_host_form():
    host = background(40, 40, "rgb_u8")
    good = [CR.fill_spline_polygon([(5, 5), (35, 8), (30, 33), (8, 30)], CR.TRANSLUCENT, 0.5, SOFT), CR.cubic_bezier((2, 3), (20, 38), (25, 1), (37, 30), CR.OPAQUE, 2, FAST)]
    nan = float("nan")
    bezier = CR.cubic_bezier((1, 1), (9, 30), (20, 2), (30, 30))
    bad = [dict(bezier, kind=7), dict(bezier, kind=16), dict(bezier, kind=17), dict(bezier, kind=22), dict(bezier, pts=bezier["pts"][:3]),
           dict(CR.quad_bezier((1, 1), (9, 30), (20, 2)), pts=bezier["pts"]), dict(bezier, pts=[]), CR.cubic_bezier((1, 1), (9, nan), (20, 2), (30, 30)),
           CR.quad_bezier((1, 1), (9, 30), (1e9, 2)), CR.spline_polygon([(1, 1), (30, 2), (9, 30)], tension=nan),
           CR.fill_spline_polygon([(1, 1), (30, 2), (9, 30)], tension=1e9), dict(bezier, mode=2), dict(bezier, width=70000)]
    want = CR.run(host, good)
    for b in bad:
        assert same_bytes(on_device(host, [good[0], b, good[1]]), want), b
        out = host.copy()
        with pytest.raises(zg.InvalidArgument):
            canvas.draw_host(out, *canvas.pack_commands([good[0], b, good[1]]))
        assert same_bytes(out, host)
    cmds, vertices = canvas.pack_commands([bezier])
    cmds[0]["first_vertex"] = 1  # the range leaves the array
    dev = torch.from_numpy(host.copy()).cuda()
    canvas.draw(dev, torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), vertices=torch.from_numpy(vertices).cuda())
    assert same_bytes(dev.cpu().numpy(), host)


@pytest.mark.gpu
def test_count_word_shorter_than_the_list_draws_the_prefix():
    host = background(40, 48, "rgba_u8")
    commands = every_curve(2, SOFT, CR.TRANSLUCENT, 40, 48)
    word = lambda v: torch.tensor([v, 12345], dtype=torch.int32, device="cuda")
    assert same_bytes(on_device(host, commands, word(0)), host)
    assert same_bytes(on_device(host, commands, word(3)), CR.run(host, commands[:3]))
    assert same_bytes(on_device(host, commands, word(99)), CR.run(host, commands))


@pytest.mark.gpu
def test_the_canvas_class_draws_curves_on_device_and_host_images():
    host = background(40, 48, "rgba_u8")
    commands = every_curve(2, SOFT, CR.TRANSLUCENT, 40, 48)
    want = CR.run(host, commands)
    for image in (torch.from_numpy(host.copy()).cuda(), host.copy()):
        cv = zg.Canvas(image)
        cv.fill_spline_polygon(commands[0]["pts"], CR.TRANSLUCENT, 0.5, "soft").draw_quadratic_bezier(*commands[1]["pts"], CR.TRANSLUCENT, 2, "soft")
        cv.draw_cubic_bezier(*commands[2]["pts"], CR.TRANSLUCENT, 2, "soft").draw_spline_polygon(commands[3]["pts"], CR.TRANSLUCENT, 2, 0.3, "soft")
        cv.flush()
        assert same_bytes(zg.Image(image).to_numpy(), want)


# ---- a captured graph -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_draw_replays_from_a_graph_on_a_changed_command_buffer_and_frame():
    rows, cols, n = 2 * T + 5, 3 * T + 1, 40
    lists = [random_commands(n, rows, cols, seed) for seed in (301, 302, 303)]
    frame = torch.zeros((rows, cols, 4), dtype=torch.uint8, device="cuda")
    dcmds = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    dverts = torch.zeros((n * 8, 2), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")

    def load(k, how_many):
        host = background(rows, cols, "rgba_u8", 10 + k)
        cmds, vertices = canvas.pack_commands(lists[k])
        frame.copy_(torch.from_numpy(host))
        dcmds.copy_(torch.from_numpy(cmds.view(np.uint8).copy()))
        dverts.zero_()
        dverts[:len(vertices)].copy_(torch.from_numpy(vertices))
        count.fill_(how_many)
        return CR.run(host, lists[k][:how_many])

    side = torch.cuda.Stream()
    load(0, n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        canvas.draw(frame, dcmds, count=count, vertices=dverts)
    for k, how_many in ((0, n), (1, n), (2, 17)):
        want = load(k, how_many)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(frame.cpu().numpy(), want), (k, how_many)
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0

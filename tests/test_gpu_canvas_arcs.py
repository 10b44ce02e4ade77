"""drawArc and fillArc on the device — zg_canvas_draw_arcs and the host form — against tests/canvas_arcs_ref.py (the reference's calls made
one after another), byte for byte: the reference's own recorded MD5 sums through both forms; every route (the gated Bresenham circle and
ring, the soft outline as Wu lines and as one polygon, the fast fill's spans, the soft fill's coverage) on every pixel type, colour, mode
and width; centres on a tile corner, between pixels, off the frame and far off it; radii from one that rounds to 0 up; angle pairs on the
axes, wrapped, negative, above 2 pi, either side of pi, empty and full; order against every other kind; the chunk boundary, the count
word, a view, the contract, the old entry point, a captured graph and the Canvas class."""
import hashlib
import math

import numpy as np
import pytest

import zignal_amd as zg
from tests import canvas_arcs_ref as AR
from tests import canvas_cases as K
from tests import canvas_curves_ref as CR
from tests.test_canvas_arcs_oracle import ANGLE_PAIRS
from tests.test_gpu_canvas import PIXELS, T, background, same_bytes
from zignal_amd import canvas

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FAST, SOFT = AR.FAST, AR.SOFT
PI = math.pi
_DOC, _GOLDEN = AR.golden_cases()
ROWS, COLS = 40, 48  # three tiles each way, the last one partial
# (what, width, mode) of the six routes
ROUTES = [("arc", 1, FAST), ("arc", 3, FAST), ("arc", 1, SOFT), ("arc", 4, SOFT), ("fill", 1, FAST), ("fill", 1, SOFT)]
ROUTE_IDS = ["bresenham", "ring", "wu-lines", "polygon", "fill-fast", "fill-soft"]


def make(route, center, radius, a0, a1, color):
    what, width, mode = route
    return AR.arc(center, radius, a0, a1, color, width, mode) if what == "arc" else AR.fill_arc(center, radius, a0, a1, color, mode)


def on_device(host, commands, count=None, n=None, arcs=True):
    """zg_canvas_draw_arcs (arcs=False: zg_canvas_draw) of `commands` into a device copy of `host`; returns the frame."""
    cmds, vertices = canvas.pack_commands(commands)
    dverts = torch.from_numpy(vertices).cuda() if len(vertices) else None
    return K.on_device(host, cmds, lambda dev, dcmds: canvas.draw(dev, dcmds, count=count, vertices=dverts, n=len(cmds) if n is None else n, arcs=arcs))


def on_host(host, commands):
    return K.on_host(host, canvas.draw_host, *canvas.pack_commands(commands))


def check(host, commands, what, host_form=False):
    """The device form (and, asked for, the host form) equals the restatement. Both fail on a library without arcs: there the device
    skips them and the host form refuses them."""
    forms = [("zg_canvas_draw_arcs", lambda: on_device(host, commands))] + [("zg_canvas_draw_host", lambda: on_host(host, commands))] * host_form
    return K.check(AR.run(host, commands), what, *forms)


# ---- the reference's own renderings ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,md5,cmd", _GOLDEN, ids=[n for n, _, _ in _GOLDEN])
def test_host_and_device_forms_reproduce_reference_md5(name, md5, cmd):
    white = np.empty((_DOC["rows"], _DOC["cols"], 4), np.uint8)
    white[:] = _DOC["background"]
    assert hashlib.md5(on_host(white, [cmd]).tobytes()).hexdigest() == md5
    assert hashlib.md5(on_device(white, [cmd]).tobytes()).hexdigest() == md5


# ---- every route x colour x pixel type, over the centres and radii ------------------------------------------------------------------------
PLACES = [((16.0, 16.0), 22.0), ((16.0, 16.0), 7.3), ((15.5, 16.25), 7.3), ((15.5, 16.25), 22.0), ((-6.0, 20.0), 22.0), ((24.0, 20.0), 1.0), ((33.25, 9.5), 1.0),
          ((30.0, 10.0), 0.4), ((17.5, 30.5), 0.4)]
PLACE_ANGLES = [(0.0, PI / 2), (3 * PI / 2, PI / 2), (-2.5, -0.4), (0.3, 0.3 + 3.1417), (1.0, 4.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("color", [AR.OPAQUE, AR.TRANSLUCENT], ids=["opaque", "a128"])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_every_route_equals_the_reference(route, color):
    commands = [make(route, center, radius, *PLACE_ANGLES[(k + j) % len(PLACE_ANGLES)], color) for k, (center, radius) in enumerate(PLACES) for j in (0, 2)]
    drawn = 0
    for k, cmd in enumerate(commands):  # each on its own, so that none hides behind a later one; both forms
        host = background(ROWS, COLS, PIXELS[k % 3], 1 + k % 2)
        drawn += not same_bytes(check(host, [cmd], (route, k, cmd["p"], cmd["pts"]), host_form=k % 4 == 0), host)
    assert drawn >= len(commands) // 2
    for pixel in PIXELS:
        check(background(ROWS, COLS, pixel), commands, (route, pixel), host_form=True)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 2, 5])
@pytest.mark.parametrize("mode", [FAST, SOFT], ids=["fast", "soft"])
def test_widths_1_2_and_5(mode, width):
    for pixel in PIXELS:
        host = background(ROWS, COLS, pixel, 3)
        for color in (AR.OPAQUE, AR.TRANSLUCENT):
            commands = [AR.arc((16.0, 16.0), 13.0, PI / 4, 3 * PI / 2, color, width, mode), AR.arc((15.5, 16.25), 22.0, 5.5, 0.7, color, width, mode),
                        AR.arc((30.0, 30.0), 2.0, -1.0, 2.0, color, width, mode)]
            assert not same_bytes(check(host, commands, (pixel, mode, width, color)), host)


# ---- angle pairs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_angle_pairs(route):
    """Exact multiples of pi / 2 (the inclusive comparisons on axis pixels and the signed zeros), wraps, negative angles, both above 2 pi,
    spans either side of pi (union against intersection of the half-planes), start == end, and spans at and above 2 pi (the circle)."""
    host = background(ROWS, COLS, "rgba_u8", 4)
    for k, (a0, a1) in enumerate(ANGLE_PAIRS):
        for center, radius in (((16.0, 16.0), 13.0), ((24.5, 19.75), 9.3)):
            check(host, [make(route, center, radius, a0, a1, AR.TRANSLUCENT)], (route, a0, a1, center), host_form=k % 5 == 0)
    quadrants = [make(route, (16.0, 16.0), 12.0, q * PI / 2, (q + 1) * PI / 2, (60 * q + 40, 200 - 50 * q, 90, 128)) for q in range(4)]
    check(host, quadrants, (route, "quadrants"))  # neighbours share their axis pixels: blended twice where the reference blends twice


@pytest.mark.gpu
def test_an_arc_that_reaches_the_frame_from_far_away():
    """Centre (-380, 20), radius 400, span pi: a sliver is visible; 200 segments (the cap) of 6 pixels each, and the 402-point polygon."""
    center, radius = (-380.0, 20.0), 400.0
    arc = AR.ArcRange(AR.F(-PI / 2), AR.F(PI / 2))
    assert AR.arc_segments(arc, AR.F(radius))[0] == AR.ARC_MAX_SEGMENTS and 2 * (AR.ARC_MAX_SEGMENTS + 1) == 402
    for k, route in enumerate(ROUTES):
        host = background(ROWS, COLS, PIXELS[k % 3], 5)
        for a0, a1 in ((-PI / 2, PI / 2), (-0.2, 0.1), (6.2, 6.2 + 3.1417)):
            want = check(host, [make(route, center, radius, a0, a1, AR.TRANSLUCENT)], (route, a0, a1), host_form=True)
            assert not same_bytes(want, host), (route, a0, a1)
    host = background(ROWS, COLS, "rgba_u8", 5)
    big = [make(route, (24.0, -3000.0), 3020.5, 1.2, 1.9, AR.TRANSLUCENT) for route in ROUTES]  # the x walk of a row starts at 0, the y walk too
    for cmd in big:
        assert not same_bytes(check(host, [cmd], ("3020", cmd["kind"], cmd["mode"], cmd["width"])), host)


@pytest.mark.gpu
def test_a_soft_thick_arc_of_a_very_large_radius_whose_chords_sag_into_the_frame():
    """The soft outline of width > 1 is a polygon whose inner edge is 200 chords of the circle of radius r - w / 2. At a radius of tens
    of thousands and a span near 2 pi a chord's middle lies pixels inside that circle (r span^2 / 320000: 7.8 at 65 000), so the
    reference writes into tiles that lie wholly inside the ring r -+ (w / 2 + 3): a tile test that took the polygon for its ring would
    leave them out. The frame sits on the middle of a chord; every parameter is within ZG_CANVAS_MAX_COORD."""
    rows, cols, a0, a1 = 64, 80, 0.05, 6.25
    exposed = 0
    for radius, width, chord in ((65000.0, 2, 100), (65000.0, 3, 37), (40000.0, 2, 100), (20000.0, 6, 163)):
        theta = a0 + (chord + 0.5) * (a1 - a0) / 200
        center = (float(np.float32(cols / 2 - radius * math.cos(theta))), float(np.float32(rows / 2 - radius * math.sin(theta))))
        assert max(abs(center[0]), abs(center[1]), radius) <= 65536.0
        host = background(rows, cols, "rgba_u8", 11)
        cmd = AR.arc(center, radius, a0, a1, AR.TRANSLUCENT, width, SOFT)
        want = check(host, [cmd], (radius, width, chord), host_form=True)
        written = np.argwhere((want != host).any(axis=2))
        assert len(written) > 100
        # pixels in tiles whose farthest pixel is still inside the ring's inner edge less the roundings' 3 pixels
        inside = [1 for y, x in written if math.hypot(x // T * T + 7.5 - center[0], y // T * T + 7.5 - center[1]) + 11.4 < radius - (width / 2 + 3)]
        exposed += len(inside)
    assert exposed > 0  # at least one of the cases writes where the ring is not
    # the same arc seen from its start: the first chords, centre far to the upper left
    host = background(rows, cols, "rgba_u8", 12)
    check(host, [AR.arc((-64850.0, -4200.0), 65000.0, a0, a1, AR.TRANSLUCENT, 2, SOFT), AR.arc((-64850.0, -4200.0), 65000.0, a0, a1, AR.OPAQUE, 1, SOFT),
                 AR.arc((-64850.0, -4200.0), 65000.0, a0, a1, AR.TRANSLUCENT, 3, FAST)], "r 65000 from its start", host_form=True)


# ---- order --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_arcs_and_every_other_kind_compose_in_list_order():
    host = background(64, 72, "rgba_u8", 9)
    A = lambda c: c + (128,)
    commands = [AR.fill_arc((36, 30), 24, 0.4, 4.0, A((255, 0, 0)), SOFT), K.fill_circle(40, 30, 18, A((0, 0, 255)), SOFT),
                AR.arc((30, 34), 20, -1.0, 2.2, A((0, 255, 0)), 5, SOFT), K.line(5, 5, 66, 58, A((255, 255, 0)), 4, SOFT),
                AR.fill_arc((30, 30), 22, 3.0, 1.0, A((255, 0, 255)), FAST), K.fill_rect(20, 20, 50, 45, A((0, 255, 255)), SOFT),
                AR.arc((40, 28), 17, 0.0, 5.0, A((30, 30, 30)), 1, SOFT), K.circle(30, 30, 15, A((0, 90, 200)), 3, SOFT),
                AR.arc((36, 32), 19, 2.0, 0.5, A((200, 90, 0)), 1, FAST), K.rect(10, 12, 60, 50, A((90, 0, 200)), 2, SOFT),
                AR.arc((34, 30), 21, 1.0, 6.0, A((9, 200, 90)), 4, FAST), K.polygon([(8, 8), (60, 14), (40, 56)], A((120, 120, 0)), 2, SOFT),
                K.fill_polygon([(20, 10), (60, 30), (30, 58)], A((0, 120, 120)), SOFT), CR.cubic_bezier((2, 30), (30, -10), (40, 70), (70, 28), A((120, 0, 120)), 3, SOFT),
                CR.quad_bezier((5, 60), (36, -20), (68, 60), A((255, 128, 0)), 2, SOFT), CR.spline_polygon([(20, 10), (60, 30), (30, 58)], A((0, 128, 255)), 2, 0.2, SOFT),
                CR.fill_spline_polygon([(10, 8), (60, 12), (55, 55), (12, 50)], A((128, 255, 0)), 0.5, SOFT), AR.fill_arc((40, 36), 20, 5.0, 8.0, A((255, 255, 255)), SOFT)]
    assert {c["kind"] for c in commands} == set(range(7)) | set(CR.CURVE_KINDS) | set(AR.ARC_KINDS)
    forward, backward = check(host, commands, "forward", host_form=True), check(host, commands[::-1], "backward")
    assert not same_bytes(forward, backward)
    # a width-1 fast arc of a radius that rounds to 0 names its centre pixel up to eight times, a quadrant arc its axis pixels twice
    check(host, [AR.arc((30.2, 30.4), 0.4, 0.0, 5.0, A((200, 40, 40)), 1, FAST), AR.arc((40, 20), 6, 0.0, PI, A((200, 40, 40)), 1, FAST)], "repeated writes")


# ---- the chunk boundary, the count word, a view -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_arcs_on_both_sides_of_the_chunk_boundary():
    """CV_CHUNK is 1024: commands 1023 and 1024 are the last of one chunk and the first of the next."""
    host = background(ROWS, COLS, "rgba_u8", 6)
    rng = np.random.default_rng(7)
    commands = [K.fill_rect(float(x), float(y), float(x) + 2, float(y) + 1, tuple(int(v) for v in rng.integers(0, 256, 3)) + (128,), SOFT)
                for x, y in zip(rng.integers(0, COLS - 2, 1030), rng.integers(0, ROWS - 1, 1030))]
    commands[1023] = AR.fill_arc((20.0, 18.0), 14.0, 0.5, 4.0, (250, 10, 10, 128), SOFT)
    commands[1024] = AR.arc((22.0, 20.0), 12.0, 4.0, 1.0, (10, 10, 250, 128), 3, SOFT)
    want = check(host, commands, "1030 commands")
    assert not same_bytes(want, AR.run(host, commands[:1023] + commands[1025:]))


@pytest.mark.gpu
def test_count_word_shorter_than_the_list_draws_the_prefix():
    host = background(ROWS, COLS, "rgba_u8")
    commands = [make(route, (20.0, 20.0), 15.0, 0.5, 4.0, AR.TRANSLUCENT) for route in ROUTES]
    word = lambda v: torch.tensor([v, 12345], dtype=torch.int32, device="cuda")
    assert same_bytes(on_device(host, commands, word(0)), host)
    assert same_bytes(on_device(host, commands, word(4)), AR.run(host, commands[:4]))
    assert same_bytes(on_device(host, commands, word(99)), AR.run(host, commands))


@pytest.mark.gpu
def test_views_of_a_wider_tensor_leave_their_surroundings_alone():
    rows, cols = T + 3, 2 * T + 1
    commands = [make(route, (cols / 2.0, rows / 2.0), 0.6 * rows, 0.5, 5.0, AR.TRANSLUCENT) for route in ROUTES] + [make(route, (-2.0, 3.0), 9.0, -1.0, 1.5, AR.OPAQUE) for route in ROUTES]
    cmds, vertices = canvas.pack_commands(commands)
    dcmds, dverts = torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), torch.from_numpy(vertices).cuda()
    for pixel in PIXELS:
        inner = background(rows, cols, pixel, 5)
        wide = np.full((rows + 6, cols + 11) + inner.shape[2:], 0xA5, np.uint8)
        wide[2:2 + rows, 4:4 + cols] = inner
        dev = torch.from_numpy(wide).cuda()
        canvas.draw(dev[2:2 + rows, 4:4 + cols], dcmds, vertices=dverts, arcs=True)
        expect = wide.copy()
        expect[2:2 + rows, 4:4 + cols] = AR.run(inner, commands)
        assert same_bytes(dev.cpu().numpy(), expect), pixel


# ---- the contract and the old entry point ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_arcs_outside_the_contract_are_skipped_on_the_device_and_refused_by_the_host_form():
    host = background(40, 40, "rgb_u8")
    good = [AR.fill_arc((20, 20), 15, 0.5, 4.0, AR.TRANSLUCENT, SOFT), AR.arc((18, 22), 12, 3.0, 1.0, AR.OPAQUE, 2, FAST)]
    nan, inf = float("nan"), float("inf")
    arc = AR.arc((20, 20), 10, 0.0, 3.0, AR.OPAQUE, 2, SOFT)
    bad = [dict(arc, pts=[]), dict(arc, pts=[(0.0, 3.0), (1.0, 2.0)]), dict(arc, kind=17, pts=[(0.0, 3.0)] * 4), dict(arc, p=[nan, 20, 10]), dict(arc, p=[20, 20, inf]),
           dict(arc, p=[20, 1e9, 10]), dict(arc, kind=17, p=[20, 20, 70000.0]), dict(arc, mode=2), dict(arc, width=70000)]
    want = AR.run(host, good)
    for b in bad:
        assert same_bytes(on_device(host, [good[0], b, good[1]]), want), b
        out = host.copy()
        with pytest.raises(zg.InvalidArgument):
            canvas.draw_host(out, *canvas.pack_commands([good[0], b, good[1]]))
        assert same_bytes(out, host)
    cmds, vertices = canvas.pack_commands([arc])
    cmds[0]["first_vertex"] = 1  # the angle pair lies outside the array
    dev = torch.from_numpy(host.copy()).cuda()
    canvas.draw(dev, torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), vertices=torch.from_numpy(vertices).cuda(), arcs=True)
    assert same_bytes(dev.cpu().numpy(), host)
    # inside the contract and drawing nothing, in both forms: angles that are not finite, radius <= 0, width 0
    nothing = [dict(arc, pts=[(nan, 1.0)]), dict(arc, kind=17, pts=[(0.0, inf)]), dict(arc, p=[20, 20, 0.0]), dict(arc, kind=17, p=[20, 20, -4.0]), dict(arc, width=0),
               AR.fill_arc((20, 20), 10, 2.0, 2.0, AR.OPAQUE, FAST)]
    assert same_bytes(check(host, [good[0]] + nothing + [good[1]], "nothing drawn", host_form=True), want)
    # any finite angle is inside it
    for a0, a1 in ((1e30, -1e30), (-70000.0, 70001.0), (12345.678, 12347.0), (-3.0e5, -3.0e5 + 2.0)):
        for route in ROUTES:
            check(host, [make(route, (20, 20), 12, a0, a1, AR.OPAQUE)], (route, a0, a1), host_form=route[1] == 4)


@pytest.mark.gpu
def test_the_old_entry_point_still_skips_arcs():
    host = background(ROWS, COLS, "rgba_u8")
    arcs = [make(route, (20.0, 20.0), 15.0, 0.5, 4.0, AR.TRANSLUCENT) for route in ROUTES]
    assert same_bytes(on_device(host, arcs, arcs=False), host)
    mixed = [K.fill_circle(20, 20, 9, AR.TRANSLUCENT, SOFT)] + arcs + [K.line(2, 3, 40, 30, AR.OPAQUE, 2, SOFT)]
    assert same_bytes(on_device(host, mixed, arcs=False), AR.run(host, [mixed[0], mixed[-1]]))
    # and a list without arcs is the same through both
    others = K.every_kind(2, SOFT, K.TRANSLUCENT, ROWS, COLS) + [CR.cubic_bezier((2, 30), (30, -10), (40, 70), (46, 28), AR.TRANSLUCENT, 1, SOFT)]
    assert same_bytes(on_device(host, others, arcs=True), on_device(host, others, arcs=False))
    assert same_bytes(on_device(host, others, arcs=True), AR.run(host, others))


# ---- the Canvas class ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_canvas_class_draws_arcs_on_device_and_host_images():
    host = background(ROWS, COLS, "rgba_u8")
    Tr = AR.TRANSLUCENT
    commands = [AR.fill_arc((20, 20), 15, 0.5, 4.0, Tr, SOFT), K.line(2, 3, 40, 30, AR.OPAQUE, 2, SOFT), AR.arc((24, 18), 12, 4.0, 1.0, Tr, 3, SOFT),
                AR.arc((20, 20), 17, 0.0, PI, AR.OPAQUE, 1, FAST), AR.fill_arc((30, 25), 9, -1.0, 1.0, AR.OPAQUE, FAST)]
    want = AR.run(host, commands)
    for image in (torch.from_numpy(host.copy()).cuda(), host.copy()):
        cv = zg.Canvas(image)
        cv.fill_arc((20, 20), 15, 0.5, 4.0, Tr, "soft").draw_line((2, 3), (40, 30), AR.OPAQUE, 2, "soft").draw_arc((24, 18), 12, 4.0, 1.0, Tr, 3, "soft")
        cv.draw_arc((20, 20), 17, 0.0, PI, AR.OPAQUE).fill_arc((30, 25), 9, -1.0, 1.0, AR.OPAQUE)
        cv.flush()
        assert same_bytes(zg.Image(image).to_numpy(), want)
        cv.draw_line((2, 3), (40, 30), AR.OPAQUE, 2, "soft").flush()  # a list without arcs takes zg_canvas_draw
        assert same_bytes(zg.Image(image).to_numpy(), AR.run(want, [commands[1]]))


# ---- a captured graph -------------------------------------------------------------------------------------------------------------------------
def graph_list(seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(12):
        center = (float(np.float32(rng.uniform(-4, COLS + 4))), float(np.float32(rng.uniform(-4, ROWS + 4))))
        a0, a1 = (float(np.float32(v)) for v in rng.uniform(0.01, 6.2, 2))
        color = tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.choice([255, 128])),)
        out.append(make(ROUTES[k % 6], center, float(np.float32(rng.uniform(2, 25))), a0, a1, color))
        if k % 4 == 3:
            out.append(K.line(*(float(v) for v in rng.uniform(0, 40, 4)), color, 2, SOFT))
    return out


def graph_replay():
    """Captures zg_canvas_draw_arcs as the first canvas call the process makes (everything before it is torch's), then replays the graph
    on other lists, frames and counts."""
    lists = [graph_list(seed) for seed in (401, 402, 403)]
    n = len(lists[0])
    frame = torch.zeros((ROWS, COLS, 4), dtype=torch.uint8, device="cuda")
    dcmds = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    dverts = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")

    def load(k, how_many):
        host = background(ROWS, COLS, "rgba_u8", 10 + k)
        cmds, vertices = canvas.pack_commands(lists[k])
        frame.copy_(torch.from_numpy(host))
        dcmds.copy_(torch.from_numpy(cmds.view(np.uint8).copy()))
        dverts.zero_()
        dverts[:len(vertices)].copy_(torch.from_numpy(vertices))
        count.fill_(how_many)
        return AR.run(host, lists[k][:how_many])

    K.replay_captured(frame, lambda: canvas.draw(frame, dcmds, count=count, vertices=dverts, arcs=True), load, ((0, n), (1, n), (2, 7)))


@pytest.mark.gpu
def test_draw_arcs_is_captured_as_a_fresh_process_first_canvas_call_and_replays_on_changed_lists():
    K.graph_replay_in_a_fresh_process("test_gpu_canvas_arcs")

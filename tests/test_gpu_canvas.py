"""zg_canvas_draw on the device against tests/canvas_ref.py (the reference's calls made one after another), byte for byte: every command
kind, mode, width and pixel type with opaque and translucent colours, the frame shapes where tiling, clipping and the per-row tables can
go wrong, order and multiplicity of blending writes, a seeded random list, views, the count word, the contract, a captured graph replayed
on changed lists and frames, two streams, and the chains detector -> device-built command list -> draw without a synchronisation."""
import numpy as np
import pytest

import zignal_amd as zg
from tests import canvas_cases as K
from tests import canvas_ref as R
from tests.canvas_cases import same_bytes
from zignal_amd import canvas

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

T = zg.canvas_tile()  # a host constant of the library: no GPU needed to read it
PIXELS = ("u8", "rgb_u8", "rgba_u8")
FAST, SOFT = R.FAST, R.SOFT


def background(rows, cols, pixel, seed=1):
    """A frame with structure in every channel; the Rgba one has transparent, translucent and opaque pixels."""
    rng = np.random.default_rng(seed)
    ch = {"u8": 1, "rgb_u8": 3, "rgba_u8": 4}[pixel]
    img = rng.integers(0, 256, (rows, cols, ch)).astype(np.uint8)
    if ch == 4:
        img[..., 3] = np.where(img[..., 3] < 64, 0, np.where(img[..., 3] > 160, 255, img[..., 3]))
    return img[..., 0].copy() if ch == 1 else img


def on_device(host, commands, count=None, n=None):
    """zg_canvas_draw of `commands` into a device copy of `host`; returns the frame."""
    cmds, vertices = canvas.pack_commands(commands)
    dev = torch.from_numpy(host.copy()).cuda()
    dcmds = torch.from_numpy(cmds.view(np.uint8).copy()).cuda() if len(cmds) else torch.zeros(40, dtype=torch.uint8, device="cuda")
    dverts = torch.from_numpy(vertices).cuda() if len(vertices) else None
    canvas.draw(dev, dcmds, count=count, vertices=dverts, n=len(cmds) if n is None else n)
    return dev.cpu().numpy()


def check(host, commands, what):
    want = R.run(host, commands)
    got = on_device(host, commands)
    if not same_bytes(got, want):
        bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first (row, col) {tuple(bad[0])}: device {got[tuple(bad[0])]}, reference {want[tuple(bad[0])]}")
    return want


# ---- every kind x mode x width x pixel type x colour ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("color", [K.OPAQUE, K.TRANSLUCENT], ids=["opaque", "a128"])
@pytest.mark.parametrize("width", [1, 2, 5])
@pytest.mark.parametrize("mode", [FAST, SOFT], ids=["fast", "soft"])
def test_every_kind_equals_the_reference(mode, width, color):
    commands = K.every_kind(width, mode, color)
    for pixel in PIXELS:
        want = check(background(100, 100, pixel), commands, (pixel, mode, width))
        assert not same_bytes(want, background(100, 100, pixel))
    for k, cmd in enumerate(commands):  # and each on its own, on one type each
        check(background(100, 100, PIXELS[k % 3]), [cmd], (k, mode, width))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(T + 1, T + 1), (1, 3 * T + 5), (2 * T + 7, 1), (257, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_edges_tiles_and_degenerate_frames(shape):
    rows, cols = shape
    commands = K.edge_cases(rows, cols) + K.every_kind(2, SOFT, K.TRANSLUCENT, rows, cols) + K.every_kind(5, FAST, K.OPAQUE, rows, cols) \
        + K.every_kind(1, FAST, K.TRANSLUCENT, rows, cols)
    for pixel in (PIXELS if rows * cols < 4096 else ("rgba_u8",)):
        check(background(rows, cols, pixel, 2), commands, (shape, pixel))


@pytest.mark.gpu
def test_edge_cases_one_by_one_on_100x100():
    """Each special case alone, so that none hides behind a later command: zero-length lines of every width, the horizontal and vertical
    cases of both thin-line routines, the axis-aligned thick soft line, parts on every edge and off the image."""
    host = background(100, 100, "rgba_u8", 3)
    for k, cmd in enumerate(K.edge_cases(100, 100)):
        check(host, [cmd], (k, cmd))


@pytest.mark.gpu
def test_shapes_that_reach_the_frame_from_far_away():
    """Long walks before the first visible pixel: Wu's intery has drifted by then, the Bresenham circle has taken thousands of steps, the
    disc's f32 row counter has crossed several binades, and the tile-level tests must still let the right tiles through."""
    T_ = K.TRANSLUCENT

    def through(x, y, dx, dy, before, after):  # a segment through (x, y) of the frame
        return (x - before * dx, y - before * dy, x + after * dx, y + after * dy)

    commands = [K.line(*through(50.3, 40.7, 0.8, 0.6, 17000.0, 14000.0), T_, 1, SOFT), K.line(*through(20.4, 70.2, -0.28, 0.96, 13000.0, 16000.0), T_, 1, SOFT),
                K.line(*through(50.3, 40.7, 0.8, 0.6, 37000.0, 31000.0), K.OPAQUE, 1, FAST), K.line(40.5, -65536.0, 61.25, 65536.0, T_, 1, FAST),
                K.line(-9000.5, 70.25, 9000.0, 20.5, T_, 3, SOFT), K.line(-9000.5, 10.25, 9000.0, 60.5, T_, 4, FAST),
                K.circle(50.4, 5020.3, 4990.6, T_, 1, FAST), K.circle(-3000.2, 40.0, 3050.5, T_, 2, SOFT), K.circle(6000.0, 6000.0, 8400.0, K.OPAQUE, 3, FAST),
                K.fill_circle(50.3, 3000.37, 2990.11, T_, FAST), K.fill_circle(70.3, -2000.6, 2040.2, K.OPAQUE, SOFT),
                K.fill_circle(30.5, 0.3, 33.25, (9, 9, 200, 255), FAST), K.fill_circle(60.25, 15.999999, 15.5, (200, 9, 9, 255), FAST),
                K.rect(-500.5, -400.25, 60.5, 70.75, T_, 1, SOFT), K.fill_polygon([(-4000.5, 50.0), (40.0, -3000.0), (5000.0, 80.0), (55.5, 90.5)], T_, SOFT)]
    host = background(100, 100, "rgba_u8", 6)
    for k, cmd in enumerate(commands):
        want = check(host, [cmd], (k, cmd))
        assert not same_bytes(want, host), k
    check(background(100, 100, "rgb_u8", 6), commands, "all")


# ---- order ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_overlapping_translucent_fills_compose_in_list_order():
    a = K.fill_rect(10, 10, 60, 60, (255, 0, 0, 128), SOFT)
    b = K.fill_circle(55, 50, 25, (0, 0, 255, 128), SOFT)
    for pixel in PIXELS:
        host = background(100, 100, pixel)
        ab, ba = check(host, [a, b], "A then B"), check(host, [b, a], "B then A")
        assert not same_bytes(ab, ba), pixel


@pytest.mark.gpu
def test_u8_and_rgb_frames_are_stored_to_never_blended():
    """setPixel converts the colour to the pixel type before assignPixel sees it, so on u8 and Rgb(u8) a translucent or faded colour
    overwrites: the result does not depend on what the frame held, and equals the opaque colour's wherever the coverage is the same."""
    translucent, opaque = (40, 180, 90, 128), (40, 180, 90, 255)
    commands = lambda c: [K.fill_rect(5, 5, 30, 30, c, SOFT), K.circle(20, 20, 9, c, 1, FAST), K.fill_polygon(K.CONCAVE, c, SOFT), K.line(3, 35, 36, 33, c, 1, SOFT)]
    for pixel in ("u8", "rgb_u8"):
        a, b = background(40, 40, pixel, 8), background(40, 40, pixel, 9)
        wa, wb = check(a, commands(translucent), pixel), check(b, commands(translucent), pixel)
        touched = (wa != a).reshape(40, 40, -1).any(axis=2) | (wb != b).reshape(40, 40, -1).any(axis=2)
        assert touched.sum() > 400 and np.array_equal(wa[touched], wb[touched]), pixel
        assert same_bytes(wa, check(a, commands(opaque), pixel)), pixel
    rgba = background(40, 40, "rgba_u8", 8)
    assert not same_bytes(check(rgba, commands(translucent), "rgba"), check(rgba, commands(opaque), "rgba"))


# ---- multiplicity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_writes_the_reference_repeats_are_repeated():
    color = (250, 10, 10, 128)
    for pixel in PIXELS:
        host = np.full_like(background(40, 40, pixel), 200)
        want = check(host, [K.circle(20, 20, 9, color, 1, FAST)], ("bresenham circle", pixel))
        once = R.Canvas(host.copy())
        once.set_pixel(20, 29, color)  # the points at y == 0 are named twice per step: one blend is not what the reference leaves there ...
        assert np.array_equal(want[20, 29], once.img[20, 29]) == (pixel != "rgba_u8"), pixel  # ... on Rgba; u8 and Rgb are stored to, not blended
        check(host, [K.circle(20.2, 19.7, 0.4, color, 1, FAST)], ("radius rounds to 0: eight writes of the centre", pixel))
        check(host, [K.line(4.2, 3.1, 4.7, 3.4, color, 1, SOFT), K.line(9.6, 5.2, 9.9, 6.4, color, 1, SOFT)], ("Wu shorter than a pixel", pixel))
        want = check(host, [K.fill_polygon(K.SHARED_PIXEL, color, SOFT)], ("spans that share a pixel", pixel))
        check(host, [K.fill_polygon(K.CONCAVE, color, SOFT), K.fill_polygon(K.CONCAVE, color, FAST)], ("concave", pixel))
    # the shared pixel really is shared: row 5 has two spans that both reach column 10
    xs = sorted(np.float32(a[0]) + (np.float32(5) - np.float32(a[1])) * (np.float32(b[0]) - np.float32(a[0])) / (np.float32(b[1]) - np.float32(a[1]))
                for a, b in zip(K.SHARED_PIXEL, K.SHARED_PIXEL[1:] + K.SHARED_PIXEL[:1]) if (a[1] <= 5 < b[1]) or (b[1] <= 5 < a[1]))
    assert len(xs) == 4 and np.ceil(xs[1]) >= np.floor(xs[2])


# ---- a seeded random list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pixel", PIXELS)
def test_a_thousand_random_commands_with_heavy_overlap(pixel):
    rows, cols = 2 * T + 9, 3 * T + 2
    commands = K.random_commands(1100, rows, cols, K.RANDOM_SEED)  # more than the 1024 commands a workgroup lists between two barriers
    check(background(rows, cols, pixel, 4), commands, pixel)


SEAMS = (63, 255, 767, 1023)  # the last entry of a wave, of the first and the third slice of 256, and of a chunk of 1024; its successor follows


@pytest.mark.gpu
def test_order_sensitive_pairs_on_the_wave_slice_and_chunk_seams_of_the_gather():
    """Where the tile's list is put together from the ballots of four waves, four slices and the chunks, a pair of overlapping
    translucent rectangles lies with one command on either side of the seam; every other command lies off the frame, has an empty
    box and must not hit. 17 x 17: two tiles each way, three of them partial, and each pair covers pixels of both tile columns."""
    host = background(T + 1, T + 1, "rgba_u8", 14)
    commands = [K.fill_rect(-40.0 - i % 7, -30.0, -35.0, -20.0 - i % 5, (i % 256, 90, 200, 128), SOFT) for i in range(1030)]
    for k, at in enumerate(SEAMS):  # pair k on rows 4 k .. 4 k + 4: the last one reaches the second tile row
        commands[at] = K.fill_rect(11.0, 4.0 * k, 17.0, 4.0 * k + 4, (250, 10 + 60 * k, 10, 128), SOFT)
        commands[at + 1] = K.fill_rect(13.0, 4.0 * k + 1, 17.0, 4.0 * k + 5, (10, 10 + 60 * k, 250, 128), SOFT)
    want = R.run(host, commands)
    assert (want != host).any(axis=2)[:, :T].any() and (want != host).any(axis=2)[:, T:].any()
    for at in SEAMS:
        swapped = list(commands)
        swapped[at], swapped[at + 1] = commands[at + 1], commands[at]
        assert not same_bytes(want, R.run(host, swapped)), at
    cmds, _ = canvas.pack_commands(commands)
    for arcs in (False, True):
        got = K.on_device(host, cmds, lambda dev, dcmds: canvas.draw(dev, dcmds, arcs=arcs))
        if not same_bytes(got, want):
            raise K.differs(got, want, "1030 commands, pairs on the seams", "zg_canvas_draw_arcs" if arcs else "zg_canvas_draw")


# ---- views ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_views_of_a_wider_tensor_leave_their_surroundings_alone():
    rows, cols = T + 3, 2 * T + 1
    commands = K.edge_cases(rows, cols) + K.every_kind(2, SOFT, K.TRANSLUCENT, rows, cols)
    cmds, vertices = canvas.pack_commands(commands)
    dcmds, dverts = torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), torch.from_numpy(vertices).cuda()
    for pixel in PIXELS:
        inner = background(rows, cols, pixel, 5)
        wide = np.full((rows + 6, cols + 11) + inner.shape[2:], 0xA5, np.uint8)
        wide[2:2 + rows, 4:4 + cols] = inner
        dev = torch.from_numpy(wide).cuda()
        canvas.draw(dev[2:2 + rows, 4:4 + cols], dcmds, vertices=dverts)
        expect = wide.copy()
        expect[2:2 + rows, 4:4 + cols] = R.run(inner, commands)
        assert same_bytes(dev.cpu().numpy(), expect), pixel


# ---- the count word -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_count_device_forms():
    host = background(50, 60, "rgba_u8")
    commands = K.every_kind(2, SOFT, K.TRANSLUCENT, 50, 60)
    word = lambda v: torch.tensor([v, 12345], dtype=torch.int32, device="cuda")
    assert same_bytes(on_device(host, commands, word(0)), host)
    assert same_bytes(on_device(host, commands, word(3)), R.run(host, commands[:3]))
    assert same_bytes(on_device(host, commands, word(len(commands) + 100)), R.run(host, commands))  # at most n
    assert same_bytes(on_device(host, commands, None), R.run(host, commands))
    assert same_bytes(on_device(host, commands, None, n=5), R.run(host, commands[:5]))
    assert same_bytes(on_device(host, [], None), host)


# ---- the contract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_commands_outside_the_contract_are_skipped_on_the_device_and_refused_by_the_host_form():
    host = background(40, 40, "rgb_u8")
    good = [K.fill_circle(20, 20, 8, K.TRANSLUCENT, SOFT), K.line(2, 3, 37, 30, K.OPAQUE, 2, FAST)]
    bad = [K.line(float("nan"), 3, 10, 10), K.line(0, 0, float("inf"), 10), K.circle(5, 5, 70000.0), K.fill_rect(-65537.0, 0, 10, 10),
           K.polygon([(1, 1), (float("nan"), 2), (3, 9)]), K.fill_polygon([(1, 1), (9, 2), (3, 1e9)]),
           dict(K.line(1, 1, 9, 9), kind=7), dict(K.line(1, 1, 9, 9), mode=2), K.line(1, 1, 9, 9, width=70000)]
    want = R.run(host, good)
    for b in bad:
        assert same_bytes(on_device(host, [good[0], b, good[1]]), want), b
        out = host.copy()
        with pytest.raises(zg.InvalidArgument):
            canvas.draw_host(out, *canvas.pack_commands([good[0], b, good[1]]))
        assert same_bytes(out, host)  # refused before anything is drawn
    cmds, vertices = canvas.pack_commands([K.fill_polygon([(1, 1), (9, 2), (3, 7)])])
    cmds[0]["first_vertex"] = 2  # a vertex range past the array
    dev = torch.from_numpy(host.copy()).cuda()
    canvas.draw(dev, torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), vertices=torch.from_numpy(vertices).cuda())
    assert same_bytes(dev.cpu().numpy(), host)
    big = K.fill_polygon([(float(i), float(i * i % 7)) for i in range(65)])
    assert same_bytes(on_device(host, [big]), host)
    with pytest.raises(zg.ZignalError) as e:
        canvas.draw_host(host.copy(), *canvas.pack_commands([big]))
    assert e.value.status == 5  # ZG_ERR_UNSUPPORTED
    ok64 = K.fill_polygon([(20 + 15 * np.cos(i * 0.0982), 20 + 15 * np.sin(i * 0.0982)) for i in range(64)], K.TRANSLUCENT, SOFT)
    check(host, [ok64, dict(ok64, kind=R.KIND_POLYGON, width=2)], "64 vertices")
    for pixel_host in (np.zeros((8, 8), np.float32), np.zeros((8, 8, 4), np.float32)):
        with pytest.raises(zg.ZignalError):
            canvas.draw_host(pixel_host, *canvas.pack_commands(good))
    dev, one = torch.from_numpy(host.copy()).cuda(), torch.zeros(40, dtype=torch.uint8, device="cuda")
    d = zg.Image(dev)._desc()
    import ctypes as C
    for rows, cols in ((32769, 1), (1, 32769)):  # a frame past 32768 a side: refused before anything is enqueued (the pixels are never touched)
        big_frame = type(d)(d.data, cols, rows, cols, d.pixel)
        assert zg.lib().zg_canvas_draw(C.byref(big_frame), C.c_void_p(one.data_ptr()), 1, None, None, 0, None) == 5
        assert zg.lib().zg_canvas_draw_host(C.byref(big_frame), C.c_void_p(one.data_ptr()), 0, None, 0) == 5
    edge_frame = torch.zeros((1, 32768), dtype=torch.uint8, device="cuda")  # 32768 itself is drawn on
    zg.Canvas(edge_frame).draw_line((32700.5, 0), (32767.5, 0), K.OPAQUE).flush()
    assert int(edge_frame[0, 32700:].min()) == R._gray(K.OPAQUE) and int(edge_frame[0, :32700].max()) == 0
    assert zg.lib().zg_canvas_draw(C.byref(d), C.c_void_p(one.data_ptr()), (1 << 24) + 1, None, None, 0, None) == 5  # more commands than a call takes
    torch.cuda.synchronize()
    assert same_bytes(dev.cpu().numpy(), host)


@pytest.mark.gpu
def test_the_canvas_class_draws_on_device_and_host_images():
    host = background(64, 80, "rgba_u8")
    commands = K.every_kind(2, SOFT, K.TRANSLUCENT, 64, 80)
    want = R.run(host, commands)
    for image in (torch.from_numpy(host.copy()).cuda(), host.copy()):
        cv = zg.Canvas(image)
        cv.fill_rectangle(commands[0]["p"], K.TRANSLUCENT, "soft").draw_line(commands[1]["p"][:2], commands[1]["p"][2:], K.TRANSLUCENT, 2, "soft")
        cv.draw_line(commands[2]["p"][:2], commands[2]["p"][2:], K.TRANSLUCENT, 2, "soft").draw_rectangle(commands[3]["p"], K.TRANSLUCENT, 2, "soft")
        cv.draw_circle(commands[4]["p"][:2], commands[4]["p"][2], K.TRANSLUCENT, 2, "soft").fill_circle(commands[5]["p"][:2], commands[5]["p"][2], K.TRANSLUCENT, "soft")
        cv.draw_polygon(commands[6]["pts"], K.TRANSLUCENT, 2, "soft").fill_polygon(commands[7]["pts"], K.TRANSLUCENT, "soft")
        cv.flush()
        assert cv.commands == []
        assert same_bytes(zg.Image(image).to_numpy(), want)


# ---- a captured graph ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_draw_replays_from_a_graph_on_a_changed_command_buffer_and_frame():
    rows, cols, n = 2 * T + 5, 3 * T + 1, 48
    lists = [K.random_commands(n, rows, cols, seed) for seed in (101, 102, 103)]
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
        return R.run(host, lists[k][:how_many])

    side = torch.cuda.Stream()
    load(0, n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # this shape's first call is the captured one
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


# ---- two streams ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_streams_draw_into_two_images_at_once():
    rows, cols = 3 * T + 3, 4 * T + 6
    lists = [K.random_commands(120, rows, cols, 201), K.random_commands(120, rows, cols, 202)]
    hosts = [background(rows, cols, "rgba_u8", 21), background(rows, cols, "rgb_u8", 22)]
    packed = [canvas.pack_commands(l) for l in lists]
    frames = [torch.from_numpy(h.copy()).cuda() for h in hosts]
    dcmds = [torch.from_numpy(c.view(np.uint8).copy()).cuda() for c, _ in packed]
    dverts = [torch.from_numpy(v).cuda() for _, v in packed]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):  # three draws each, interleaved: each later draw composites over the earlier ones
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                canvas.draw(frames[k], dcmds[k], vertices=dverts[k])
    torch.cuda.synchronize()
    for k in (0, 1):
        want = hosts[k]
        for _ in range(3):
            want = R.run(want, lists[k])
        assert same_bytes(frames[k].cpu().numpy(), want), k


# ---- detector -> command list -> draw, nothing synchronised in between ------------------------------------------------------------------------
def _scene(rows, cols):
    rng = np.random.default_rng(31)
    img = rng.integers(90, 110, (rows, cols)).astype(np.uint8)
    img[20:70, 30:120] = 230
    img[55:100, 90:150] = 30
    return img


@pytest.mark.gpu
def test_canny_hough_find_lines_build_draw_chain():
    size, box, shape, cap = 128, (20, 0, 148, 128), (128, 170), 256
    gray = _scene(*shape)
    frame_host = np.repeat(gray[..., None], 4, axis=2).copy()
    frame_host[..., 3] = 255
    src, frame = torch.from_numpy(gray).cuda(), torch.from_numpy(frame_host.copy()).cuda()
    edges = zg.Image(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    acc = torch.zeros((size, size), dtype=torch.int32, device="cuda")
    lines = torch.zeros(cap * 28, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    h = zg.HoughTransform(size)
    color = (255, 40, 0, 160)
    zg.Image(src).canny(1.0, 40, 120, out=edges)
    h.compute_into(edges, acc, box)
    h.find_lines_into(acc, 40, 5.0, 5.0, lines, counts, cap)
    cmds, count = canvas.cmds_from_hough_lines(lines, counts, color, 2, "soft")
    canvas.draw(frame, cmds, count=count)
    torch.cuda.synchronize()
    n = int(counts.cpu().numpy().view(np.uint32)[1])
    assert 0 < n <= cap and int(count.item()) == n
    found = lines.cpu().numpy()[:n * 28].view(zg.HOUGH_LINE_DTYPE)
    commands = [K.line(float(l["p1"][0]), float(l["p1"][1]), float(l["p2"][0]), float(l["p2"][1]), color, 2, SOFT) for l in found]
    built = cmds.cpu().numpy()[:n * 40].view(zg.DRAW_CMD_DTYPE)
    assert built.tobytes() == canvas.pack_commands(commands)[0].tobytes()
    assert same_bytes(frame.cpu().numpy(), R.run(frame_host, commands))


@pytest.mark.gpu
def test_fast_keypoints_build_draw_chain():
    shape, cap = (96, 120), 64  # fewer slots than keypoints: the builder stops at the capacity
    gray = _scene(*shape)
    frame_host = np.repeat(gray[..., None], 3, axis=2).copy()
    src, frame = torch.from_numpy(gray).cuda(), torch.from_numpy(frame_host.copy()).cuda()
    kps = torch.zeros(cap * zg.KEYPOINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    kcount = torch.zeros(1, dtype=torch.int32, device="cuda")
    color = (0, 255, 64, 128)
    zg.Fast(10, True).detect_into(src, kps, kcount, cap)
    cmds, count = canvas.cmds_from_keypoints(kps, kcount, 3.0, color, 1, "fast")
    canvas.draw(frame, cmds, count=count)
    torch.cuda.synchronize()
    n = min(int(kcount.item()), cap)
    assert n > 0 and int(count.item()) == n
    found = kps.cpu().numpy()[:n * zg.KEYPOINT_DTYPE.itemsize].view(zg.KEYPOINT_DTYPE)
    commands = [K.circle(float(k["x"]), float(k["y"]), 3.0, color, 1, FAST) for k in found]
    assert same_bytes(frame.cpu().numpy(), R.run(frame_host, commands))
    assert not same_bytes(frame.cpu().numpy(), frame_host)

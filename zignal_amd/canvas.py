"""Canvas(T) (reference src/canvas/Canvas.zig) over the zg_canvas_* entry points (include/zignal_hip_canvas.h): lines, rectangles,
circles, polygons, Bézier curves and spline polygons drawn into a u8, Rgb(u8) or Rgba(u8) image in place, as one device operation over a command list. The result
equals the reference making the same calls one after another, byte for byte.

    cv = zg.Canvas(image)                       # a device (or host) zg.Image or the tensor / array under it
    cv.draw_line((10, 20), (90, 70), (255, 0, 0, 255), width=2, mode="soft")
    cv.fill_circle((50, 50), 12.5, (0, 255, 0, 128), mode="soft")
    cv.flush()                                  # uploads the list and draws it: asynchronous on the current stream

Colours are Rgba(u8) tuples (three values mean a = 255)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .image import Image, KEYPOINT_DTYPE, _is_torch, torch
from .hough import HOUGH_LINE_DTYPE

# zg_draw_cmd as a numpy structured dtype: the bytes of the C struct
DRAW_CMD_DTYPE = np.dtype([("kind", "<i4"), ("mode", "<i4"), ("width", "<u4"), ("color", "u1", (4,)), ("p", "<f4", (4,)),
                           ("first_vertex", "<u4"), ("n_vertices", "<u4")])
assert DRAW_CMD_DTYPE.itemsize == C.sizeof(L.ZgDrawCmd)
_MODES = {"fast": L.DRAW_FAST, "soft": L.DRAW_SOFT}


def _mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in _MODES:
            raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"canvas: mode {mode!r} (\"fast\" or \"soft\")")
        return _MODES[mode]
    return int(mode)


def _color(color):
    c = tuple(int(v) for v in color)
    if len(c) == 3:
        c += (255,)
    if len(c) != 4 or any(v < 0 or v > 255 for v in c):
        raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"canvas: colour {color!r} (r, g, b[, a] in 0..255)")
    return c


def canvas_tile() -> int:
    """The side of the pixel tiles a workgroup rasterises (zg_canvas_tile)."""
    return int(L.lib().zg_canvas_tile())


def pack_commands(commands):
    """A list of command dicts — kind (zignal_amd._lib.DRAW_*), mode, width, color and p (the float parameters), pts (polygon vertices
    or a curve's points) or both (a spline polygon: p = [tension]) — as (a DRAW_CMD_DTYPE array, an (n_vertices, 2) float32 array): the host form of zg_canvas_draw's two lists."""
    cmds = np.zeros(len(commands), DRAW_CMD_DTYPE)
    vertices = []
    for i, c in enumerate(commands):
        cmds[i]["kind"], cmds[i]["mode"], cmds[i]["width"] = int(c["kind"]), _mode(c.get("mode", L.DRAW_FAST)), int(c.get("width", 1))
        cmds[i]["color"] = _color(c["color"])
        if "pts" in c:
            cmds[i]["first_vertex"], cmds[i]["n_vertices"] = len(vertices), len(c["pts"])
            vertices += [(float(x), float(y)) for x, y in c["pts"]]
        if "p" in c or "pts" not in c:  # a command with neither is an error (KeyError), as it always was
            p = [float(v) for v in c["p"]]
            cmds[i]["p"] = p + [0.0] * (4 - len(p))
    return cmds, np.asarray(vertices, np.float32).reshape(-1, 2)


def draw_host(image, cmds: np.ndarray, vertices=None) -> None:
    """zg_canvas_draw_host: host pixels (a numpy array or a host zg.Image), a DRAW_CMD_DTYPE array and float32 vertex pairs. Synchronous;
    a command outside the contract raises InvalidArgument (a polygon of more than 64 vertices or a filled spline polygon of more than
    CANVAS_MAX_CURVE_POINTS points: ZignalError, unsupported)."""
    img = image if isinstance(image, Image) else Image(image)
    cmds = np.ascontiguousarray(cmds, DRAW_CMD_DTYPE)
    v = np.ascontiguousarray(np.zeros((0, 2), np.float32) if vertices is None else vertices, np.float32).reshape(-1, 2)
    d = img._desc()
    L.check(L.lib().zg_canvas_draw_host(C.byref(d), cmds.ctypes.data if len(cmds) else None, len(cmds), v.ctypes.data if len(v) else None, len(v)))


def _bytes_of(t) -> int:
    return t.numel() * t.element_size()


def has_arcs(commands) -> bool:
    """Does a list of command dicts, or a DRAW_CMD_DTYPE array, hold a drawArc or fillArc? Such a list goes to zg_canvas_draw_arcs."""
    if isinstance(commands, np.ndarray):
        return bool(np.isin(commands["kind"], (L.DRAW_ARC, L.DRAW_FILL_ARC)).any())
    return any(int(c["kind"]) in (L.DRAW_ARC, L.DRAW_FILL_ARC) for c in commands)


def _device_lists(who, img, cmds, itemsize, n, count, *lists) -> int:
    """The checks draw and draw_text (`who`) share: a device image and device tensors (`count` may be None), `cmds` of at least n structs
    of `itemsize` bytes, `count` of a word. Returns n, by default all that `cmds` holds."""
    if not img.on_device or not all(_is_torch(t) for t in (cmds, *lists) + (() if count is None else (count,))):
        raise ValueError(f"{who} takes a device image and device tensors")
    cap = _bytes_of(cmds) // itemsize
    n = cap if n is None else int(n)
    if n > cap or (count is not None and _bytes_of(count) < 4):
        raise ValueError("cmds or count tensor too small")
    return n


def _run_uploaded(device, stream, call, *arrays):
    """A flush's device half: uploads the numpy arrays (None stays None; one synchronous copy each), makes `call` with the tensors on
    `stream` (None: the current one) and records them on it, so that their memory is not reused before the call has run."""
    tensors = [None if a is None else torch.from_numpy(a).to(device) for a in arrays]
    with torch.cuda.stream(stream):  # None: no change of stream, and nothing to record
        call(*tensors)
    for t in tensors if stream is not None else ():
        if t is not None:
            t.record_stream(stream)


def draw(image, cmds, count=None, vertices=None, n=None, arcs=False) -> None:
    """zg_canvas_draw, the device-list form: `cmds` is a device tensor holding zg_draw_cmd structs (n of them; by default as many as it
    holds), `count` an optional device tensor whose first 4 bytes are the number of commands to execute (at most n), `vertices` a
    float32 device tensor of (x, y) pairs. Asynchronous on the current stream; nothing is synchronised, copied or uploaded.
    arcs=True: zg_canvas_draw_arcs, the entry point that also draws DRAW_ARC and DRAW_FILL_ARC (zg_canvas_draw skips them); the host
    cannot see a device list, so the caller who built it says whether it may hold arcs."""
    img = image if isinstance(image, Image) else Image(image)
    n = _device_lists("draw", img, cmds, DRAW_CMD_DTYPE.itemsize, n, count, *(() if vertices is None else (vertices,)))
    if vertices is not None and (vertices.dtype != torch.float32 or not vertices.is_contiguous()):
        raise ValueError("vertices must be a contiguous float32 tensor of (x, y) pairs")
    nv = 0 if vertices is None else vertices.numel() // 2
    d = img._desc()
    entry = L.lib().zg_canvas_draw_arcs if arcs else L.lib().zg_canvas_draw
    with torch.cuda.device(img.data.device):
        L.check(entry(C.byref(d), C.c_void_p(cmds.data_ptr()), n, C.c_void_p(count.data_ptr()) if count is not None else None,
                      C.c_void_p(vertices.data_ptr()) if nv else None, nv, img._stream()))


def _builder_out(list_tensor, itemsize, cmds_out, count_out):
    cap = _bytes_of(list_tensor) // itemsize
    dev = list_tensor.device
    if cmds_out is None:
        cmds_out = torch.zeros(max(cap, 1) * DRAW_CMD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    if count_out is None:
        count_out = torch.zeros(1, dtype=torch.int32, device=dev)
    cap = min(cap, _bytes_of(cmds_out) // DRAW_CMD_DTYPE.itemsize)
    return cap, cmds_out, count_out


def cmds_from_hough_lines(lines, counts, color, width: int = 1, mode="fast", cmds_out=None, count_out=None):
    """zg_canvas_cmds_from_hough_lines: one line command from p1 to p2 per line of HoughTransform.find_lines_into's device list (`lines`,
    `counts`: its two count words). Returns (cmds, count) device tensors for draw(); asynchronous on the current stream."""
    cap, cmds_out, count_out = _builder_out(lines, HOUGH_LINE_DTYPE.itemsize, cmds_out, count_out)
    col = (C.c_uint8 * 4)(*_color(color))
    with torch.cuda.device(lines.device):
        stream = C.c_void_p(torch.cuda.current_stream(lines.device).cuda_stream)
        L.check(L.lib().zg_canvas_cmds_from_hough_lines(C.c_void_p(lines.data_ptr()), C.c_void_p(counts.data_ptr()), cap, col, int(width), _mode(mode),
                                                        C.c_void_p(cmds_out.data_ptr()), C.c_void_p(count_out.data_ptr()), stream))
    return cmds_out, count_out


def cmds_from_keypoints(keypoints, count, radius: float, color, width: int = 1, mode="fast", cmds_out=None, count_out=None):
    """zg_canvas_cmds_from_keypoints: one circle outline of `radius` at each keypoint's (x, y) of a detector's device list (`keypoints`,
    `count`: its count word). Returns (cmds, count) device tensors for draw(); asynchronous on the current stream."""
    cap, cmds_out, count_out = _builder_out(keypoints, KEYPOINT_DTYPE.itemsize, cmds_out, count_out)
    col = (C.c_uint8 * 4)(*_color(color))
    with torch.cuda.device(keypoints.device):
        stream = C.c_void_p(torch.cuda.current_stream(keypoints.device).cuda_stream)
        L.check(L.lib().zg_canvas_cmds_from_keypoints(C.c_void_p(keypoints.data_ptr()), C.c_void_p(count.data_ptr()), cap, float(radius), col, int(width),
                                                      _mode(mode), C.c_void_p(cmds_out.data_ptr()), C.c_void_p(count_out.data_ptr()), stream))
    return cmds_out, count_out


def cmds_from_paths(points, path_offsets, counts, color, width: int = 1, mode="fast", cmds_out=None, count_out=None):
    """zg_canvas_cmds_from_paths: one line command per consecutive pair of points of every path Tracer.trace_into wrote (`points`,
    `path_offsets`, `counts`: its three device tensors). cmds_out defaults to room for one command per point, which no list of paths
    exceeds. Returns (cmds, count) device tensors for draw(); asynchronous on the current stream."""
    cap, cmds_out, count_out = _builder_out(points, 8, cmds_out, count_out)
    col = (C.c_uint8 * 4)(*_color(color))
    with torch.cuda.device(points.device):
        stream = C.c_void_p(torch.cuda.current_stream(points.device).cuda_stream)
        L.check(L.lib().zg_canvas_cmds_from_paths(C.c_void_p(points.data_ptr()), C.c_void_p(path_offsets.data_ptr()), C.c_void_p(counts.data_ptr()), cap, col,
                                                  int(width), _mode(mode), C.c_void_p(cmds_out.data_ptr()), C.c_void_p(count_out.data_ptr()), stream))
    return cmds_out, count_out


def cmds_from_qr(grids, detection, color, width: int = 1, mode="fast", cmds_out=None, count_out=None):
    """zg_canvas_cmds_from_qr: four line commands per grid QrDetector.detect_into wrote (`grids`, `detection`: its device tensors),
    outlining the symbol's corners. cmds_out defaults to room for four commands per grid record `grids` can hold. Returns (cmds, count)
    device tensors for draw(); asynchronous on the current stream."""
    cap, cmds_out, count_out = _builder_out(grids, 32, cmds_out, count_out)  # a grid record is 128 bytes and gives four commands
    col = (C.c_uint8 * 4)(*_color(color))
    with torch.cuda.device(grids.device):
        stream = C.c_void_p(torch.cuda.current_stream(grids.device).cuda_stream)
        L.check(L.lib().zg_canvas_cmds_from_qr(C.c_void_p(grids.data_ptr()), C.c_void_p(detection.data_ptr()), cap, col, int(width), _mode(mode),
                                               C.c_void_p(cmds_out.data_ptr()), C.c_void_p(count_out.data_ptr()), stream))
    return cmds_out, count_out


class Canvas:
    """Canvas(T): the draw methods append to a command list, flush() executes it into the image in list order and empties it."""

    def __init__(self, image):
        self.image = image if isinstance(image, Image) else Image(image)
        self.commands = []

    def _add(self, kind, color, width, mode, p=None, pts=None):
        c = {"kind": kind, "mode": _mode(mode), "width": int(width), "color": _color(color)}
        if pts is not None:
            c["pts"] = [(float(x), float(y)) for x, y in pts]
        if p is not None or pts is None:
            c["p"] = [float(v) for v in p]
        self.commands.append(c)
        return self

    def draw_line(self, p1, p2, color, width: int = 1, mode="fast"):
        return self._add(L.DRAW_LINE, color, width, mode, (p1[0], p1[1], p2[0], p2[1]))

    def draw_rectangle(self, rect, color, width: int = 1, mode="fast"):
        """rect = (l, t, r, b), r and b exclusive."""
        return self._add(L.DRAW_RECT, color, width, mode, rect)

    def fill_rectangle(self, rect, color, mode="fast"):
        return self._add(L.DRAW_FILL_RECT, color, 1, mode, rect)

    def draw_circle(self, center, radius: float, color, width: int = 1, mode="fast"):
        return self._add(L.DRAW_CIRCLE, color, width, mode, (center[0], center[1], radius))

    def fill_circle(self, center, radius: float, color, mode="fast"):
        return self._add(L.DRAW_FILL_CIRCLE, color, 1, mode, (center[0], center[1], radius))

    def draw_polygon(self, points, color, width: int = 1, mode="fast"):
        return self._add(L.DRAW_POLYGON, color, width, mode, pts=points)

    def fill_polygon(self, points, color, mode="fast"):
        return self._add(L.DRAW_FILL_POLYGON, color, 1, mode, pts=points)

    def draw_quadratic_bezier(self, p0, p1, p2, color, width: int = 1, mode="fast"):
        return self._add(L.DRAW_QUAD_BEZIER, color, width, mode, pts=(p0, p1, p2))

    def draw_cubic_bezier(self, p0, p1, p2, p3, color, width: int = 1, mode="fast"):
        return self._add(L.DRAW_CUBIC_BEZIER, color, width, mode, pts=(p0, p1, p2, p3))

    def draw_spline_polygon(self, points, color, width: int = 1, tension: float = 0.5, mode="fast"):
        """The polygon's edges as cubic Béziers through its vertices; tension 0 (sharp corners) to 1 (smoothest), clamped."""
        return self._add(L.DRAW_SPLINE_POLYGON, color, width, mode, p=(tension,), pts=points)

    def fill_spline_polygon(self, points, color, tension: float = 0.5, mode="fast"):
        """At most CANVAS_MAX_CURVE_POINTS points once tessellated (3 pixels a segment, 4 to 50 points an edge)."""
        return self._add(L.DRAW_FILL_SPLINE_POLYGON, color, 1, mode, p=(tension,), pts=points)

    def draw_arc(self, center, radius: float, start_angle: float, end_angle: float, color, width: int = 1, mode="fast"):
        """Angles in radians from the positive x axis towards positive y, any finite value (normalised as the reference does); a span of
        2 pi or more is the circle, a NaN or infinite angle draws nothing."""
        return self._add(L.DRAW_ARC, color, width, mode, (center[0], center[1], radius), pts=((start_angle, end_angle),))

    def fill_arc(self, center, radius: float, start_angle: float, end_angle: float, color, mode="fast"):
        """The pie slice between the two angles (see draw_arc)."""
        return self._add(L.DRAW_FILL_ARC, color, 1, mode, (center[0], center[1], radius), pts=((start_angle, end_angle),))

    def draw_text(self, text, position, color, font, scale: float = 1.0, mode="fast"):
        """drawText: `text` (a str, decoded to its codepoints; "\\n" starts a new line) with its top left corner at `position`, in a
        zg.BitmapFont. scale == 1 lights the glyphs' bits in either mode; otherwise "fast" writes a block per bit and "soft" box-filtered
        coverage. scale <= 0 draws nothing; scale at most TEXT_MAX_SCALE."""
        from .text import codepoints_of

        self.commands.append({"text": codepoints_of(text), "x": float(position[0]), "y": float(position[1]), "scale": float(scale), "mode": _mode(mode),
                              "color": _color(color), "font": font})
        return self

    def flush(self, stream=None) -> None:
        """Draw the list and empty it. Device image: the two lists are uploaded (one synchronous copy each) and zg_canvas_draw — or
        zg_canvas_draw_arcs when the list holds an arc — runs on `stream` (a torch stream; default: the current one). Host image:
        zg_canvas_draw_host. A list with text in it is cut into maximal runs of text and of everything else, issued in list order on the one
        stream: the others as above, a run of text through zg_canvas_draw_text (host image: zg_canvas_draw_text_host), one call per font."""
        commands, self.commands = self.commands, []
        if not commands:
            return
        if not any("text" in c for c in commands):
            self._flush_shapes(commands, stream)
            return
        run = []
        for c in commands + [None]:
            if run and (c is None or ("text" in c) != ("text" in run[0]) or ("text" in c and c["font"] is not run[0]["font"])):
                if "text" in run[0]:
                    self._flush_text(run, stream)
                else:
                    self._flush_shapes(run, stream)
                run = []
            run.append(c)

    def _flush_text(self, commands, stream) -> None:
        from . import text as T

        font = commands[0]["font"]
        cmds, cps = T.pack_text(commands)
        if not self.image.on_device:
            T.draw_text_host(self.image, font, cmds, cps)
            return
        if len(cps):
            _run_uploaded(self.image.data.device, stream, lambda dcmds, dcps: T.draw_text(self.image, font, dcmds, dcps), cmds.view(np.uint8), cps.view(np.int32))

    def _flush_shapes(self, commands, stream) -> None:
        cmds, vertices = pack_commands(commands)
        if not self.image.on_device:
            draw_host(self.image, cmds, vertices)
            return
        arcs = has_arcs(cmds)
        _run_uploaded(self.image.data.device, stream, lambda dcmds, dverts: draw(self.image, dcmds, vertices=dverts, arcs=arcs), cmds.view(np.uint8),
                      vertices if len(vertices) else None)

    def draw(self, cmds_tensor, count=None, vertices=None, arcs=False) -> None:
        """The device-list form: see zignal_amd.canvas.draw."""
        draw(self.image, cmds_tensor, count, vertices, arcs=arcs)

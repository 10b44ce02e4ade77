"""Command lists shared by the CPU and GPU Canvas tests. A command is the dict tests/canvas_ref.run executes: kind, mode, width, color
(Rgba(u8)) and p (x1 y1 x2 y2 | l t r b | cx cy radius) or pts (polygon vertices)."""
from __future__ import annotations

import json
import os

import numpy as np

from tests import canvas_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canvas_md5.json")
_CALLS = {"line": ref.KIND_LINE, "rect": ref.KIND_RECT, "fill_rect": ref.KIND_FILL_RECT, "circle": ref.KIND_CIRCLE,
          "fill_circle": ref.KIND_FILL_CIRCLE, "polygon": ref.KIND_POLYGON, "fill_polygon": ref.KIND_FILL_POLYGON}
_MODES = {"fast": ref.FAST, "soft": ref.SOFT}
OPAQUE, TRANSLUCENT = (200, 60, 120, 255), (40, 180, 90, 128)
RANDOM_SEED = 20261019  # the seeded random list of test_gpu_canvas.py


def golden_cases():
    """(name, md5, command) of the eighteen in-scope cases of the reference's regression list, and the fixture's header."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for c in doc["cases"]:
        cmd = {"kind": _CALLS[c["call"]], "mode": _MODES[c["mode"]], "width": c["width"], "color": tuple(c["color"])}
        if "pts" in c:
            cmd["pts"] = [tuple(p) for p in c["pts"]]
        else:
            cmd["p"] = list(c["p"])
        out.append((c["name"], c["md5"], cmd))
    return doc, out


def line(x1, y1, x2, y2, color=OPAQUE, width=1, mode=ref.FAST):
    return {"kind": ref.KIND_LINE, "mode": mode, "width": width, "color": color, "p": [x1, y1, x2, y2]}


def rect(l, t, r, b, color=OPAQUE, width=1, mode=ref.FAST):
    return {"kind": ref.KIND_RECT, "mode": mode, "width": width, "color": color, "p": [l, t, r, b]}


def fill_rect(l, t, r, b, color=OPAQUE, mode=ref.FAST):
    return {"kind": ref.KIND_FILL_RECT, "mode": mode, "width": 1, "color": color, "p": [l, t, r, b]}


def circle(cx, cy, radius, color=OPAQUE, width=1, mode=ref.FAST):
    return {"kind": ref.KIND_CIRCLE, "mode": mode, "width": width, "color": color, "p": [cx, cy, radius]}


def fill_circle(cx, cy, radius, color=OPAQUE, mode=ref.FAST):
    return {"kind": ref.KIND_FILL_CIRCLE, "mode": mode, "width": 1, "color": color, "p": [cx, cy, radius]}


def polygon(pts, color=OPAQUE, width=1, mode=ref.FAST):
    return {"kind": ref.KIND_POLYGON, "mode": mode, "width": width, "color": color, "pts": [tuple(p) for p in pts]}


def fill_polygon(pts, color=OPAQUE, mode=ref.FAST):
    return {"kind": ref.KIND_FILL_POLYGON, "mode": mode, "width": 1, "color": color, "pts": [tuple(p) for p in pts]}


CONCAVE = [(4.0, 3.0), (12.0, 14.0), (20.5, 3.0), (28.0, 17.0), (16.0, 27.5), (3.0, 20.0)]      # an M: two spans on its upper rows
# a notch 0.2 px wide cut into the top edge: on the rows it crosses, the span left of it and the span right of it end in the same pixels
SHARED_PIXEL = [(2.0, 2.0), (10.4, 2.0), (10.5, 12.0), (10.6, 2.0), (19.0, 2.0), (19.0, 18.0), (2.0, 18.0)]


def every_kind(width, mode, color, rows=100, cols=100):
    """One command of every kind, sized to the frame, that straddles the 16-pixel tile borders and crosses the others."""
    w, h = float(cols), float(rows)
    return [
        fill_rect(0.1 * w, 0.15 * h, 0.7 * w, 0.6 * h, color, mode),
        line(0.05 * w, 0.1 * h, 0.9 * w, 0.8 * h, color, width, mode),
        line(0.9 * w, 0.05 * h, 0.65 * w, 0.95 * h, color, width, mode),
        rect(0.2 * w, 0.3 * h, 0.85 * w, 0.9 * h, color, width, mode),
        circle(0.5 * w, 0.5 * h, 0.31 * min(w, h), color, width, mode),
        fill_circle(0.3 * w + 0.25, 0.6 * h + 0.5, 0.17 * min(w, h), color, mode),
        polygon([(0.5 * w, 0.1 * h), (0.92 * w, 0.45 * h), (0.6 * w, 0.93 * h), (0.12 * w, 0.7 * h)], color, width, mode),
        fill_polygon([(0.1 * w, 0.1 * h), (0.4 * w, 0.45 * h), (0.7 * w, 0.12 * h), (0.95 * w, 0.66 * h), (0.55 * w, 0.9 * h), (0.08 * w, 0.7 * h)], color, mode),
    ]


def edge_cases(rows, cols):
    """Parts on each image edge, wholly off the image, covering all of it; zero-length lines; the special cases of each line routine."""
    w, h = float(cols), float(rows)
    T = TRANSLUCENT
    out = [fill_rect(-5, -5, w + 5, h + 5, (10, 20, 30, 128), ref.SOFT)]                                 # covers the whole image
    out += [fill_circle(-40, -40, 10, OPAQUE, m) for m in (ref.FAST, ref.SOFT)]                           # wholly off the image
    out += [line(-30, -8, -2, -3, OPAQUE, wd, m) for wd in (1, 3) for m in (ref.FAST, ref.SOFT)]
    out += [circle(w + 50, h / 2, 20, OPAQUE, wd, ref.FAST) for wd in (1, 4)]
    out += [fill_polygon([(w + 3, 1), (w + 30, 5), (w + 9, 40)], OPAQUE, m) for m in (ref.FAST, ref.SOFT)]
    for m in (ref.FAST, ref.SOFT):                                                                      # on each edge
        out += [line(-4, 0, w + 4, 0, T, 1, m), line(0, -3, 0, h + 3, T, 1, m), line(-2.5, h - 1, w + 3, h - 1, T, 2, m),
                line(w - 1, -2, w - 1, h + 6, T, 3, m), circle(0, 0, 6.5, T, 1, m), circle(w - 1, h - 1, 7, T, 2, m),
                fill_circle(w - 0.5, 2.25, 4.75, T, m), fill_circle(1.5, h - 0.25, 5, T, m), rect(0, 0, w, h, T, 1, m),
                rect(-3, -3, w + 3, h + 3, T, 5, m), fill_polygon([(-6, h / 2), (w / 3, -4), (w + 5, h / 3), (w / 2, h + 7)], T, m)]
    for wd in (1, 2, 5):                                                                                # zero-length lines
        for m in (ref.FAST, ref.SOFT):
            out += [line(w / 2 + wd, h / 3, w / 2 + wd, h / 3, T, wd, m), line(3.5 + wd, 2.25, 3.5 + wd, 2.25, OPAQUE, wd, m)]
    out += [line(2.3, 7.0, w - 3.6, 7.004, T, 1, ref.SOFT), line(w - 2.5, 9.5, 1.25, 9.5, OPAQUE, 1, ref.SOFT),  # Wu's horizontal case
            line(5.0, 11.0, 9.0, 11.0, T, 1, ref.SOFT),                                                       # integer ends: no end pixels
            line(4.2, 3.1, 4.7, 3.4, T, 1, ref.SOFT), line(6.6, 5.2, 6.9, 6.4, T, 1, ref.SOFT),              # Wu lines shorter than a pixel
            line(3, h / 2, w - 4, h / 2, OPAQUE, 1, ref.FAST), line(w / 2, 2, w / 2, h - 3, OPAQUE, 1, ref.FAST),  # Bresenham's special cases
            line(w - 4.2, 2.9, 2.1, h - 2.2, T, 1, ref.FAST), line(2, 3, 9, h - 2, T, 1, ref.FAST),          # its general case, both majors
            line(4.5, h / 4, w - 6.25, h / 4, OPAQUE, 4, ref.SOFT), line(4.5, h / 4 + 8, w - 6.25, h / 4 + 8, T, 5, ref.SOFT),  # axis-aligned thick soft
            line(w / 4, h - 3.5, w / 4, 2.75, OPAQUE, 2, ref.SOFT), line(w / 4 + 7.5, h - 3.5, w / 4 + 7.5, 2.75, T, 3, ref.SOFT)]
    return out


def random_commands(n, rows, cols, seed=RANDOM_SEED):
    """n mixed commands with heavy overlap: small shapes scattered over (and a little beyond) the frame, half of them translucent."""
    rng = np.random.default_rng(seed)
    w, h = float(cols), float(rows)
    out = []

    def pt():
        return float(np.float32(rng.uniform(-6, w + 6))), float(np.float32(rng.uniform(-6, h + 6)))

    for _ in range(n):
        kind = int(rng.integers(0, 7))
        mode = int(rng.integers(0, 2))
        width = int(rng.choice([1, 1, 2, 3, 5]))
        color = tuple(int(v) for v in rng.integers(0, 256, 3)) + (255 if rng.random() < 0.5 else int(rng.integers(0, 255)),)
        x, y = pt()
        s = float(np.float32(rng.uniform(1, 14)))
        if kind == ref.KIND_LINE:
            dx, dy = rng.uniform(-14, 14, 2)
            if rng.random() < 0.3:
                (dx, dy) = (0.0, dy) if rng.random() < 0.5 else (dx, 0.0)
            out.append(line(x, y, float(np.float32(x + dx)), float(np.float32(y + dy)), color, width, mode))
        elif kind == ref.KIND_RECT:
            out.append(rect(x, y, float(np.float32(x + s)), float(np.float32(y + rng.uniform(1, 14))), color, width, mode))
        elif kind == ref.KIND_FILL_RECT:
            out.append(fill_rect(x, y, float(np.float32(x + s)), float(np.float32(y + rng.uniform(1, 14))), color, mode))
        elif kind == ref.KIND_CIRCLE:
            out.append(circle(x, y, s * 0.6, color, width, mode))
        elif kind == ref.KIND_FILL_CIRCLE:
            out.append(fill_circle(x, y, s * 0.6, color, mode))
        else:
            nv = int(rng.integers(3, 8))
            ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
            rad = rng.uniform(0.3, 1.0, nv) * s
            pts = [(float(np.float32(x + r * np.cos(a))), float(np.float32(y + r * np.sin(a)))) for a, r in zip(ang, rad)]
            out.append(polygon(pts, color, width, mode) if kind == ref.KIND_POLYGON else fill_polygon(pts, color, mode))
    return out


# ---- what the GPU tests of the drawing entry points share (shapes, arcs, text) ---------------------------------------------------------
def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def on_device(host, cmds, draw):
    """A device copy of `host` after draw(frame, dcmds), dcmds being the packed `cmds` as bytes on the device (an empty list: one zeroed
    struct, so that there is an address); returns the frame."""
    import torch

    dev = torch.from_numpy(host.copy()).cuda()
    dcmds = torch.from_numpy(cmds.view(np.uint8).copy()).cuda() if len(cmds) else torch.zeros(cmds.dtype.itemsize, dtype=torch.uint8, device="cuda")
    draw(dev, dcmds)
    return dev.cpu().numpy()


def on_host(host, draw_host, *packed):
    out = host.copy()
    draw_host(out, *packed)
    return out


def differs(got, want, what, form):
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2))
    return AssertionError(f"{what} ({form}): {len(bad)} pixels differ, first (row, col) {tuple(bad[0])}: got {got[tuple(bad[0])]}, reference {want[tuple(bad[0])]}")


def check(want, what, *forms):
    """Every form — (entry point's name, callable that returns the frame it drew) — equals the restatement's `want`."""
    for form, draw in forms:
        got = draw()
        if not same_bytes(got, want):
            raise differs(got, want, what, form)
    return want


def replay_captured(frame, draw, load, rounds):
    """Captures draw() on a side stream, then replays the graph once per (k, how_many) of `rounds`, after load(k, how_many) has
    refilled the buffers the capture saw and returned what `frame` must hold afterwards."""
    import torch

    import zignal_amd as zg

    side = torch.cuda.Stream()
    load(*rounds[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        draw()
    for k, how_many in rounds:
        want = load(k, how_many)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(frame.cpu().numpy(), want), (k, how_many)
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0


def graph_replay_in_a_fresh_process(module):
    """tests.<module>.graph_replay() in a process of its own, so that its capture holds the first drawing call the process makes."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", f"from tests.{module} import graph_replay; graph_replay(); print('ok')"], capture_output=True,
                         text=True, timeout=300, cwd=root)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]

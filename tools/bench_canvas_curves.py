"""Canvas curves on the device: µs per zg_canvas_draw into a 1080p Rgba(u8) frame for one list,
  curves    200 cubic Béziers (width 2, soft, a few hundred pixels long) plus 100 soft spline-polygon outlines of width 3 (five vertices
            40-200 pixels from their centre)
timed as tools/bench_canvas.py times its lists (tools/bench_orb.py's time_leg: three rotating frames, warm, HIP events round a batch of
calls, eager and as a replayed graph). The lists are device-resident.

usage: python tools/bench_canvas_curves.py [--reps N] [--json OUT]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_orb import ROTATE, time_leg  # noqa: E402

ROWS, COLS = 1080, 1920
SEED = 7


def curves():
    from zignal_amd import _lib as L
    rng = np.random.default_rng(SEED)
    w, h = float(COLS), float(ROWS)

    def color():
        return tuple(int(v) for v in rng.integers(0, 256, 3)) + (128,)

    out = []
    for _ in range(200):
        x, y = rng.uniform(0, w), rng.uniform(0, h)
        pts = [(x + dx, y + dy) for dx, dy in rng.uniform(-250, 250, (4, 2))]
        out.append({"kind": L.DRAW_CUBIC_BEZIER, "mode": L.DRAW_SOFT, "width": 2, "color": color(), "pts": pts})
    for _ in range(100):
        x, y, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(40, 200)
        angles = np.sort(rng.uniform(0, 2 * np.pi, 5))
        out.append({"kind": L.DRAW_SPLINE_POLYGON, "mode": L.DRAW_SOFT, "width": 3, "color": color(), "p": [0.5],
                    "pts": [(x + r * np.cos(a), y + r * np.sin(a)) for a in angles]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import canvas
    if not torch.cuda.is_available():
        sys.exit("bench_canvas_curves needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    rng = np.random.default_rng(SEED)
    host = rng.integers(0, 256, (ROWS, COLS, 4)).astype(np.uint8)
    frames = [torch.from_numpy(np.roll(host, 37 * i, axis=1).copy()).cuda() for i in range(ROTATE)]
    descs = [zg.Image(f)._desc() for f in frames]
    cmds, vertices = canvas.pack_commands(curves())
    dcmds = torch.from_numpy(cmds.view(np.uint8).copy()).cuda()
    dverts = torch.from_numpy(vertices).cuda()
    n, nv = len(cmds), len(vertices)

    def draw(stream, i):
        L.check(lib.zg_canvas_draw(C.byref(descs[i % ROTATE]), C.c_void_p(dcmds.data_ptr()), n, None, C.c_void_p(dverts.data_ptr()), nv, stream))

    replay, eager, reps = time_leg(torch, L, draw, args.reps)
    r = {"frame": "1080p", "pixel": "rgba_u8", "list": "curves", "commands": n, "us_graph_replay": replay, "us_eager": eager, "reps": reps}
    print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump([r], f, indent=1)


if __name__ == "__main__":
    main()

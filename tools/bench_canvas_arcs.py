"""Canvas arcs on the device: µs per call into a 1080p Rgba(u8) frame, for
  --list overlay   tools/bench_canvas.py's overlay list (500 circle outlines + 100 width-2 soft lines; no arc in it) through
                   --entry draw (zg_canvas_draw) or --entry arcs (zg_canvas_draw_arcs): what the larger kernel costs a list without arcs
  --list arcs      300 soft arc outlines of width 2, 200 soft pie slices and 200 fast arcs of width 1, radius 20-60, through
                   zg_canvas_draw_arcs
timed as tools/bench_canvas.py times its lists (tools/bench_orb.py's time_leg: three rotating frames, warm, HIP events round a batch of
calls, eager and as a replayed graph). The lists are device-resident. One list and one entry point per process.

usage: python tools/bench_canvas_arcs.py [--list overlay|arcs] [--entry draw|arcs] [--reps N] [--json OUT]
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

from bench_canvas import lists  # noqa: E402
from bench_orb import ROTATE, time_leg  # noqa: E402

ROWS, COLS = 1080, 1920
SEED = 7


def arcs():
    from zignal_amd import _lib as L
    rng = np.random.default_rng(SEED)
    w, h = float(COLS), float(ROWS)
    out = []
    for kind, mode, width, count in ((L.DRAW_ARC, L.DRAW_SOFT, 2, 300), (L.DRAW_FILL_ARC, L.DRAW_SOFT, 1, 200), (L.DRAW_ARC, L.DRAW_FAST, 1, 200)):
        for _ in range(count):
            start = float(rng.uniform(0.01, 6.2))
            out.append({"kind": kind, "mode": mode, "width": width, "color": tuple(int(v) for v in rng.integers(0, 256, 3)) + (128,),
                        "p": [rng.uniform(0, w), rng.uniform(0, h), rng.uniform(20, 60)], "pts": [(start, start + float(rng.uniform(0.3, 5.5)))]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", default="arcs", choices=("overlay", "arcs"))
    ap.add_argument("--entry", default="arcs", choices=("draw", "arcs"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.list == "arcs" and args.entry != "arcs":
        sys.exit("the arcs list is drawn by zg_canvas_draw_arcs only (zg_canvas_draw skips arcs)")
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import canvas
    if not torch.cuda.is_available():
        sys.exit("bench_canvas_arcs needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    rng = np.random.default_rng(SEED)
    host = rng.integers(0, 256, (ROWS, COLS, 4)).astype(np.uint8)
    frames = [torch.from_numpy(np.roll(host, 37 * i, axis=1).copy()).cuda() for i in range(ROTATE)]
    descs = [zg.Image(f)._desc() for f in frames]
    cmds, vertices = canvas.pack_commands(arcs() if args.list == "arcs" else lists(ROWS, COLS)["overlay"])
    dcmds = torch.from_numpy(cmds.view(np.uint8).copy()).cuda()
    dverts = torch.from_numpy(vertices).cuda() if len(vertices) else None
    n, nv = len(cmds), len(vertices)
    entry = lib.zg_canvas_draw_arcs if args.entry == "arcs" else lib.zg_canvas_draw

    def draw(stream, i):
        L.check(entry(C.byref(descs[i % ROTATE]), C.c_void_p(dcmds.data_ptr()), n, None, C.c_void_p(dverts.data_ptr()) if nv else None, nv, stream))

    replay, eager, reps = time_leg(torch, L, draw, args.reps)
    r = {"frame": "1080p", "pixel": "rgba_u8", "list": args.list, "entry": "zg_canvas_draw_arcs" if args.entry == "arcs" else "zg_canvas_draw", "commands": n,
         "us_graph_replay": replay, "us_eager": eager, "reps": reps}
    print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump([r], f, indent=1)


if __name__ == "__main__":
    main()

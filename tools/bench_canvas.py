"""Canvas on the device: µs per zg_canvas_draw into a 1080p and a 4096^2 Rgba(u8) frame, for three lists:
  overlay   500 circle outlines (radius 6, width 1, fast) plus 100 width-2 soft lines across the frame: what ORB + Hough leave to draw
  fill      one full-frame translucent fillRectangle (.soft): every pixel loaded, blended and stored once
  discs     10 000 small filled discs (radius 2-6, both modes, half of them translucent)
Timed with tools/bench_orb.py's time_leg: three rotating frames, warm, HIP events round a batch of calls, eager and as a replayed graph.
The lists are device-resident; drawing over an already drawn frame costs the same as over a fresh one, so the frames are not restored.

Beside every row, from the same run and the same frames: zg_copy of the frame (the floor for touching every pixel once) and the download
+ upload of the frame through pinned host memory (the round trip that drawing on the device removes; the CPU's own drawing time would
come on top of it and is not measured here).

usage: python tools/bench_canvas.py [--reps N] [--json OUT] [--frame 1080p|4096] [--list overlay|fill|discs]
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

SHAPES = {"1080p": (1080, 1920), "4096": (4096, 4096)}
SEED = 7


def lists(rows, cols):
    from zignal_amd import _lib as L
    rng = np.random.default_rng(SEED)
    w, h = float(cols), float(rows)

    def color(translucent):
        return tuple(int(v) for v in rng.integers(0, 256, 3)) + (128 if translucent else 255,)

    overlay = [{"kind": L.DRAW_CIRCLE, "mode": L.DRAW_FAST, "width": 1, "color": color(False), "p": [rng.uniform(0, w), rng.uniform(0, h), 6.0]} for _ in range(500)]
    overlay += [{"kind": L.DRAW_LINE, "mode": L.DRAW_SOFT, "width": 2, "color": color(True),
                 "p": [0.0, rng.uniform(0, h), w - 1, rng.uniform(0, h)] if k % 2 else [rng.uniform(0, w), 0.0, rng.uniform(0, w), h - 1]} for k in range(100)]
    fill = [{"kind": L.DRAW_FILL_RECT, "mode": L.DRAW_SOFT, "width": 1, "color": (40, 120, 200, 128), "p": [0.0, 0.0, w, h]}]
    discs = [{"kind": L.DRAW_FILL_CIRCLE, "mode": int(k % 2), "width": 1, "color": color(k % 4 < 2), "p": [rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 6)]}
             for k in range(10000)]
    return {"overlay": overlay, "fill": fill, "discs": discs}


def time_round_trip(torch, frames, reps):
    """µs per download + upload of one frame through pinned host memory, HIP events round a batch."""
    stream = torch.cuda.Stream()
    pinned = torch.empty(frames[0].shape, dtype=frames[0].dtype).pin_memory()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(stream):
        for i in range(2 * ROTATE + reps):
            if i == 2 * ROTATE:
                ev[0].record(stream)
            pinned.copy_(frames[i % ROTATE], non_blocking=True)
            frames[i % ROTATE].copy_(pinned, non_blocking=True)
        ev[1].record(stream)
    stream.synchronize()
    return round(ev[0].elapsed_time(ev[1]) * 1000.0 / reps, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--json", default=None)
    ap.add_argument("--frame", default=None, choices=sorted(SHAPES))
    ap.add_argument("--list", default=None, choices=("overlay", "fill", "discs"))
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import canvas
    if not torch.cuda.is_available():
        sys.exit("bench_canvas needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    out = []
    for fname, (rows, cols) in SHAPES.items():
        if args.frame not in (None, fname):
            continue
        rng = np.random.default_rng(SEED)
        host = rng.integers(0, 256, (rows, cols, 4)).astype(np.uint8)
        frames = [torch.from_numpy(np.roll(host, 37 * i, axis=1).copy()).cuda() for i in range(ROTATE)]
        images = [zg.Image(f) for f in frames]
        dst = zg.Image(torch.empty_like(frames[0]))
        descs, ddesc = [im._desc() for im in images], dst._desc()

        def copy(stream, i):
            L.check(lib.zg_copy(C.byref(descs[i % ROTATE]), C.byref(ddesc), stream))

        copy_replay, copy_eager, _ = time_leg(torch, L, copy, args.reps)
        round_trip = time_round_trip(torch, frames, max(6, args.reps // 4))
        for name, commands in lists(rows, cols).items():
            if args.list not in (None, name):
                continue
            cmds, vertices = canvas.pack_commands(commands)
            dcmds = torch.from_numpy(cmds.view(np.uint8).copy()).cuda()
            n = len(cmds)

            def draw(stream, i):
                L.check(lib.zg_canvas_draw(C.byref(descs[i % ROTATE]), C.c_void_p(dcmds.data_ptr()), n, None, None, 0, stream))

            replay, eager, reps = time_leg(torch, L, draw, args.reps)
            r = {"frame": fname, "pixel": "rgba_u8", "list": name, "commands": n, "us_graph_replay": replay, "us_eager": eager, "reps": reps,
                 "copy_us_graph_replay": copy_replay, "copy_us_eager": copy_eager, "download_upload_us": round_trip}
            print(json.dumps(r), flush=True)
            out.append(r)
            assert len(vertices) == 0
        del frames, images, dst
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

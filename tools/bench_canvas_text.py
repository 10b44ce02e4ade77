"""drawText on the device: µs per call of zg_canvas_draw_text into a 1080p Rgba(u8) frame, 100 labels of 12 characters in an 8 x 8 fixed
font (seeded bitmaps made here), translucent, at
  scale 1            the unscaled path
  scale 2 fast       a block per bit
  scale 2 soft       box-filtered coverage
  overlay + soft     tools/bench_canvas.py's 600-command overlay list through zg_canvas_draw, then the scale 2 soft labels: two calls
and, in the same run, the frame's download plus upload through pinned memory (tools/bench_canvas.py's time_round_trip): the round trip a
label drawn on the CPU costs before a single glyph is drawn, the only comparison made. Timed as tools/bench_canvas.py times its lists
(tools/bench_orb.py's time_leg: three rotating frames, warm, HIP events round a batch of calls, eager and as a replayed graph). The lists
and the font are device-resident.

usage: python tools/bench_canvas_text.py [--reps N] [--json OUT]
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

from bench_canvas import lists, time_round_trip  # noqa: E402
from bench_orb import ROTATE, time_leg  # noqa: E402

ROWS, COLS = 1080, 1920
SEED = 7
LABELS, CHARS = 100, 12


def labels(scale, mode):
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(LABELS):
        text = "".join(chr(int(v)) for v in rng.integers(33, 127, CHARS))
        out.append({"text": text, "x": float(rng.uniform(0, COLS - CHARS * 8 * scale)), "y": float(rng.uniform(0, ROWS - 8 * scale)), "scale": scale, "mode": mode,
                    "color": tuple(int(v) for v in rng.integers(0, 256, 3)) + (128,)})
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
    from zignal_amd import text as T
    if not torch.cuda.is_available():
        sys.exit("bench_canvas_text needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    rng = np.random.default_rng(SEED)
    host = rng.integers(0, 256, (ROWS, COLS, 4)).astype(np.uint8)
    frames = [torch.from_numpy(np.roll(host, 37 * i, axis=1).copy()).cuda() for i in range(ROTATE)]
    descs = [zg.Image(f)._desc() for f in frames]
    font = zg.BitmapFont.from_fixed(8, 8, 32, rng.integers(0, 256, 96 * 8).astype(np.uint8))
    dfont = font._device_font(frames[0].device)
    ocmds, overts = canvas.pack_commands(lists(ROWS, COLS)["overlay"])
    docmds, doverts = torch.from_numpy(ocmds.view(np.uint8).copy()).cuda(), torch.from_numpy(overts).cuda() if len(overts) else None
    results = []
    for name, scale, mode, overlay in (("scale 1", 1.0, L.DRAW_FAST, False), ("scale 2 fast", 2.0, L.DRAW_FAST, False), ("scale 2 soft", 2.0, L.DRAW_SOFT, False),
                                       ("overlay + scale 2 soft", 2.0, L.DRAW_SOFT, True)):
        cmds, cps = T.pack_text(labels(scale, mode))
        dcmds, dcps = torch.from_numpy(cmds.view(np.uint8).copy()).cuda(), torch.from_numpy(cps.view(np.int32).copy()).cuda()
        n, ncp = len(cmds), len(cps)

        def draw(stream, i, dcmds=dcmds, dcps=dcps, n=n, ncp=ncp, overlay=overlay):
            d = C.byref(descs[i % ROTATE])
            if overlay:
                L.check(lib.zg_canvas_draw(d, C.c_void_p(docmds.data_ptr()), len(ocmds), None, C.c_void_p(doverts.data_ptr()) if doverts is not None else None, len(overts), stream))
            L.check(lib.zg_canvas_draw_text(d, C.byref(dfont), C.c_void_p(dcmds.data_ptr()), n, None, C.c_void_p(dcps.data_ptr()), ncp, stream))

        replay, eager, reps = time_leg(torch, L, draw, args.reps)
        r = {"frame": "1080p", "pixel": "rgba_u8", "setting": name, "labels": n, "codepoints": ncp, "us_graph_replay": replay, "us_eager": eager, "reps": reps}
        print(json.dumps(r), flush=True)
        results.append(r)
    r = {"frame": "1080p", "pixel": "rgba_u8", "setting": "download + upload", "us_round_trip": time_round_trip(torch, frames, args.reps)}
    print(json.dumps(r), flush=True)
    results.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

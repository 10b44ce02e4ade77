"""Flood fill on the device: µs per zg_flood_fill on 1080p and 4096^2 frames of u8 and Rgba(u8), for three fills: sparse (a blob of
about a hundredth of the frame), dense (the whole frame is one region) and corridor (a one-pixel spiral through the whole frame: the
longest chains and the most unions across tiles). Timed with tools/bench_orb.py's time_leg: three rotating inputs, warm, HIP events
round a batch of calls, eager and as a replayed graph. The frames are two-valued, the threshold is 0 and the fill value is the region's
own value, so a fill writes the region and leaves the bytes as they were: the same call can be repeated without restoring the frame.

Beside every row, from the same run and the same frames: zg_copy (the floor for "read once, write the region") and zg_canny (whose
hysteresis stage is the same labelling).

usage: python tools/bench_flood.py [--reps N] [--json OUT] [--frame 1080p|4096] [--fill sparse|dense|corridor]     timing, one JSON line per leg
       python tools/bench_flood.py --kernels-only [--frame ...] [--fill ...]                                        a few eager calls per leg (what a kernel trace wraps)
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
WALL, FLOOR = 200, 50


def spiral(rows, cols):
    g = np.full((rows, cols), WALL, np.uint8)
    t, l, b, r = 0, 0, rows - 1, cols - 1
    while t <= b and l <= r:
        g[t, max(l - 2, 0):r + 1] = FLOOR
        g[t:b + 1, r] = FLOOR
        g[b, l:r + 1] = FLOOR
        g[t + 2:b + 1, l] = FLOOR
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
    return g


def planes(rows, cols):
    """{fill: (plane, seed)}: two-valued planes; the seed's region is FLOOR."""
    sparse = np.full((rows, cols), WALL, np.uint8)
    rr, cc = np.indices((rows, cols))
    sparse[(rr - rows // 2) ** 2 + (cc - cols // 2) ** 2 < rows * cols // 314] = FLOOR  # a disc of a hundredth of the frame
    return {"sparse": (sparse, (rows // 2, cols // 2)), "dense": (np.full((rows, cols), FLOOR, np.uint8), (rows // 2, cols // 2)),
            "corridor": (spiral(rows, cols), (0, 0))}


def typed(plane, pixel):
    if pixel == "u8":
        return plane
    out = np.empty(plane.shape + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = plane, 60, 30, 255
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--frame", default=None, choices=sorted(SHAPES))
    ap.add_argument("--fill", default=None, choices=("sparse", "dense", "corridor"))
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("bench_flood needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    rows_out = []
    for fname, (rows, cols) in SHAPES.items():
        if args.frame not in (None, fname):
            continue
        for pixel in ("u8", "rgba_u8"):
            for fill, (plane, seed) in planes(rows, cols).items():
                if args.fill not in (None, fill):
                    continue
                host = typed(plane, pixel)
                # rolling by whole rows keeps the spiral a spiral only for i = 0; the rotating inputs are copies at different addresses
                srcs = [zg.Image(torch.from_numpy(host).cuda()) for _ in range(ROTATE)]
                dst = zg.Image(torch.empty_like(srcs[0].data))
                edges = zg.Image(torch.empty((rows, cols), dtype=torch.uint8, device="cuda"))
                descs = [s._desc() for s in srcs]
                ddesc, edesc = dst._desc(), edges._desc()
                value = host[seed].tobytes()
                fill_value = (C.c_uint8 * len(value)).from_buffer_copy(value)
                opt = L.ZgFloodFillOptions(0.0, 4, L.FLOOD_MODE_SEED)
                count = torch.zeros(1, dtype=torch.int32, device="cuda")

                def flood(stream, i):
                    L.check(lib.zg_flood_fill(C.byref(descs[i % ROTATE]), seed[0], seed[1], None, fill_value, C.byref(opt), C.c_void_p(count.data_ptr()), stream))

                def copy(stream, i):
                    L.check(lib.zg_copy(C.byref(descs[i % ROTATE]), C.byref(ddesc), stream))

                def canny(stream, i):
                    L.check(lib.zg_canny(C.byref(descs[i % ROTATE]), C.byref(edesc), 1.0, 40.0, 120.0, stream))

                if args.kernels_only:
                    for i in range(ROTATE):
                        flood(None, i)
                    torch.cuda.synchronize()
                    continue
                base = {"frame": fname, "pixel": pixel, "fill": fill}
                replay, eager, reps = time_leg(torch, L, flood, args.reps)
                filled = int(count.cpu().numpy().view(np.uint32)[0])
                assert filled == int((plane == FLOOR).sum()) and all(np.array_equal(s.to_numpy(), host) for s in srcs)
                r = dict(base, leg="flood_fill", us_graph_replay=replay, us_eager=eager, reps=reps, filled=filled)
                for name, fn in (("copy", copy), ("canny", canny)):
                    if fill != "sparse" and args.fill is None and name == "canny":  # one canny per frame and pixel type is the yardstick: its time barely depends on the fill
                        continue
                    r[f"{name}_us_graph_replay"], r[f"{name}_us_eager"], _ = time_leg(torch, L, fn, args.reps)
                print(json.dumps(r), flush=True)
                rows_out.append(r)
                del srcs, dst, edges
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()

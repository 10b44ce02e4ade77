"""Quantisation and dithering on the device: µs per call of zg_color_histogram, zg_palette_lut and zg_dither (ordered, Floyd-Steinberg,
Atkinson) on 1080p and 4096^2 Rgb(u8) noise, and of zg_dither_frames on 16 and 64 frames of 1080p. Timed with tools/bench_orb.py's
time_leg: three rotating inputs, warm, HIP events round a batch of calls, eager and as a replayed graph. The palette is the fixed 6x7x6
one. Dithering works in place and its arithmetic takes the same instructions whatever the pixels hold, so the frames are dithered again
and again without being restored.

Two figures come with the timings:
  cpu_ratio     single-frame error diffusion against tools/dither_literal.c (the reference's loop, cc -O2, one thread) on this host;
  batch_ratio   the time per frame of the 16- and 64-frame batches relative to a single frame (one workgroup per frame: does it fill
                the device?).

usage: python tools/bench_quantize.py [--reps N] [--json OUT] [--frame 1080p|4096] [--no-cpu]     timing, one JSON line per leg
       python tools/bench_quantize.py --kernels-only                                              a few eager calls per leg (what a kernel trace wraps)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_orb import ROTATE, time_leg  # noqa: E402

SHAPES = {"1080p": (1080, 1920), "4096": (4096, 4096)}
MODES = {"ordered": 3, "floyd_steinberg": 1, "atkinson": 2}
BATCHES = (16, 64)


def cpu_literal(frame, palette, lut, atkinson):
    """ms of one call of tools/dither_literal.c on a copy of `frame`, best of three."""
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "dither_literal.so")
        subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "dither_literal.c")], check=True)
        fn = C.CDLL(so).dither_literal
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        fn.restype = None
        best = float("inf")
        for _ in range(3):
            work = frame.copy()
            t = time.perf_counter()
            fn(work.ctypes.data, frame.shape[0], frame.shape[1], palette.ctypes.data, lut.ctypes.data, int(atkinson))
            best = min(best, (time.perf_counter() - t) * 1e3)
        return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--frame", default=None, choices=sorted(SHAPES))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("bench_quantize needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    palette = zg.build_palette(zg.PaletteMode.fixed_6x7x6)
    lut_host = zg.palette_lut(palette)
    pal = torch.from_numpy(palette).cuda()
    lut = torch.from_numpy(lut_host).cuda()
    counts = torch.empty(L.HISTOGRAM_CELLS, dtype=torch.int32, device="cuda")
    first = torch.empty(L.HISTOGRAM_CELLS, dtype=torch.int32, device="cuda")
    p_ptr, l_ptr, n = C.c_void_p(pal.data_ptr()), C.c_void_p(lut.data_ptr()), len(palette)
    rows_out = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows_out.append(r)

    def run(base, fn, reps):
        if args.kernels_only:
            for i in range(ROTATE):
                fn(None, i)
            torch.cuda.synchronize()
            return None
        replay, eager, reps = time_leg(torch, L, fn, reps)
        r = dict(base, us_graph_replay=replay, us_eager=eager, reps=reps)
        return r

    single = {}
    for fname, (rows, cols) in SHAPES.items():
        if args.frame not in (None, fname):
            continue
        host = np.random.default_rng(5).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        frames = [zg.Image(torch.from_numpy(np.ascontiguousarray(np.roll(host, 37 * i, axis=1))).cuda()) for i in range(ROTATE)]
        descs = [f._desc() for f in frames]

        def histogram(stream, i):
            L.check(lib.zg_color_histogram(C.byref(descs[i % ROTATE]), C.c_void_p(counts.data_ptr()), C.c_void_p(first.data_ptr()), stream))

        def table(stream, i):
            L.check(lib.zg_palette_lut(p_ptr, n, l_ptr, stream))

        r = run({"frame": fname, "leg": "color_histogram"}, histogram, args.reps)
        if r:
            emit(r)
        if fname == next(iter(SHAPES)) or args.frame:
            r = run({"frame": "-", "leg": "palette_lut", "entries": n}, table, args.reps)
            if r:
                emit(r)
        for mname, mode in MODES.items():
            def dither(stream, i, mode=mode):
                L.check(lib.zg_dither(C.byref(descs[i % ROTATE]), p_ptr, n, l_ptr, mode, stream))

            r = run({"frame": fname, "leg": f"dither_{mname}"}, dither, args.reps if mname == "ordered" else max(ROTATE, args.reps // 5))
            if not r:
                continue
            single[(fname, mname)] = r["us_graph_replay"]
            if mname != "ordered" and not args.no_cpu:
                r["cpu_literal_ms"] = round(cpu_literal(host, palette, lut_host, mname == "atkinson"), 2)
                r["cpu_ratio"] = round(r["cpu_literal_ms"] * 1e3 / r["us_graph_replay"], 1)
            emit(r)
        del frames
    if args.frame in (None, "1080p"):
        rows, cols = SHAPES["1080p"]
        for count in BATCHES:
            host = np.random.default_rng(6).integers(0, 256, (count, rows, cols, 3), dtype=np.uint8)
            batches = [torch.from_numpy(host).cuda() for _ in range(ROTATE)]
            descs = [zg.Image(b[0])._desc() for b in batches]
            for mname in ("floyd_steinberg", "atkinson"):
                def dither_frames(stream, i, mode=MODES[mname]):
                    L.check(lib.zg_dither_frames(C.byref(descs[i % ROTATE]), count, rows * cols * 3, p_ptr, n, l_ptr, mode, stream))

                r = run({"frame": "1080p", "leg": f"dither_frames_{mname}", "frames": count}, dither_frames, ROTATE * 2)
                if not r:
                    continue
                r["us_per_frame"] = round(r["us_graph_replay"] / count, 2)
                if ("1080p", mname) in single:
                    r["batch_ratio"] = round(r["us_per_frame"] / single[("1080p", mname)], 4)
                emit(r)
            del batches
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()

"""The Hough transform on the device: µs per zg_hough_compute, per zg_hough_find_lines (threshold = max / 2 read on the device, NMS
5 / 5: the reference's hough_animation example) and per captured chain Canny -> clear -> compute -> max / 2 -> find_lines, on the
Canny output of a photo-like 1080p frame and of a sparse synthetic one, with size 300 (the example's) and 1024, the box centred.
compute and find_lines are timed with tools/bench_orb.py's time_leg (HIP events round a batch of calls over rotating inputs; graph
replay and eager), the chain as a torch.cuda.graph, since its maximum is a torch reduction. Beside every compute time: the votes
(edge pixels in the box x size) and the votes per second.

The voting form is chosen once per process: run again with ZIGNAL_HIP_HOUGH_DIRECT=1 in the environment for the direct form (every
row names its form; sizes above zg_hough_lds_max_size() take it anyway).

usage: python tools/bench_hough.py [--reps N] [--json OUT] [--size N]     timing, one JSON line per leg
       python tools/bench_hough.py --kernels-only [--size N]              a few eager calls per leg (what a kernel trace wraps)
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

SIZES = (300, 1024)
SHAPE = (1080, 1920)
CAPACITY = 4096


def frames():
    from oracle import pyoracle as oracle
    from tests.fast_ref import photo_like
    from tests.hough_cases import draw_line
    sparse = np.full(SHAPE, 30, np.uint8)
    rng = np.random.default_rng(3)
    for _ in range(12):  # long lines through the middle of the frame, where the boxes are
        r, c = SHAPE[0] // 2 + rng.integers(-120, 120), SHAPE[1] // 2 + rng.integers(-120, 120)
        a = rng.uniform(0, np.pi)
        dr, dc = 1200 * np.sin(a), 1200 * np.cos(a)
        draw_line(sparse, (r - dr, c - dc), (r + dr, c + dc), 220)
    sparse[440:600, 700:1300] = 200  # a bright rectangle: four straight edges
    return [("photo_1080p", photo_like(oracle.synth_u8(41, SHAPE))), ("sparse_1080p", sparse)]


def time_torch_graph(torch, fn, reps):
    """µs per call of fn() (one input per call, ROTATE of them) replayed from a torch.cuda.graph, and eager."""
    stream = torch.cuda.Stream()
    reps = max(ROTATE, reps // ROTATE * ROTATE)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.stream(stream):
        for i in range(2 * ROTATE):
            fn(i)
        ev[0].record(stream)
        for i in range(reps):
            fn(i)
        ev[1].record(stream)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for i in range(ROTATE):
            fn(i)
    with torch.cuda.stream(stream):
        for _ in range(3):
            graph.replay()
        ev[2].record(stream)
        for _ in range(reps // ROTATE):
            graph.replay()
        ev[3].record(stream)
    stream.synchronize()
    return round(ev[2].elapsed_time(ev[3]) * 1000.0 / reps, 2), round(ev[0].elapsed_time(ev[1]) * 1000.0 / reps, 2), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--size", type=int, default=None)
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("bench_hough needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    forced = os.environ.get("ZIGNAL_HIP_HOUGH_DIRECT", "") not in ("", "0")
    rows = []
    for fname, img in frames():
        srcs = [zg.Image(torch.from_numpy(np.ascontiguousarray(np.roll(img, 37 * i, axis=1))).cuda()) for i in range(ROTATE)]
        edges = [s.canny(1.0, 40, 120) for s in srcs]
        torch.cuda.synchronize()
        for size in SIZES:
            if args.size not in (None, size):
                continue
            form = "direct" if forced or size > lib.zg_hough_lds_max_size() else "lds"
            h = zg.HoughTransform(size)
            t, l = (SHAPE[0] - size) // 2, (SHAPE[1] - size) // 2
            box = (l, t, l + size, t + size)
            pixels = [int(np.count_nonzero(e.to_numpy()[t:t + size, l:l + size])) for e in edges]
            descs = [e._desc() for e in edges]
            acc = torch.zeros((size, size), dtype=torch.int32, device="cuda")
            accs = [h.compute(e, box) for e in edges]  # one accumulator per input for the find_lines leg
            thr = [torch.clamp(torch.div(a.max(), 2, rounding_mode="floor"), min=1).reshape(1).to(torch.int32) for a in accs]
            lines = torch.empty(CAPACITY * 28, dtype=torch.uint8, device="cuda")
            counts = torch.zeros(2, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def compute(stream, i):
                L.check(lib.zg_hough_compute(h._h, C.byref(descs[i % ROTATE]), *box, C.c_void_p(acc.data_ptr()), size, stream))

            def find(stream, i):
                L.check(lib.zg_hough_find_lines(h._h, C.c_void_p(accs[i % ROTATE].data_ptr()), size, 0, C.c_void_p(thr[i % ROTATE].data_ptr()), 5.0, 5.0, 65536,
                                                C.c_void_p(lines.data_ptr()), CAPACITY, C.c_void_p(counts.data_ptr()), stream))

            chain_edges = zg.Image(torch.zeros(SHAPE, dtype=torch.uint8, device="cuda"))
            chain_thr = torch.zeros(1, dtype=torch.int32, device="cuda")

            def chain(i):
                srcs[i % ROTATE].canny(1.0, 40, 120, out=chain_edges)
                acc.zero_()
                h.compute_into(chain_edges, acc, box)
                chain_thr.copy_(torch.clamp(torch.div(acc.max(), 2, rounding_mode="floor"), min=1).reshape(1))
                h.find_lines_into(acc, chain_thr, 5.0, 5.0, lines, counts, CAPACITY)

            if args.kernels_only:
                for i in range(ROTATE):
                    compute(None, i)
                    find(None, i)
                    chain(i)
                torch.cuda.synchronize()
                continue
            base = {"frame": fname, "size": size, "form": form}
            replay, eager, reps = time_leg(torch, L, compute, args.reps)
            votes = sum(pixels) / ROTATE * size
            r = dict(base, leg="compute", us_graph_replay=replay, us_eager=eager, reps=reps, edge_pixels=round(sum(pixels) / ROTATE), votes=round(votes),
                     gvotes_per_s=round(votes / replay / 1e3, 2))
            print(json.dumps(r), flush=True)
            rows.append(r)
            replay, eager, reps = time_leg(torch, L, find, args.reps)
            c = counts.cpu().numpy().view(np.uint32)
            r = dict(base, leg="find_lines", us_graph_replay=replay, us_eager=eager, reps=reps, candidates=int(c[0]), lines=int(c[1]))
            print(json.dumps(r), flush=True)
            rows.append(r)
            replay, eager, reps = time_torch_graph(torch, chain, max(args.reps // 3, ROTATE))
            c = counts.cpu().numpy().view(np.uint32)
            r = dict(base, leg="canny_clear_compute_max_find_lines", us_graph_replay=replay, us_eager=eager, reps=reps, candidates=int(c[0]), lines=int(c[1]))
            print(json.dumps(r), flush=True)
            rows.append(r)
            del h
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

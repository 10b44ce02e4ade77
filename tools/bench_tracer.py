"""Tracer on the device: ms per zg_trace_paths on 1080p and 4096^2 edge maps, timed with HIP events round single calls after a warm-up,
median of the repetitions (a trace is long enough for one call to be measured on its own). Cases: the Canny map of a photo-like frame
(tests/tracer_cases.py's, tiled to the size), 1 % noise, and at 1024^2 the serpentine, one path through half the pixels. Beside every
row, from the same run: the download of the edge map alone, into pinned and into pageable host memory (what a caller without a device
tracer pays before the CPU tracer can start), the number of raw paths and the longest one, and two partial times that bracket the stages:
raw (epsilon 0: no simplification) and min_path_length 10^9 (no path kept: labels, lists and the walk, nothing simplified or emitted).
The per-kernel times of one call come from a kernel trace of --kernels-only.

usage: python tools/bench_tracer.py [--reps N] [--json OUT] [--case NAME]     timing, one JSON line per case
       python tools/bench_tracer.py --kernels-only [--case NAME]              two eager calls per case (what a kernel trace wraps)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import tracer_cases as K  # noqa: E402

SHAPES = {"1080p": (1080, 1920), "4096": (4096, 4096)}


def tiled_photo(rows, cols):
    base = K.photo()
    return np.ascontiguousarray(np.tile(base, (rows // base.shape[0] + 1, cols // base.shape[1] + 1))[:rows, :cols])


def event_ms(torch, fn, reps, warmup=2):
    for _ in range(warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps = max(1, min(reps, int(2.0 / max(time.perf_counter() - t0, 1e-6))))  # a call of seconds is repeated less often: about 2 s a leg
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    if not torch.cuda.is_available():
        sys.exit("bench_tracer needs a GPU")
    cases = []
    for fname, (rows, cols) in SHAPES.items():
        cases.append((f"canny_photo_{fname}", "canny", rows, cols))
        cases.append((f"noise1pct_{fname}", "noise", rows, cols))
    cases.append(("serpentine_1024", "serpentine", 1024, 1024))
    out_rows = []
    for name, kind, rows, cols in cases:
        if args.case not in (None, name):
            continue
        if kind == "canny":
            edges = zg.Image(torch.zeros((rows, cols), dtype=torch.uint8, device="cuda"))
            zg.Image(torch.from_numpy(tiled_photo(rows, cols)).cuda()).canny(1.4, 10, 30, out=edges)
            edges = edges.data
        elif kind == "noise":
            edges = torch.from_numpy(K.noise(0.01, 1, (rows, cols))).cuda()
        else:
            edges = torch.from_numpy(K.serpentine(rows, cols)).cuda()
        torch.cuda.synchronize()
        n_edge = int((edges > 0).sum().item())
        points = torch.zeros(2 * max(n_edge, 1), dtype=torch.float32, device="cuda")
        offsets = torch.zeros(max(n_edge, 1) + 1, dtype=torch.int32, device="cuda")
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")

        def run(tracer):
            return lambda: tracer.trace_into(edges, points, offsets, counts, n_edge, n_edge)

        if args.kernels_only:
            run(zg.Tracer())()
            run(zg.Tracer())()
            torch.cuda.synchronize()
            continue
        run(zg.Tracer(0, 0.0))()
        c = counts.cpu().numpy().view(np.uint32)
        raw_paths = int(c[0])
        longest = int(np.diff(offsets[:raw_paths + 1].cpu().numpy().view(np.uint32)).max()) if raw_paths else 0
        row = {"case": name, "rows": rows, "cols": cols, "edge_pixels": n_edge, "raw_paths": raw_paths, "longest_raw_path": longest,
               "scratch_mb": round(zg.tracer.scratch_bytes(rows, cols) / 2 ** 20, 1)}
        for key, tracer in (("trace_ms", zg.Tracer()), ("trace_raw_ms", zg.Tracer(5, 0.0)), ("trace_nothing_kept_ms", zg.Tracer(10 ** 9, 1.0))):
            row[key], row[key + "_min"], row[key + "_max"] = (round(v, 3) for v in event_ms(torch, run(tracer), args.reps))
        run(zg.Tracer())()
        c = counts.cpu().numpy().view(np.uint32)
        row["paths"], row["points"] = int(c[0]), int(c[1])
        pinned = torch.empty((rows, cols), dtype=torch.uint8).pin_memory()
        row["download_pinned_ms"] = round(event_ms(torch, lambda: pinned.copy_(edges, non_blocking=True), args.reps)[0], 3)
        walls = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            edges.cpu()
            walls.append((time.perf_counter() - t0) * 1e3)
        row["download_pageable_ms"] = round(statistics.median(walls), 3)
        row["paths_download_ms"] = round(event_ms(torch, lambda: (points[:2 * row["points"]].cpu(), offsets[:row["paths"] + 1].cpu()), args.reps)[0], 3)
        print(json.dumps(row), flush=True)
        out_rows.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out_rows, f, indent=1)


if __name__ == "__main__":
    main()

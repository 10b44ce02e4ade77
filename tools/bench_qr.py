"""The QR detector on the device: microseconds per zg_qr_detect on a 1080p Image(u8) frame, timed with HIP events around many calls in a
row after a warm-up, over rotating copies of the frame and of the output buffers (so that no call finds its input in a cache because the
call before it read the same bytes), median of the repetitions. Scenes: one version-10 symbol at 6 pixels per module on a noisy grey
background (tests/qr_cases.py's planted matrix), as a binary map (mode 2: the detector alone) and as the grey frame through the adaptive
threshold (mode 0) and through Otsu (mode 1); and the same background with no symbol. Beside them, from the same run: the download plus
upload of the frame through pinned host memory, which is what doing the job on the host costs before any host detector has run.
Not measured here: other frame sizes, and the pathological frame with thousands of confirmed hits (the merge is one lane).

usage: python tools/bench_qr.py [--reps N] [--iters N] [--json OUT]     timing, one JSON line per scene
       python tools/bench_qr.py --kernels-only                          two eager calls per scene (what a kernel trace wraps)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import qr_cases as K  # noqa: E402

ROWS, COLS, VERSION, PX, COPIES = 1080, 1920, 10, 6, 4


def scene(with_symbol):
    if with_symbol:
        frame = K.render(K.matrix(VERSION), PX, ROWS, COLS, K.shift(700, 300), noise=20, seed=1)
    else:
        frame = K.render(np.zeros((21, 21), np.uint8), PX, ROWS, COLS, K.shift(-4000, -4000), noise=20, seed=1)
    return frame


def event_us(torch, fn, iters, reps):
    """fn(i) is call number i; the median, least and largest time per call over `reps` windows of `iters` calls."""
    for i in range(2 * COPIES):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import qr
    if not torch.cuda.is_available():
        sys.exit("bench_qr needs a GPU")
    detector = zg.QrDetector()
    rows_out = []
    for name, with_symbol in (("v10_6px", True), ("no_symbol", False)):
        gray = scene(with_symbol)
        binary = K.binarize(gray)
        for mode_name, mode, host in (("binary", qr.BINARY, binary), ("adaptive", qr.ADAPTIVE, gray), ("otsu", qr.OTSU, gray)):
            frames = [torch.from_numpy(np.array(host)).cuda() for _ in range(COPIES)]
            dets = [torch.zeros(qr.DETECTION_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(COPIES)]
            grids = [torch.zeros(16 * qr.GRID_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(COPIES)]
            modules = [torch.zeros(16 * 57 * 57, dtype=torch.uint8, device="cuda") for _ in range(COPIES)]

            def run(i, mode=mode, frames=frames, dets=dets, grids=grids, modules=modules):
                k = i % COPIES
                detector.detect_into(frames[k], dets[k], grids[k], modules[k], mode)

            if args.kernels_only:
                run(0)
                run(1)
                torch.cuda.synchronize()
                continue
            med, lo, hi = event_us(torch, run, args.iters, args.reps)
            record = dets[0].cpu().numpy().view(qr.DETECTION_DTYPE)[0]
            row = {"scene": name, "mode": mode_name, "rows": ROWS, "cols": COLS, "detect_us": round(med, 1), "detect_us_min": round(lo, 1), "detect_us_max": round(hi, 1),
                   "merged_finders": int(record["merged_count"]), "triple": int(record["triple_found"]), "fourths": int(record["fourth_count"]),
                   "versions": int(record["version_count"]), "grids": int(record["grids_total"]), "scratch_mb": round(qr.scratch_bytes(ROWS, COLS) / 2 ** 20, 1)}
            print(json.dumps(row), flush=True)
            rows_out.append(row)
    if not args.kernels_only:
        dev = [torch.from_numpy(scene(True)).cuda() for _ in range(COPIES)]
        pinned = [torch.empty((ROWS, COLS), dtype=torch.uint8).pin_memory() for _ in range(COPIES)]

        def round_trip(i):
            k = i % COPIES
            pinned[k].copy_(dev[k], non_blocking=True)
            dev[k].copy_(pinned[k], non_blocking=True)

        def download(i):
            k = i % COPIES
            pinned[k].copy_(dev[k], non_blocking=True)

        for key, fn in (("download_upload_pinned_us", round_trip), ("download_pinned_us", download)):
            med, lo, hi = event_us(torch, fn, args.iters, args.reps)
            row = {"scene": "round_trip", "rows": ROWS, "cols": COLS, key: round(med, 1), key + "_min": round(lo, 1), key + "_max": round(hi, 1)}
            print(json.dumps(row), flush=True)
            rows_out.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()

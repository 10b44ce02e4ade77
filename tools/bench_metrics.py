"""Image metrics on the device: µs per zg_psnr, zg_mean_pixel_error and zg_ssim on 1080p and 4096^2 frames of Rgba(u8) and f32, and per
zg_sum_f64_sequential on 2^24 terms at three chunk lengths and forced fully serial (an all-negative input). Timed with
tools/bench_orb.py's time_leg: three rotating input pairs, warm, HIP events round a batch of calls, eager and as a replayed graph. Beside
every metric: the seconds the CPU restatement (tests/metrics_ref.py, numpy f64) takes for the same frame, measured once (--no-cpu skips it;
SSIM's restatement is measured on the 1080p frames only, a 4096^2 frame takes 8.1 times as long).

usage: python tools/bench_metrics.py [--reps N] [--json OUT] [--frame 1080p|4096] [--no-cpu]     timing, one JSON line per leg
       python tools/bench_metrics.py --kernels-only [--frame ...]                                   a few eager calls per leg (what a kernel trace wraps)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_orb import ROTATE, time_leg  # noqa: E402

SHAPES = {"1080p": (1080, 1920), "4096": (4096, 4096)}
SUM_TERMS = 1 << 24


def frame_pair(pixel, rows, cols, seed):
    """A frame and a disturbed copy of it: what a blur or a codec leaves."""
    rng = np.random.default_rng(seed)
    if pixel == "rgba_u8":
        a = rng.integers(0, 256, (rows, cols, 4)).astype(np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    else:
        a = rng.random((rows, cols), np.float32)
        b = (a + (rng.random((rows, cols), np.float32) - np.float32(0.5)) * np.float32(0.05)).astype(np.float32)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--frame", default=None, choices=sorted(SHAPES))
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd.metrics import _record
    from tests import metrics_ref as R
    if not torch.cuda.is_available():
        sys.exit("bench_metrics needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    out = []

    def emit(r):
        print(json.dumps(r), flush=True)
        out.append(r)

    window = zg.ssim_window()
    for fname, (rows, cols) in SHAPES.items():
        if args.frame not in (None, fname):
            continue
        for pixel in ("rgba_u8", "f32"):
            hosts = [frame_pair(pixel, rows, cols, 10 + i) for i in range(ROTATE)]
            pairs = [(zg.Image(torch.from_numpy(a).cuda()), zg.Image(torch.from_numpy(b).cuda())) for a, b in hosts]
            descs = [(a._desc(), b._desc()) for a, b in pairs]
            res = torch.zeros(4 * ROTATE, dtype=torch.float64, device="cuda")
            for name in ("psnr", "mean_pixel_error", "ssim"):
                fn = getattr(lib, f"zg_{name}")

                def launch(stream, i, fn=fn):
                    k = i % ROTATE
                    L.check(fn(C.byref(descs[k][0]), C.byref(descs[k][1]), None, C.c_void_p(res.data_ptr() + 32 * k), stream))

                if args.kernels_only:
                    for i in range(ROTATE):
                        launch(None, i)
                    torch.cuda.synchronize()
                    continue
                replay, eager, reps = time_leg(torch, L, launch, args.reps)
                rec = _record(res)
                r = {"frame": fname, "pixel": pixel, "leg": name, "us_graph_replay": replay, "us_eager": eager, "reps": reps, "value": float(rec["value"]),
                     "serial_terms": int(rec["serial_terms"]), "terms": int(rec["count"])}
                a, b = hosts[0]
                if not args.no_cpu and (name != "ssim" or fname == "1080p"):
                    t0 = time.perf_counter()
                    want = {"psnr": R.mse, "mean_pixel_error": R.mean_pixel_error, "ssim": lambda x, y: R.ssim(x, y, window)}[name](a, b)
                    r["cpu_restatement_s"] = round(time.perf_counter() - t0, 3)
                    r["equal_bits"] = R.bits(want) == R.bits(float(rec["value"]))
                emit(r)
            del pairs
    if args.frame is None:
        rng = np.random.default_rng(3)
        inputs = {"uniform": rng.random(SUM_TERMS), "all_negative (fully serial)": -rng.random(SUM_TERMS)}
        for iname, host in inputs.items():
            devs = [torch.from_numpy(np.roll(host, 1001 * i)).cuda() for i in range(ROTATE)]
            res = torch.zeros(4 * ROTATE, dtype=torch.float64, device="cuda")
            for chunk_log2 in ((10, 12, 14) if iname == "uniform" else (12,)):

                def launch(stream, i, chunk_log2=chunk_log2):
                    k = i % ROTATE
                    L.check(lib.zg_sum_f64_sequential(C.c_void_p(devs[k].data_ptr()), SUM_TERMS, chunk_log2, C.c_void_p(res.data_ptr() + 32 * k), stream))

                if args.kernels_only:
                    for i in range(ROTATE):
                        launch(None, i)
                    torch.cuda.synchronize()
                    continue
                replay, eager, reps = time_leg(torch, L, launch, args.reps if iname == "uniform" else ROTATE)
                rec = _record(res)
                r = {"leg": "sum_f64_sequential", "input": iname, "terms": SUM_TERMS, "chunk": 1 << chunk_log2, "us_graph_replay": replay, "us_eager": eager,
                     "reps": reps, "serial_terms": int(rec["serial_terms"])}
                r["ns_per_serial_term"] = round(replay * 1000.0 / SUM_TERMS, 3) if iname != "uniform" else None
                if not args.no_cpu:
                    t0 = time.perf_counter()
                    want = R.left_to_right(host)
                    r["cpu_restatement_s"] = round(time.perf_counter() - t0, 3)
                    r["equal_bits"] = R.bits(want) == R.bits(float(rec["sum"]))
                emit(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""Order-statistic blurs on the device: µs per median_blur on a 4096^2 frame of u8 and of Rgba(u8), for the two kernels of
zignal_amd/csrc/order_stat.hip — k_order_stat (every window evaluated directly, radius 1..15) at r = 4, 8, 15 and k_order_stat_hist (a
sliding histogram per lane, radius 16..256) at r = 16, 32, 64, 127, 128, 256 — and for the sliding kernel at r = 4, 8, 15 through
ZIGNAL_HIP_ORDER_STAT_HIST_MIN=1. The hook is read once per process, so those three rows come from a child process of this tool. Timed with
tools/bench_orb.py's time_leg: three rotating inputs, warm, HIP events round a batch of calls, eager and as a replayed graph.

After the table the tool prints two checks (figures to report, not assertions):
  growth     t(r=64) / t(r=16) on the sliding kernel: work linear in r predicts 129 / 33 = 3.9, quadratic work 15.3; above 8 the kernel is
             not doing linear work.
  crossover  the direct kernel at r = 15, the largest radius it takes, against the sliding kernel at r = 16 on the same frame, and the
             three hook rows against the direct kernel at the same radius.

usage: python tools/bench_order_stat.py [--reps N] [--json OUT] [--pixel u8|rgba_u8] [--rows N --cols N]    timing, one JSON line per row
       python tools/bench_order_stat.py --kernels-only [...]                                                 one eager call per row (what a kernel trace wraps)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_orb import ROTATE, time_leg  # noqa: E402

DIRECT = (4, 8, 15)
SLIDING = (16, 32, 64, 127, 128, 256)
HOOK = "ZIGNAL_HIP_ORDER_STAT_HIST_MIN"
PIXELS = {"u8": (), "rgba_u8": (4,)}


def reps_for(radius, reps):
    """Fewer calls where one call is long: the sliding kernel's time grows with r and doubles again with the u32 counters."""
    return max(ROTATE, reps // max(1, radius // 8) // ROTATE * ROTATE)


def run_rows(args, radii, kernel):
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("bench_order_stat needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    rows = []
    for pixel, tail in PIXELS.items():
        if args.pixel not in (None, pixel):
            continue
        rng = np.random.default_rng(7)
        host = rng.integers(0, 256, (args.rows, args.cols) + tail).astype(np.uint8)
        inputs = [zg.Image(torch.from_numpy(np.ascontiguousarray(np.roll(host, 37 * i, axis=1))).cuda()) for i in range(ROTATE)]
        out = zg.Image(torch.empty_like(inputs[0].data))
        descs, od = [d._desc() for d in inputs], out._desc()
        for radius in radii:

            def launch(stream, i, radius=radius):
                L.check(lib.zg_order_statistic_blur(C.byref(descs[i % ROTATE]), C.byref(od), C.c_uint32(radius), 0, C.c_double(0.5), 2, stream))

            if not rows and not args.kernels_only:  # the process's first row: a few tens of milliseconds of work first, so that it is not timed on cold clocks
                for i in range(24):
                    launch(None, i)
                torch.cuda.synchronize()

            if args.kernels_only:
                launch(None, 0)
                torch.cuda.synchronize()
                continue
            replay, eager, reps = time_leg(torch, L, launch, reps_for(radius, args.reps))
            r = {"pixel": pixel, "rows": args.rows, "cols": args.cols, "radius": radius, "kernel": kernel, "us_graph_replay": replay, "us_eager": eager,
                 "reps": reps}
            print(json.dumps(r), flush=True)
            rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--pixel", default=None, choices=sorted(PIXELS))
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--cols", type=int, default=4096)
    ap.add_argument("--hook-rows", action="store_true", help="internal: the child process that runs the sliding kernel at the small radii")
    args = ap.parse_args()
    if args.hook_rows:
        assert os.environ.get(HOOK) == "1"
        run_rows(args, DIRECT, "k_order_stat_hist (hook)")
        return
    assert HOOK not in os.environ, f"{HOOK} is set: the default routing is what this process measures"
    rows = run_rows(args, DIRECT, "k_order_stat") + run_rows(args, SLIDING, "k_order_stat_hist")
    # the hook rows: a fresh process (the hook is read once), started once, with a time limit
    cmd = [sys.executable, os.path.abspath(__file__), "--hook-rows", "--reps", str(args.reps), "--rows", str(args.rows), "--cols", str(args.cols)]
    cmd += ["--pixel", args.pixel] if args.pixel else []
    cmd += ["--kernels-only"] if args.kernels_only else []
    child = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, **{HOOK: "1"}))
    if child.returncode != 0:
        sys.exit("the hook rows' process failed:\n" + child.stdout[-2000:] + child.stderr[-3000:])
    for line in child.stdout.splitlines():
        if line.startswith("{"):
            print(line, flush=True)
            rows.append(json.loads(line))
    if args.kernels_only:
        return
    t = {(r["pixel"], r["radius"], r["kernel"]): r["us_graph_replay"] for r in rows}
    for pixel in PIXELS:
        if args.pixel not in (None, pixel):
            continue
        t16, t64, t15 = t[(pixel, 16, "k_order_stat_hist")], t[(pixel, 64, "k_order_stat_hist")], t[(pixel, 15, "k_order_stat")]
        ratio = t64 / t16
        print(f"check growth    {pixel}: t(r=64) / t(r=16) = {t64:.0f} / {t16:.0f} us = {ratio:.2f} (linear work 3.9, quadratic 15.3): "
              + ("linear" if ratio <= 8.0 else "ABOVE 8: the sliding kernel is not doing linear work"))
        print(f"check crossover {pixel}: direct r=15 {t15:.0f} us, sliding r=16 {t16:.0f} us: the sliding kernel is "
              + (f"{t15 / t16:.2f}x faster" if t16 < t15 else f"NOT faster ({t16 / t15:.2f}x the time)"))
        for radius in DIRECT:
            d, s = t[(pixel, radius, "k_order_stat")], t[(pixel, radius, "k_order_stat_hist (hook)")]
            print(f"      hook      {pixel}: r={radius}: direct {d:.0f} us, sliding {s:.0f} us ({d / s:.2f}x)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

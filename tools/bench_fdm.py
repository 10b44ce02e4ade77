"""Feature distribution matching on the device: µs per call and bytes moved over the time, for a 4096 x 4096 Rgba(u8) and a 1080p Rgb(u8)
frame (seeded correlated noise), of
  moments            zg_fdm_compute_moments alone: the frame read once
  apply              zg_fdm_apply alone, colour route: the frame read once and written once
  match              zg_fdm_match against a target of the same size: source and target read for their moments, the source read and written
  match_frames x16   zg_fdm_match_frames over 16 frames against one target image: the target's statistics once
and, in the same run, a device-to-device copy of the frame (read once, written once) and the frame's download plus upload through pinned
memory (tools/bench_canvas.py's time_round_trip). Timed as tools/bench_canvas.py times its lists (tools/bench_orb.py's time_leg: rotating
frames, warm, HIP events round a batch of calls, eager and as a replayed graph). No time is a pass condition.

It also measures, on the CPU, the one departure from the reference's bits on the end-to-end test frames (tests/fdm_cases.py): how far the
exact-moment statistics move 255 * clamp(res), the value before @round, away from what Welford statistics give (tests/fdm_ref.py), and how
close any of those values comes to a tie.

usage: python tools/bench_fdm.py [--reps N] [--out profiles/fdm_bench.txt] [--no-gpu]
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

SEED = 11
FRAMES = (("4096x4096 rgba_u8", 4096, 4096, 4), ("1080p rgb_u8", 1080, 1920, 3))
BATCH = 16


def departure():
    """[(case, largest shift of the value before @round, smallest distance of a value to a tie, differing bytes)] on the CPU."""
    from tests import fdm_cases as K
    from tests import fdm_ref as R

    rows = []
    for name, src, tgt in K.end_to_end_cases():
        out, pre = R.apply(src, R.source_transform(src, R.prepare_target(tgt)), return_pre=True)
        out2, pre2 = K.match_with_exact_statistics(src, tgt, return_pre=True)
        rows.append((name, float(np.max(np.abs(pre - pre2))), float(np.min(np.abs((pre - np.floor(pre)) - 0.5))), int(np.sum(out != out2))))
    return rows


def correlated(rng, rows, cols, ch, base):
    z = rng.normal(size=(rows, cols, 3)).astype(np.float32)
    v = z @ rng.uniform(-1.0, 1.0, size=(3, 3)).astype(np.float32).T * 38.0 + np.asarray(base, np.float32)
    rgb = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return rgb if ch == 3 else np.dstack([rgb, np.full((rows, cols, 1), 255, np.uint8)])


def gpu_legs(reps):
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import fdm
    from bench_canvas import time_round_trip
    from bench_orb import ROTATE, time_leg
    lib = L.lib()
    L.check(lib.zg_init(0))
    results = []
    for label, rows, cols, ch in FRAMES:
        rng = np.random.default_rng(SEED)
        host = correlated(rng, rows, cols, ch, (110, 120, 100))
        target = zg.Image(torch.from_numpy(correlated(rng, rows, cols, ch, (90, 140, 70))).cuda())
        frames = [torch.from_numpy(np.roll(host, 37 * i, axis=1).copy()).cuda() for i in range(BATCH)]
        images = [zg.Image(f) for f in frames]
        descs = [im._desc() for im in images]
        batch = fdm._descs(images)
        td = target._desc()
        frame_bytes = rows * cols * ch
        moments = torch.zeros(ROTATE * C.sizeof(L.ZgFdmMoments), dtype=torch.uint8, device="cuda")
        # a transform of the colour route that a match of these frames gives: computed once, kept on the device
        matcher = zg.FeatureDistributionMatching().set_target(target)
        m0 = fdm.compute_moments(images[0])
        xform = torch.zeros(C.sizeof(L.ZgFdmTransform), dtype=torch.uint8, device="cuda")
        L.check(lib.zg_fdm_transform_from_moments(C.c_void_p(m0.data_ptr()), images[0].pixel, C.c_void_p(matcher._prepared.data_ptr()), C.c_void_p(xform.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert fdm._to_host(xform, L.ZgFdmTransform, 1)[0].route == L.FDM_ROUTE_COLOR

        def leg_moments(stream, i):
            L.check(lib.zg_fdm_compute_moments(C.byref(descs[i % ROTATE]), C.c_void_p(moments.data_ptr() + (i % ROTATE) * C.sizeof(L.ZgFdmMoments)), stream))

        def leg_apply(stream, i):
            L.check(lib.zg_fdm_apply(C.byref(descs[i % ROTATE]), C.c_void_p(xform.data_ptr()), stream))

        def leg_match(stream, i):
            L.check(lib.zg_fdm_match(C.byref(descs[i % ROTATE]), C.byref(td), stream))

        def leg_frames(stream, i):
            L.check(lib.zg_fdm_match_frames(batch, BATCH, C.byref(td), None, stream))

        def leg_copy(stream, i):
            frames[ROTATE + i % ROTATE].copy_(frames[i % ROTATE], non_blocking=True)

        for name, leg, moved, n in (("moments", leg_moments, frame_bytes, reps), ("apply", leg_apply, 2 * frame_bytes, reps),
                                    ("match", leg_match, 4 * frame_bytes, reps), (f"match_frames x{BATCH}", leg_frames, (3 * BATCH + 1) * frame_bytes, max(ROTATE, reps // 4)),
                                    ("device-to-device copy", leg_copy, 2 * frame_bytes, reps)):
            if leg is leg_copy:  # torch's copy, on torch's stream: eager only
                stream = torch.cuda.Stream()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                with torch.cuda.stream(stream):
                    for i in range(ROTATE):
                        leg(None, i)
                    ev[0].record(stream)
                    for i in range(n):
                        leg(None, i)
                    ev[1].record(stream)
                stream.synchronize()
                replay, eager, done = None, round(ev[0].elapsed_time(ev[1]) * 1000.0 / n, 2), n
            else:
                replay, eager, done = time_leg(torch, L, leg, n)
            best = replay if replay is not None else eager
            r = {"frame": label, "leg": name, "us_graph_replay": replay, "us_eager": eager, "reps": done, "bytes_moved": moved, "GB_per_s": round(moved / best / 1e3, 1)}
            print(json.dumps(r), flush=True)
            results.append(r)
        trip = time_round_trip(torch, frames, max(6, reps // 4))
        r = {"frame": label, "leg": "download + upload", "us_graph_replay": None, "us_eager": trip, "reps": max(6, reps // 4), "bytes_moved": 2 * frame_bytes,
             "GB_per_s": round(2 * frame_bytes / trip / 1e3, 1)}
        print(json.dumps(r), flush=True)
        results.append(r)
        del frames, images, target
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fdm_bench.txt"))
    ap.add_argument("--no-gpu", action="store_true", help="the CPU measurement only")
    args = ap.parse_args()
    lines = ["Feature distribution matching (tools/bench_fdm.py).", ""]
    rows = departure()
    lines += ["The departure from the reference's bits, measured on the CPU on the end-to-end test frames (tests/fdm_cases.py): statistics from exact",
              "moments (zg_fdm_stats_from_moments_host) against Welford statistics (tests/fdm_ref.py), everything after them the same restatement.",
              "shift: the largest change of 255 * clamp(res), the value before @round; tie: the smallest distance of such a value to a half-integer.", "",
              f"{'case':26s}{'shift':>12s}{'tie':>12s}  differing bytes"]
    for name, shift, tie, differ in rows:
        lines.append(f"{name:26s}{shift:12.3e}{tie:12.3e}  {differ}")
    worst = max(r[1] for r in rows)
    lines += ["", f"largest shift {worst:.3e}; the tests' tie guard is 100 times 5.4e-13 = 5.4e-11.", ""]
    print("\n".join(lines), flush=True)
    if not args.no_gpu:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_fdm needs a GPU (or --no-gpu)")
        results = gpu_legs(args.reps)
        lines += [f"Timings on one MI355X, one session, µs per call (--reps {args.reps}: rotating frames, warm, HIP events round a batch of calls). bytes: what the",
                  "call has to move at the least (reads and writes of the frames; the records are a few hundred bytes), GB/s: those over the better time.", "",
                  f"{'frame':20s}{'leg':24s}{'replayed graph':>16s}{'eager':>12s}{'MB moved':>12s}{'GB/s':>10s}"]
        for r in results:
            replay = "-" if r["us_graph_replay"] is None else f"{r['us_graph_replay']:.2f}"
            lines.append(f"{r['frame']:20s}{r['leg']:24s}{replay:>16s}{r['us_eager']:12.2f}{r['bytes_moved'] / 1e6:12.1f}{r['GB_per_s']:10.1f}")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

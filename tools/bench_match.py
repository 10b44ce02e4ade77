"""The matcher on the device: µs per zg_match_descriptors (with and without the cross-check), zg_match_knn (k = 2) and zg_match_radius
at 500 x 500, 2000 x 2000 and 10 000 x 10 000 clustered descriptors, and per graph of ORB on two 1080p frames followed by match —
timed with tools/bench_orb.py's time_leg (HIP events round a batch of calls over rotating inputs; graph replay and eager). Beside
every shape's times: the popcount floor 16 P / (256 CUs x 64 lanes x 2.4 GHz) for its P pairs, and the time of the numpy
restatement (tests/match_ref.py) on the host.

usage: python tools/bench_match.py [--reps N] [--json OUT] [--shape N] [--host-large]   timing, one JSON line per leg
       python tools/bench_match.py --kernels-only [--shape N]                           a few eager calls per leg (what a rocprofv3
                                                                                        --kernel-trace --stats run wraps)

--host-large also times the restatement at 10 000 x 10 000 (in blocks of 1000 queries; half a minute of host time).
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

SHAPES = (500, 2000, 10000)
RADIUS = 64.0  # about one entry per query on the clustered inputs (the leg reports the count)
CLOCK_HZ, CUS, LANES = 2.4e9, 256, 64


def floor_us(pairs: int) -> float:
    return 16.0 * pairs / (CUS * LANES * CLOCK_HZ) * 1e6


def host_us(R, q, t, cross: bool) -> float:
    """The numpy restatement of match on the host, in blocks of 1000 queries without the cross-check (it needs the whole matrix)."""
    t0 = time.perf_counter()
    if cross or len(q) <= 2000:
        R.match_fast(q, t, R.Params(cross_check=cross))
    else:
        for i in range(0, len(q), 1000):
            R.match_fast(q[i:i + 1000], t, R.Params())
    return (time.perf_counter() - t0) * 1e6


def shape_legs(torch, zg, L, R, n):
    """[(name, launch(stream, i))] for n x n descriptors: input set i % ROTATE."""
    lib = L.lib()
    sets = [R.clustered(900 + i, n, n) for i in range(ROTATE)]
    dq = [torch.from_numpy(R.bits(q).copy()).cuda() for q, _ in sets]
    dt = [torch.from_numpy(R.bits(t).copy()).cuda() for _, t in sets]
    qs = [L.ZgDescriptorSet(a.data_ptr(), n, None) for a in dq]
    ts = [L.ZgDescriptorSet(a.data_ptr(), n, None) for a in dt]
    d = R.distance_matrix(sets[0][0][:500], sets[0][1])
    per_query = float((d <= RADIUS).sum()) / 500.0
    cap = int(per_query * n * 2) + 1024
    out = torch.empty(max(n * 2, cap) * 12, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    plain, cross = L.ZgMatcherParams(0, 64, 0.8), L.ZgMatcherParams(1, 64, 0.8)
    o, r, c = C.c_void_p(out.data_ptr()), C.c_void_p(rows.data_ptr()), C.c_void_p(count.data_ptr())

    def match(p):
        return lambda stream, i: L.check(lib.zg_match_descriptors(C.byref(qs[i % ROTATE]), C.byref(ts[i % ROTATE]), C.byref(p), o, n, c, stream))

    def knn(stream, i):
        L.check(lib.zg_match_knn(C.byref(qs[i % ROTATE]), C.byref(ts[i % ROTATE]), C.byref(plain), 2, o, r, stream))

    def radius(stream, i):
        L.check(lib.zg_match_radius(C.byref(qs[i % ROTATE]), C.byref(ts[i % ROTATE]), RADIUS, o, cap, r, c, stream))

    keep = [sets, dq, dt, qs, ts, out, rows, count, plain, cross]
    return [("match", match(plain)), ("match_cross_check", match(cross)), ("knn_k2", knn), ("radius", radius)], sets, count, keep


def orb_match_leg(torch, zg, L):
    """ORB on two 1080p frames (a frame and its shift), then match on ORB's device arrays and count words."""
    from oracle import pyoracle as oracle
    lib = L.lib()
    base = oracle.synth_u8(41, (1080, 1920))
    orb, p = zg.Orb(), zg.Orb()._params()
    mp = L.ZgMatcherParams(1, 64, 0.8)
    frames, bufs = [], []
    for i in range(ROTATE):
        pair = [zg.Image(torch.from_numpy(np.ascontiguousarray(np.roll(base, (s, 37 * i + s), axis=(0, 1)))).cuda()) for s in (0, 3)]
        frames.append((pair, [f._desc() for f in pair]))
    for _ in range(2):
        bufs.append((torch.empty(500 * 28, dtype=torch.uint8, device="cuda"), torch.empty(500 * 32, dtype=torch.uint8, device="cuda"),
                     torch.zeros(1, dtype=torch.int32, device="cuda")))
    out = torch.empty(500 * 12, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    sets = [L.ZgDescriptorSet(des.data_ptr(), 500, n.data_ptr()) for _, des, n in bufs]

    def launch(stream, i):
        for d, (kps, des, n) in zip(frames[i % ROTATE][1], bufs):
            L.check(lib.zg_orb_detect_and_compute(C.byref(d), C.byref(p), C.c_void_p(kps.data_ptr()), C.c_void_p(des.data_ptr()), 500, C.c_void_p(n.data_ptr()), stream))
        L.check(lib.zg_match_descriptors(C.byref(sets[0]), C.byref(sets[1]), C.byref(mp), C.c_void_p(out.data_ptr()), 500, C.c_void_p(count.data_ptr()), stream))

    return launch, count, [frames, bufs, out, sets, orb, p, mp]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=600)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--shape", type=int, default=None, help="only this n (500, 2000, 10000); 0 for the ORB chain alone")
    ap.add_argument("--host-large", action="store_true")
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from tests import match_ref as R
    if not torch.cuda.is_available():
        sys.exit("bench_match needs a GPU")
    L.check(L.lib().zg_init(0))
    rows = []
    for n in SHAPES:
        if args.shape not in (None, n):
            continue
        legs, sets, count, keep = shape_legs(torch, zg, L, R, n)
        if args.kernels_only:
            for _, launch in legs:
                for i in range(ROTATE):
                    launch(None, i)
            torch.cuda.synchronize()
            continue
        for leg, launch in legs:
            replay, eager, reps = time_leg(torch, L, launch, args.reps)
            r = {"shape": f"{n}x{n}", "leg": leg, "us_graph_replay": replay, "us_eager": eager, "reps": reps, "entries": int(count.item()) if leg != "knn_k2" else None,
                 "popcount_floor_us": round(floor_us(n * n * (2 if leg == "match_cross_check" else 1)), 2)}
            if leg.startswith("match") and (n <= 2000 or (args.host_large and leg == "match")):
                r["numpy_host_us"] = round(host_us(R, *sets[0], leg == "match_cross_check"), 0)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del legs, keep
        torch.cuda.empty_cache()
    if args.shape in (None, 0):
        launch, count, keep = orb_match_leg(torch, zg, L)
        if args.kernels_only:
            for i in range(ROTATE):
                launch(None, i)
            torch.cuda.synchronize()
        else:
            replay, eager, reps = time_leg(torch, L, launch, max(args.reps // 10, ROTATE))
            r = {"shape": "2 x 1080p", "leg": "orb_orb_match_cross_check", "us_graph_replay": replay, "us_eager": eager, "reps": reps, "entries": int(count.item())}
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

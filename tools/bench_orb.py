"""ORB on the device: µs per zg_orb_detect_and_compute at the defaults (HIP events round a batch of calls over rotating inputs; graph
replay and eager), beside the two stages the library already had for the same frames: zg_pyramid_build and zg_fast_detect_batch on the
pyramid's levels with ORB's thresholds. What selection, orientation and descriptors cost is the difference.

usage: python tools/bench_orb.py [--reps N] [--json OUT] [--frame NAME]    timing, one JSON line per leg
       python tools/bench_orb.py --kernels-only [--frame NAME]             a few eager calls per frame (what a rocprofv3
                                                                           --kernel-trace --stats run wraps)

Frames: 1080p noise, the 4096^2 photo-like frame and 4096^2 noise of tests/test_gpu_orb.py:test_frames; three inputs per frame (the
frame and two of its shifts), one call on each in turn.
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

ROTATE = 3
KP_CAP = 1 << 22  # the FAST-only leg's keypoints per level


def frames():
    from oracle import pyoracle as oracle
    from tests.fast_ref import photo_like
    noise = oracle.synth_u8(32, (4096, 4096))
    return [("noise_1080p", oracle.synth_u8(41, (1080, 1920))), ("photo_4096", photo_like(noise)), ("noise_4096", noise)]


def build_legs(torch, zg, L, img):
    """[(name, launch(stream, i))] for one frame: input i % ROTATE."""
    lib = L.lib()
    orb = zg.Orb()
    inputs = [zg.Image(torch.from_numpy(np.ascontiguousarray(np.roll(img, 37 * i, axis=1))).cuda()) for i in range(ROTATE)]
    kps = torch.empty(500 * 28, dtype=torch.uint8, device="cuda")
    des = torch.empty(500 * 32, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = orb._params()
    descs = [d._desc() for d in inputs]

    def launch_orb(stream, i):
        L.check(lib.zg_orb_detect_and_compute(C.byref(descs[i % ROTATE]), C.byref(p), C.c_void_p(kps.data_ptr()), C.c_void_p(des.data_ptr()), 500,
                                              C.c_void_p(count.data_ptr()), stream))

    pyrs = [zg.ImagePyramid.build_default(d) for d in inputs]
    torch.cuda.synchronize()
    n = pyrs[0].n_levels
    lv = [(L.ZgImage * (n - 1))(*[l._desc() for l in pyr.levels[1:]]) for pyr in pyrs]
    sig = []
    for i in range(1, n):
        r, c, s = C.c_uint32(), C.c_uint32(), C.c_float()
        L.check(lib.zg_pyramid_level(inputs[0].rows, inputs[0].cols, C.c_float(lib.zg_pyramid_scale(C.c_float(1.2), i)), C.c_float(1.6), C.byref(r), C.byref(c), C.byref(s)))
        sig.append(s.value)
    sigmas = (C.c_float * (n - 1))(*sig)

    def launch_pyramid(stream, i):
        L.check(lib.zg_pyramid_build(C.byref(descs[i % ROTATE]), lv[i % ROTATE], sigmas, n - 1, stream))

    all_lv = [(L.ZgImage * n)(*[l._desc() for l in pyr.levels]) for pyr in pyrs]
    th = (C.c_uint32 * n)(*[orb.adaptive_threshold(l) for l in range(n)])
    caps = (C.c_uint32 * n)(*([KP_CAP // n] * n))
    offs = (C.c_uint64 * n)(*[l * (KP_CAP // n) for l in range(n)])
    fkps = torch.empty(KP_CAP * 28, dtype=torch.uint8, device="cuda")
    fcounts = torch.zeros(n, dtype=torch.int32, device="cuda")

    def launch_fast(stream, i):
        L.check(lib.zg_fast_detect_batch(all_lv[i % ROTATE], n, th, 9, 1, C.c_void_p(fkps.data_ptr()), caps, offs, C.c_void_p(fcounts.data_ptr()), stream))

    keep = [inputs, kps, des, count, p, descs, pyrs, lv, sigmas, all_lv, th, caps, offs, fkps, fcounts]
    return [("orb_detect_and_compute", launch_orb), ("pyramid_build", launch_pyramid), ("fast_detect_batch", launch_fast)], count, fcounts, keep


def time_leg(torch, L, launch, reps):
    """µs per call: eager, and as a replayed graph of ROTATE calls (one per input)."""
    lib = L.lib()
    stream = torch.cuda.Stream()
    h = C.c_void_p(stream.cuda_stream)
    reps = max(ROTATE, reps // ROTATE * ROTATE)
    with torch.cuda.stream(stream):
        for i in range(2 * ROTATE):
            launch(h, i)
    stream.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.stream(stream):
        ev[0].record(stream)
        for i in range(reps):
            launch(h, i)
        ev[1].record(stream)
    stream.synchronize()
    eager = ev[0].elapsed_time(ev[1]) * 1000.0 / reps
    with torch.cuda.stream(stream):
        L.check(lib.zg_graph_begin_capture(h))
        try:
            for i in range(ROTATE):
                launch(h, i)
        finally:
            g = C.c_void_p()
            rc = lib.zg_graph_end_capture(h, C.byref(g))
        L.check(rc)
    try:
        for _ in range(3):
            L.check(lib.zg_graph_launch(g, h))
        with torch.cuda.stream(stream):
            ev[2].record(stream)
            for _ in range(reps // ROTATE):
                L.check(lib.zg_graph_launch(g, h))
            ev[3].record(stream)
        stream.synchronize()
        replay = ev[2].elapsed_time(ev[3]) * 1000.0 / reps
    finally:
        L.check(lib.zg_graph_destroy(g))
    return round(replay, 2), round(eager, 2), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--frame", default=None, help="only this frame (noise_1080p, photo_4096, noise_4096)")
    args = ap.parse_args()
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("bench_orb needs a GPU")
    L.check(L.lib().zg_init(0))
    rows = []
    for name, img in frames():
        if args.frame not in (None, name):
            continue
        legs, count, fcounts, keep = build_legs(torch, zg, L, img)
        if args.kernels_only:
            for i in range(ROTATE):
                legs[0][1](None, i)
            torch.cuda.synchronize()
            continue
        for leg, launch in legs:
            replay, eager, reps = time_leg(torch, L, launch, args.reps)
            r = {"frame": name, "leg": leg, "us_graph_replay": replay, "us_eager": eager, "reps": reps}
            if leg == "orb_detect_and_compute":
                r["keypoints"] = int(count.item())
            if leg == "fast_detect_batch":
                r["corners_per_level"] = fcounts.cpu().numpy().tolist()
            print(json.dumps(r), flush=True)
            rows.append(r)
        del legs, keep
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

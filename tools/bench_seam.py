"""Seam carving on the device: µs per removed seam of zg_seam_carve at n = 1 and averaged over n = 64, on a 1080p and a 4096^2
Rgba(u8) frame of the benchmark's synthetic kind (oracle.synth_u8), the split by stage (zg_sobel, zg_seam_energy, zg_seam_find,
zg_seam_remove on the same frame) and, from the same run, the frame's download plus upload: what a caller without the device form pays
before any host work. Timed with tools/bench_orb.py's time_leg: three rotating inputs, warm, HIP events round a batch of calls, eager and
as a replayed graph. The two walks of k_seam_find are timed in processes of their own (the hook is read once per process).

usage: python tools/bench_seam.py [--reps N] [--out FILE] [--frame 1080p|4096]      every leg, one JSON line each; FILE also gets them
       python tools/bench_seam.py --one-process [...]                               this process's walk only (what the above starts twice)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_orb import ROTATE, time_leg  # noqa: E402

SHAPES = {"1080p": (1080, 1920), "4096": (4096, 4096)}
HOOK = "ZIGNAL_HIP_SEAM_PLAIN_WALK"


def one_process(args):
    import torch
    import zignal_amd as zg
    from oracle import pyoracle as oracle
    from zignal_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("bench_seam needs a GPU")
    lib = L.lib()
    L.check(lib.zg_init(0))
    walk = "plain" if os.environ.get(HOOK) == "1" else "staged"
    for fname, (rows, cols) in SHAPES.items():
        if args.frame not in (None, fname):
            continue
        host = oracle.synth_u8(5, (rows, cols, 4))
        srcs = [zg.Image(torch.from_numpy(np.ascontiguousarray(np.roll(host, 37 * i, axis=1))).cuda()) for i in range(ROTATE)]
        descs = [s._desc() for s in srcs]
        edges = zg.Image(torch.empty((rows, cols), dtype=torch.uint8, device="cuda"))
        energy = torch.empty(rows * cols, dtype=torch.int32, device="cuda")
        seam = torch.empty(rows, dtype=torch.int32, device="cuda")
        edesc = edges._desc()
        ep, sp = C.c_void_p(energy.data_ptr()), C.c_void_p(seam.data_ptr())
        base = {"frame": fname, "pixel": "rgba_u8", "walk": walk}

        def emit(leg, launch, reps, per=1):
            replay, eager, reps = time_leg(torch, L, launch, reps)
            row = dict(base, leg=leg, us_graph_replay=round(replay / per, 2), us_eager=round(eager / per, 2), reps=reps)
            print(json.dumps(row), flush=True)

        if walk == "staged":  # the stages the hook does not touch are timed once
            emit("sobel", lambda s, i: L.check(lib.zg_sobel(C.byref(descs[i % ROTATE]), C.byref(edesc), s)), args.reps)
            emit("seam_energy", lambda s, i: L.check(lib.zg_seam_energy(C.byref(edesc), ep, s)), args.reps)
        else:
            L.check(lib.zg_sobel(C.byref(descs[0]), C.byref(edesc), None))
            L.check(lib.zg_seam_energy(C.byref(edesc), ep, None))
        emit("seam_find", lambda s, i: L.check(lib.zg_seam_find(ep, rows, cols, sp, s)), args.reps)
        if walk == "staged":
            one = zg.Image(torch.empty((rows, cols - 1, 4), dtype=torch.uint8, device="cuda"))
            odesc = one._desc()
            emit("seam_remove", lambda s, i: L.check(lib.zg_seam_remove(C.byref(descs[i % ROTATE]), sp, C.byref(odesc), s)), args.reps)
        for n, reps in ((1, args.reps), (64, max(ROTATE, args.reps // 10))):
            out = zg.Image(torch.empty((rows, cols - n, 4), dtype=torch.uint8, device="cuda"))
            d = out._desc()
            emit(f"seam_carve_n{n}_per_seam", lambda s, i: L.check(lib.zg_seam_carve(C.byref(descs[i % ROTATE]), C.byref(d), n, 0, None, None, s)), reps, per=n)
        if walk == "staged":
            # the round trip a caller of a host-only implementation pays: pageable memory, as an image library's caller holds it
            dev = srcs[0].data
            torch.cuda.synchronize()
            best = None
            for _ in range(5):
                t0 = time.perf_counter()
                back = dev.cpu()
                dev.copy_(back)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e6
                best = dt if best is None else min(best, dt)
            print(json.dumps(dict(base, leg="download_plus_upload", us_best_of_5=round(best, 1), bytes=int(host.nbytes))), flush=True)
        del srcs, edges, energy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frame", default=None, choices=sorted(SHAPES))
    ap.add_argument("--one-process", action="store_true")
    args = ap.parse_args()
    if args.one_process:
        return one_process(args)
    lines = []
    for hook in ("0", "1"):  # a fresh child each: the hook is a function-local static of the library
        cmd = [sys.executable, os.path.abspath(__file__), "--one-process", "--reps", str(args.reps)] + (["--frame", args.frame] if args.frame else [])
        res = subprocess.run(cmd, env=dict(os.environ, **{HOOK: hook}), capture_output=True, text=True, timeout=900)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            sys.exit(res.stderr[-4000:])
        lines += [l for l in res.stdout.splitlines() if l.startswith("{")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

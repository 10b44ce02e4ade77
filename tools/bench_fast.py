"""FAST on the device: µs per call (HIP events; graph replay and eager), keypoint counts, and with --pmc the counters of the kernels.

usage: python tools/bench_fast.py [--reps N] [--json OUT]              timing, one JSON line per leg
       python tools/bench_fast.py --kernels-only [--leg NAME]           a few eager calls per leg (what a rocprofv3 --pmc run wraps)
       python tools/bench_fast.py --pmc "FETCH_SIZE WRITE_SIZE" --dir D  a rocprofv3 --kernel-trace --stats pass, then one --pmc pass per
                                                                        counter, each over --kernels-only; per-kernel means

Frames: the 4096^2 field-plus-noise frame of tests/test_next_rows.py:test_detectors_at_frame_sizes, a 4096^2 synth_u8 noise plane and a
1080p grey frame, NMS on and off; and ORB's default pyramid (8 levels, 1.2, sigma 1.6) of the 4096^2 photo-like frame through
zg_fast_detect_batch with ORB's per-level thresholds (orb.zig:511-517).
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KP_CAP = 1 << 22


def orb_thresholds(n, t=20, f=1.2):
    return [int(np.round(np.clip(np.float32(t) * (np.float32(1) / np.float32(f) ** np.float32(i)), 5, 255))) for i in range(n)]


def frames():
    from oracle import pyoracle as oracle
    from tests.fast_ref import photo_like
    noise = oracle.synth_u8(32, (4096, 4096))
    return [("photo_4096", photo_like(noise)), ("noise_4096", noise), ("grey_1080p", oracle.synth_u8(41, (1080, 1920)))]


class Leg:
    """One captured call (or batch) and its eager twin."""

    def __init__(self, name, launch):
        self.name, self.launch = name, launch


def build_legs(torch, zg, L):
    lib = L.lib()
    kps = torch.empty(KP_CAP * 28, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(16, dtype=torch.int32, device="cuda")
    legs, keep = [], []
    for name, img in frames():
        dev = zg.Image(torch.from_numpy(np.ascontiguousarray(img)).cuda())
        keep.append(dev)
        for nms in (1, 0):
            d = dev._desc()
            keep.append(d)

            def launch(stream, d=d, nms=nms):
                L.check(lib.zg_fast_detect(C.byref(d), 20, 9, nms, C.c_void_p(kps.data_ptr()), KP_CAP, C.c_void_p(counts.data_ptr()), stream))
            legs.append(Leg(f"{name}_{'nms' if nms else 'raw'}", launch))
    src = keep[0]
    pyr = zg.ImagePyramid.build_default(src)
    torch.cuda.synchronize()
    n = pyr.n_levels
    descs = (L.ZgImage * n)(*[lv._desc() for lv in pyr.levels])
    th = (C.c_uint32 * n)(*orb_thresholds(n))
    caps = (C.c_uint32 * n)(*([KP_CAP // n] * n))
    offs = (C.c_uint64 * n)(*[i * (KP_CAP // n) for i in range(n)])
    keep += [pyr, descs, th, caps, offs]

    def launch_batch(stream):
        L.check(lib.zg_fast_detect_batch(descs, n, th, 9, 1, C.c_void_p(kps.data_ptr()), caps, offs, C.c_void_p(counts.data_ptr()), stream))
    legs.append(Leg("orb_pyramid_batch_nms", launch_batch))
    return legs, counts, keep


def time_leg(torch, L, leg, counts, reps):
    lib = L.lib()
    stream = torch.cuda.Stream()
    h = C.c_void_p(stream.cuda_stream)
    with torch.cuda.stream(stream):
        for _ in range(3):
            leg.launch(h)
    stream.synchronize()
    n = counts[:8].cpu().numpy().tolist()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.cuda.stream(stream):
        ev[0].record(stream)
        for _ in range(reps):
            leg.launch(h)
        ev[1].record(stream)
    stream.synchronize()
    eager = ev[0].elapsed_time(ev[1]) * 1000.0 / reps
    with torch.cuda.stream(stream):
        L.check(lib.zg_graph_begin_capture(h))
        leg.launch(h)
        g = C.c_void_p()
        L.check(lib.zg_graph_end_capture(h, C.byref(g)))
    try:
        for _ in range(3):
            L.check(lib.zg_graph_launch(g, h))
        with torch.cuda.stream(stream):
            ev[2].record(stream)
            for _ in range(reps):
                L.check(lib.zg_graph_launch(g, h))
            ev[3].record(stream)
        stream.synchronize()
        replay = ev[2].elapsed_time(ev[3]) * 1000.0 / reps
    finally:
        L.check(lib.zg_graph_destroy(g))
    return {"leg": leg.name, "us_graph_replay": round(replay, 2), "us_eager": round(eager, 2),
            "keypoints": n if leg.name.startswith("orb") else n[0], "reps": reps}


def _profile(args, extra, tag):
    """rocprofv3 <extra> over a fresh child running --kernels-only; returns the output directory of that pass."""
    d = os.path.join(args.dir, tag)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", *extra, "-d", d, "-o", "r", "--", sys.executable, os.path.abspath(__file__), "--kernels-only"] + (["--leg", args.leg] if args.leg else [])
    rc = subprocess.run(cmd, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT).returncode
    if rc != 0:
        sys.exit(f"rocprofv3 {' '.join(extra)}: exit status {rc}")
    return d


def _kernel(name):
    m = re.search(r"k_fast_\w+", name)
    return m.group(0) if m else name


def pmc(args):
    """Counters of the FAST kernels, ONE counter per rocprofv3 --pmc pass (each a fresh child, nothing but the kernel trace beside
    it), plus a --kernel-trace --stats pass for the durations; per-kernel means over every dispatch of the --kernels-only run."""
    out = defaultdict(dict)
    d = _profile(args, ["--kernel-trace", "--stats", "--output-format", "csv"], "trace")
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        for row in csv.DictReader(open(f)):
            if "fast" in row.get("Name", ""):
                out[_kernel(row["Name"])]["avg_us"] = round(float(row["AverageNs"]) / 1000.0, 2)
                out[_kernel(row["Name"])]["calls"] = int(row["Calls"])
    print(json.dumps({"trace": out}), flush=True)
    for ctr in args.pmc.split():
        d = _profile(args, ["--kernel-trace", "--pmc", ctr], "pmc_" + ctr)
        acc = defaultdict(list)
        for db in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
            c = sqlite3.connect(db)
            for k, name, v in c.execute("select kernel_name, counter_name, value from counters_collection"):
                if "fast" in k:
                    acc[_kernel(k)].append(v)
        for k, v in acc.items():
            out[k][ctr] = sum(v) / len(v)
        print(json.dumps({ctr: {k: out[k].get(ctr) for k in acc}}), flush=True)
    print(json.dumps({"pmc": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--pmc", default=None)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "bench_fast_pmc"), help="where rocprofv3 writes its passes")
    ap.add_argument("--leg", default=None, help="only this leg (e.g. photo_4096_nms)")
    args = ap.parse_args()
    if args.pmc:
        return pmc(args)
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("bench_fast needs a GPU")
    L.check(L.lib().zg_init(0))
    legs, counts, keep = build_legs(torch, zg, L)
    legs = [leg for leg in legs if args.leg in (None, leg.name)]
    if args.kernels_only:
        for leg in legs:
            for _ in range(3):
                leg.launch(None)
        torch.cuda.synchronize()
        return
    rows = []
    for leg in legs:
        r = time_leg(torch, L, leg, counts, args.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

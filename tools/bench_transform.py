"""Geometry fitting on the device (include/zignal_hip_transform.h): µs per call on one GPU of
  fit                zg_transform_fit_points at N = 500 and N = 4096 for each kind and scalar type, as a replayed graph and eager (tools/bench_orb.py's
                     time_leg: three rotating inputs, warm, HIP events round a batch), with the library's default and with each form the tuning hook
                     ZIGNAL_HIP_FIT_VARIANT selects (1: projective's 9 x 9 SVD on one lane instead of through the workgroup; 2: the SVD's dot
                     products multiplied and added by one lane instead of staged through LDS; 3: both). The hook is read once per process, so
                     every variant is a child process of this tool.
  chain              ORB twice, match with cross-check, fit (similarity, f64), warp on 1080p Image(u8) frames: the device chain (nothing but
                     enqueues; as a replayed graph, and by the wall clock from the first enqueue to the stream's end) against the same chain with
                     the fit on the host (ORB twice and match on the device, the download of the count, the matches and both keypoint arrays,
                     zg_transform_fit_matches_host, zg_warp), by the wall clock; and the stages alone.
No time is a pass condition.

usage: python tools/bench_transform.py [--reps N] [--out profiles/transform_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ((0, "similarity"), (1, "affine"), (2, "projective"))
SCALARS = ((0, "f32"), (1, "f64"))
SIZES = (500, 4096)
VARIANTS = ((0, "default"), (1, "9x9 SVD on one lane"), (2, "unstaged dot products"), (3, "both"))
CAP = 500


def fit_legs(reps):
    """[(kind, scalar, n, replay µs, eager µs)] in this process (whatever ZIGNAL_HIP_FIT_VARIANT it was started with)."""
    import torch
    from zignal_amd import _lib as L
    from zignal_amd import transform as TF
    from tests import transform_cases as K
    from bench_orb import ROTATE, time_leg
    L.check(L.lib().zg_init(0))
    rows = []
    for kind, _ in KINDS:
        for scalar, _ in SCALARS:
            for n in SIZES:
                pts = [[torch.from_numpy(a).cuda() for a in K.cloud(kind, scalar, n, seed=i)] for i in range(ROTATE)]
                recs = [TF.new_record() for _ in range(ROTATE)]
                replay, eager, _ = time_leg(torch, L, lambda h, i: TF.fit_points_into(kind, pts[i % ROTATE][0], pts[i % ROTATE][1], recs[i % ROTATE]), reps)
                torch.cuda.synchronize()
                assert all(int(TF.record_to_host(r)["status"]) == L.FIT_OK for r in recs)
                rows.append((kind, scalar, n, replay, eager))
    return rows


def host_fit_times():
    """[(kind, scalar, µs)] of zg_transform_fit_points_host at N = 500 on the CPU this runs on, by the wall clock."""
    from zignal_amd import transform as TF
    from tests import transform_cases as K
    rows = []
    for kind, _ in KINDS:
        for scalar, _ in SCALARS:
            f, t = K.cloud(kind, scalar, 500)
            TF.fit_points_host(kind, f, t)
            t0 = time.perf_counter()
            for _ in range(100):
                TF.fit_points_host(kind, f, t)
            rows.append((kind, scalar, round((time.perf_counter() - t0) * 1e6 / 100, 1)))
    return rows


def chain_legs(reps):
    import torch
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import transform as TF
    from oracle import pyoracle as oracle
    from tests import fast_ref as F
    from bench_orb import ROTATE, time_leg
    L.check(L.lib().zg_init(0))
    rows_, cols_ = 1080, 1920
    kp, ma = zg.KEYPOINT_DTYPE.itemsize, zg.MATCH_DTYPE.itemsize
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    sets = []
    for i in range(ROTATE):
        base = F.photo_like(oracle.synth_u8(1300 + i, (rows_, cols_)))
        a = zg.Image(torch.from_numpy(base).cuda())
        ang = np.deg2rad(2.0 + i)
        m = 1.02 * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        centre = np.array([cols_ / 2, rows_ / 2])
        b = a.warp(zg.SimilarityTransform(m, centre - m @ centre + (6.0, -4.0)), (rows_, cols_), zg.Interpolation.bilinear)
        sets.append(dict(a=a, b=b, out=zg.Image(z((rows_, cols_))), kps=[z(CAP * kp), z(CAP * kp)], des=[z(CAP * 32), z(CAP * 32)], counts=[z(1, torch.int32), z(1, torch.int32)],
                         matches=z(CAP * ma), n=z(1, torch.int32), rec=TF.new_record()))
    orb, matcher = zg.Orb(), zg.BruteForceMatcher(cross_check=True)

    def features(s):
        for img, k, d, c in zip((s["a"], s["b"]), s["kps"], s["des"], s["counts"]):
            orb.detect_and_compute_into(img, k, d, c, CAP)
        matcher.match_into(s["des"][0], s["des"][1], s["matches"], s["n"], CAP, query_count=s["counts"][0], train_count=s["counts"][1])

    def fit(s):
        TF.fit_matches_into(TF.SIMILARITY, L.SCALAR_F64, s["kps"][0], s["kps"][1], s["matches"], s["rec"], count=s["n"], capacity=CAP)

    def warp(s):
        TF.warp_fitted(s["b"], s["rec"], s["out"], zg.Interpolation.bilinear)

    def device_chain(s):
        features(s)
        fit(s)
        warp(s)

    class M32:
        def __init__(self, r):
            self.kind, self.m = int(r["kind"]), np.array(r["m32"])

        def coefficients(self):
            return self.m[:6]

    def host_chain(s):
        features(s)
        n = int(s["n"].item())  # waits for the stream
        r = TF.fit_matches_host(TF.SIMILARITY, L.SCALAR_F64, s["kps"][0].cpu().numpy(), s["kps"][1].cpu().numpy(), s["matches"][:n * ma].cpu().numpy())
        s["b"].warp(M32(r), s["out"], zg.Interpolation.bilinear)
        return r

    out = {}
    for name, fn in (("orb x 2 + match", features), ("fit from matches", fit), ("warp_fitted", warp), ("device chain", device_chain)):
        replay, eager, _ = time_leg(torch, L, lambda h, i, fn=fn: fn(sets[i % ROTATE]), reps)
        out[name] = (replay, eager)
    torch.cuda.synchronize()
    points = [int(TF.record_to_host(s["rec"])["n_points"]) for s in sets]
    statuses = [int(TF.record_to_host(s["rec"])["status"]) for s in sets]

    def wall(fn):
        for i in range(2 * ROTATE):
            fn(sets[i % ROTATE])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            fn(sets[i % ROTATE])
            torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e6 / reps, 1)
    out["device chain, wall clock, a synchronisation per frame pair"] = (wall(device_chain), None)
    out["chain with the fit on the host, wall clock"] = (wall(host_chain), None)
    # the host fit alone, and the downloads alone
    s = sets[0]
    torch.cuda.synchronize()
    n = int(s["n"].item())
    k0, k1, mm = s["kps"][0].cpu().numpy(), s["kps"][1].cpu().numpy(), s["matches"][:n * ma].cpu().numpy()
    t0 = time.perf_counter()
    for _ in range(200):
        TF.fit_matches_host(TF.SIMILARITY, L.SCALAR_F64, k0, k1, mm)
    out["zg_transform_fit_matches_host alone"] = (round((time.perf_counter() - t0) * 1e6 / 200, 1), None)
    t0 = time.perf_counter()
    for _ in range(200):
        int(s["n"].item())
        s["kps"][0].cpu(), s["kps"][1].cpu(), s["matches"][:n * ma].cpu()
    out["download of the count, the matches and both keypoint arrays"] = (round((time.perf_counter() - t0) * 1e6 / 200, 1), None)
    return out, points, statuses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_bench.txt"))
    ap.add_argument("--fits-json", action="store_true", help="(internal) time the fit legs in this process and print them as JSON")
    args = ap.parse_args()
    if args.fits_json:
        print("FITS " + json.dumps(fit_legs(args.reps)))
        return
    lines = ["tools/bench_transform.py: one MI355X, µs per call; replay = a replayed graph of three calls on rotating inputs, eager = the same calls enqueued one by one",
             "", "fit: zg_transform_fit_points (one workgroup of 256 lanes a fit)", ""]
    tables = {}
    for variant, label in VARIANTS:
        env = dict(os.environ, ZIGNAL_HIP_FIT_VARIANT=str(variant))
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--fits-json", "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        got = [ln for ln in child.stdout.splitlines() if ln.startswith("FITS ")]
        if child.returncode != 0 or not got:
            raise SystemExit(f"variant {variant}: {child.stdout[-2000:]}{child.stderr[-4000:]}")
        tables[variant] = {(k, s, n): (r, e) for k, s, n, r, e in json.loads(got[0][5:])}
    lines.append(f"{'kind':<11} {'T':<4} {'N':>5}   " + "   ".join(f"{label + ' (replay)':>40}" for _, label in VARIANTS) + f"   {'default (eager)':>16}")
    for kind, kname in KINDS:
        for scalar, sname in SCALARS:
            for n in SIZES:
                cells = "   ".join(f"{tables[v][(kind, scalar, n)][0]:>40.2f}" for v, _ in VARIANTS)
                lines.append(f"{kname:<11} {sname:<4} {n:>5}   {cells}   {tables[0][(kind, scalar, n)][1]:>16.2f}")
    lines += ["", "the same fit on the host at N = 500 (zg_transform_fit_points_host, one CPU thread, wall clock): "
              + ", ".join(f"{KINDS[k][1]} {SCALARS[s][1]} {us}" for k, s, us in host_fit_times())]
    chain, points, statuses = chain_legs(min(args.reps, 60))
    lines += ["", f"chain: 1080p Image(u8) frames, ORB (500 features) twice, match with cross-check, similarity fit in f64, bilinear warp; the fits ran on {points} matches, statuses {statuses}", ""]
    lines.append(f"{'':<66} {'replay':>10} {'eager':>10}")
    for name, (a, b) in chain.items():
        lines.append(f"{name:<66} {a:>10.1f} " + (f"{b:>10.1f}" if b is not None else f"{'':>10}"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

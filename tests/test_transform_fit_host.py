"""zignal_amd/csrc/zg_transform_fit.h on the CPU: tests/c/transform_fit.cpp includes only that header, is built with plain g++ under
-fsanitize=address,undefined with the two HIP qualifiers defined away and -ffp-contract=off, and prints the bits of every record for the
point sets of tests/transform_cases.py (at least 300 per kind and scalar type: random fits, exact maps and noise, reflections, duplicated,
all-equal and collinear points, N at each minimum, affine at 85 and 86 points, coordinates at 1e-20 and 1e+15), which must equal
tests/transform_ref.py's bit for bit. The library's _host forms are held to the same cases. Nothing is loaded into python under a
sanitizer."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import transform_cases as K
from tests import transform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "transform_fit.cpp")
BIN = os.path.join(ROOT, "tests", "c", "transform_fit")
KINDS, SCALARS = (0, 1, 2), (0, 1)


def _hex(v, scalar) -> str:
    if scalar == 0:
        return "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _points(T, a):
    return [(T(p[0]), T(p[1])) for p in a.tolist()]


@pytest.fixture(scope="module")
def program():
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__host__=", "-D__device__=", "-o", BIN, SRC], check=True)

    def run(lines):
        out = subprocess.run([BIN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and f"transform fit ok {len(lines)}" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        return out.stdout.splitlines()[:-1]
    return run


@pytest.fixture(scope="module")
def restated():
    """(kind, scalar) -> [(status, the nine values as hex)] from the restatement, computed once for both tests."""
    out = {}
    with np.errstate(all="ignore"):
        for kind in KINDS:
            for scalar in SCALARS:
                T = R.F32 if scalar == 0 else R.F64
                out[kind, scalar] = [(lambda st, m: (st, [_hex(v, scalar) for v in m]))(*R.fit(T, kind, _points(T, f), _points(T, t)))
                                     for _, f, t in K.fit_cases(kind, scalar)]
    return out


@pytest.mark.parametrize("scalar", SCALARS)
@pytest.mark.parametrize("kind", KINDS)
def test_record_bits_equal_the_restatement(program, restated, kind, scalar):
    cases = K.fit_cases(kind, scalar)
    assert len(cases) >= 300
    lines = [" ".join(["F", str(kind), str(scalar), str(len(f))] + [_hex(v, scalar) for v in f.ravel()] + [_hex(v, scalar) for v in t.ravel()]) for _, f, t in cases]
    out = program(lines)
    assert len(out) == len(cases)
    statuses = set()
    for i, ((name, f, t), line, (status, want)) in enumerate(zip(cases, out, restated[kind, scalar])):
        p = line.split()
        assert p[0] == "R" and int(p[1]) == kind and int(p[3]) == len(f)
        assert int(p[2]) == status, (i, name)
        m64, m32 = p[5:14], p[14:23]
        assert (m32 if scalar == 0 else m64) == want, (i, name)
        if scalar == 0:  # an f32 fit: m64 holds the f32 values widened
            assert m64 == [_hex(struct.unpack("<f", struct.pack("<I", int(h, 16)))[0], 1) for h in m32], (i, name)
        else:            # an f64 fit: m32 is .as(f32)
            with np.errstate(all="ignore"):
                assert m32 == [_hex(np.float32(struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]), 0) for h in m64], (i, name)
        statuses.add(status)
    assert {R.OK, R.RANK_DEFICIENT} <= statuses


def test_bad_counts_project_and_invert(program):
    rng = np.random.default_rng(5)
    lines, wants = [], []
    for kind in KINDS:
        for scalar in SCALARS:
            T = R.F32 if scalar == 0 else R.F64
            n = R.MIN_POINTS[kind] - 1
            pts = rng.uniform(0, 9, size=(n, 2))
            lines.append(" ".join(["F", str(kind), str(scalar), str(n)] + [_hex(v, scalar) for v in pts.ravel()] * 2))
            wants.append(("R", R.BAD_COUNT, [_hex(v, scalar) for v in R.identity_flat(T, kind)]))
            m = [T(v) for v in (rng.uniform(-2, 2, size=9) + np.eye(3).ravel())]
            if kind != R.PROJECTIVE:
                m[6:] = [T(0)] * 3
            for _ in range(20):
                x, y = T(rng.uniform(-50, 700)), T(rng.uniform(-50, 700))
                lines.append(" ".join(["P", str(kind), str(scalar)] + [_hex(v, scalar) for v in m] + [_hex(x, scalar), _hex(y, scalar)]))
                with np.errstate(all="ignore"):
                    wants.append(("P", [_hex(v, scalar) for v in R.project(T, kind, m, (x, y))]))
            if kind == R.PROJECTIVE:
                for mat in (m, [T(v) for v in (1, 2, 3, 2, 4, 6, 0, 0, 1)]):
                    lines.append(" ".join(["I", str(scalar)] + [_hex(v, scalar) for v in mat]))
                    inv = R.inv3(T, [mat[0:3], mat[3:6], mat[6:9]])
                    wants.append(("R", R.RANK_DEFICIENT, [_hex(v, scalar) for v in R.identity_flat(T, kind)]) if inv is None else
                                 ("R", R.OK, [_hex(v, scalar) for row in inv for v in row]))
    out = program(lines)
    for line, want, src in zip(out, wants, lines):
        p = line.split()
        assert p[0] == want[0]
        if want[0] == "P":
            assert p[1:] == want[1], src
        else:
            scalar = int(src.split()[2] if src[0] == "F" else src.split()[1])
            assert int(p[2]) == want[1] and (p[14:23] if scalar == 0 else p[5:14]) == want[2], src


def test_the_librarys_host_forms_run_the_same_header(restated):
    """zg_transform_fit_points_host (the header compiled by hipcc's host pass, -ffp-contract=off) against the restatement, every third
    case; zg_transform_fit_matches_host against the points form; the Python mirror's find."""
    import zignal_amd as zg
    from zignal_amd import _lib as L
    from zignal_amd import transform as TF
    for kind in KINDS:
        for scalar in SCALARS:
            cases = K.fit_cases(kind, scalar)
            for i in range(0, len(cases), 3):
                name, f, t = cases[i]
                r = TF.fit_points_host(kind, f, t)
                status, want = restated[kind, scalar][i]
                got = r["m32"] if scalar == 0 else r["m64"]
                assert int(r["status"]) == status and [_hex(v, scalar) for v in got] == want, (kind, scalar, name)
                assert int(r["kind"]) == kind and int(r["n_points"]) == len(f)
    # a match list names the same points
    rng = np.random.default_rng(3)
    q, t = np.zeros(30, zg.KEYPOINT_DTYPE), np.zeros(40, zg.KEYPOINT_DTYPE)
    for k in (q, t):
        k["x"], k["y"] = rng.uniform(0, 300, len(k)).astype(np.float32), rng.uniform(0, 200, len(k)).astype(np.float32)
    m = np.zeros(20, zg.MATCH_DTYPE)
    m["query_idx"], m["train_idx"] = rng.permutation(30)[:20], rng.permutation(40)[:20]
    f = np.stack([q["x"][m["query_idx"]], q["y"][m["query_idx"]]], 1)
    o = np.stack([t["x"][m["train_idx"]], t["y"][m["train_idx"]]], 1)
    for kind in KINDS:
        for scalar, dt in ((L.SCALAR_F32, np.float32), (L.SCALAR_F64, np.float64)):
            assert TF.fit_matches_host(kind, scalar, q, t, m).tobytes() == TF.fit_points_host(kind, f.astype(dt), o.astype(dt)).tobytes()
            assert TF.fit_matches_host(kind, scalar, q, t, m, train_to_query=True).tobytes() == TF.fit_points_host(kind, o.astype(dt), f.astype(dt)).tobytes()
            assert TF.fit_matches_host(kind, scalar, q, t, m, count=7).tobytes() == TF.fit_points_host(kind, f[:7].astype(dt), o[:7].astype(dt)).tobytes()
    bad = m.copy()
    bad["train_idx"][5] = 40
    r = TF.fit_matches_host(TF.AFFINE, L.SCALAR_F64, q, t, bad)
    assert r["status"] == L.FIT_BAD_INPUT and r["m64"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0]
    with pytest.raises(TF.FitError, match="RankDeficient"):
        TF.find(TF.SIMILARITY, [(0, 0), (0, 0)], [(1, 1), (1, 1)])
    with pytest.raises(L.InvalidArgument):
        TF.fit_points_host(7, f, o)
    fitted = TF.find(TF.AFFINE, [(0, 0), (0, 1), (1, 1)], [(0, 1), (1, 1), (1, 0)])
    assert np.allclose(fitted.matrix, [[0, 1], [-1, 0]], atol=1e-9) and np.allclose(fitted.bias, [0, 1], atol=1e-9)
    assert len(fitted.coefficients()) == 6 and fitted.kind == TF.AFFINE

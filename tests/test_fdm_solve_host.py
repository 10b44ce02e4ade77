"""zignal_amd/csrc/zg_fdm_solve.h on the CPU: tests/c/fdm_solve.cpp includes only that header, is built with plain g++ under
-fsanitize=address,undefined with the two HIP qualifiers defined away and -ffp-contract=off, and prints the bits of U, s, W, bias, scale
and offset for a few hundred covariance pairs (random SPD, rank-deficient, zero, diagonal, nearly equal singular values), which must equal
tests/fdm_ref.py's bit for bit. The moments-to-statistics step is checked against fractions.Fraction within 2 ulp, n = 2^32 - 1 with
every sum at its largest and n = 0, 1, 2 included. Nothing is loaded into python under a sanitizer."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import fdm_cases as K
from tests import fdm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "fdm_solve.cpp")
BIN = os.path.join(ROOT, "tests", "c", "fdm_solve")


def _hex(v) -> str:
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _f64(h: str) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


@pytest.fixture(scope="module")
def program():
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__host__=", "-D__device__=", "-o", BIN, SRC], check=True)

    def run(lines):
        out = subprocess.run([BIN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and f"fdm solve ok {len(lines)}" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        return out.stdout.splitlines()[:-1]
    return run


def test_solve_bits_equal_the_restatement(program):
    cases = K.solve_cases()
    assert len(cases) >= 300
    lines = []
    for pixel, gray, tmean, tcov, smean, scov in cases:
        vals = list(tmean) + list(tcov.ravel()) + list(smean) + list(scov.ravel())
        lines.append(" ".join(["P", str(pixel), str(gray)] + [_hex(v) for v in vals]))
    out = program(lines)
    assert len(out) == 2 * len(cases)
    routes = set()
    for i, (pixel, gray, tmean, tcov, smean, scov) in enumerate(cases):
        t_line, x_line = out[2 * i].split(), out[2 * i + 1].split()
        target = R.make_target(list(tmean), tcov.tolist(), bool(gray))  # every family converges (tests/test_fdm_oracle.py)
        assert t_line[0] == "T" and int(t_line[1]) == 0
        assert t_line[2:] == [_hex(v) for row in target["u"] for v in row] + [_hex(v) for v in target["s"]], i
        x = R.make_transform(pixel == 0, target, list(smean), scov.tolist())
        assert x_line[0] == "X" and int(x_line[1]) == x["route"] and int(x_line[2]) == 0
        want = [_hex(v) for row in x["w"] for v in row] + [_hex(v) for v in x["bias"]] + [_hex(x["scale"]), _hex(x["offset"])]
        assert x_line[3:] == want, i
        routes.add(x["route"])
    assert routes == {R.ROUTE_COLOR, R.ROUTE_SCALAR, R.ROUTE_GRAY_TARGET}


def _within_2_ulp(got: float, exact: Fraction) -> bool:
    if exact == 0:
        return got == 0.0
    return abs(Fraction(got) - exact) <= 2 * Fraction(math.ulp(got))


def test_moments_to_statistics_within_2_ulp_of_the_exact_rational(program):
    rng = np.random.default_rng(22)
    big = 2 ** 32 - 1
    cov_cases = [(0, 0, 0, 0), (1, 200, 100, 20000), (2, 255, 0, 0), (2, 300, 300, 2 * 150 * 150), (2, 255, 255, 65025), (2, 10, 500, 255 * 10),
                 (big, 255 * big, 255 * big, 65025 * big),  # every sum at its largest: the covariance of a constant frame, exactly 0
                 (big, 255 * big, 0, 0), (big, 128 * big, 127 * big, 65025 * big), (big, 1, 1, 65025 * big), (big, 255 * big, 255 * big, 0),
                 (big, 3, 5, 0), (big, 0, 0, 1), (big, 255 * big - 1, 255 * big, 65025 * big)]
    for _ in range(150):  # frames that exist
        n = int(rng.integers(2, 5000))
        a, b = rng.integers(0, 256, size=n).astype(object), rng.integers(0, 256, size=n).astype(object)
        cov_cases.append((n, int(a.sum()), int(b.sum()), int((a * b).sum())))
        cov_cases.append((n, int(a.sum()), int(a.sum()), int((a * a).sum())))
    for _ in range(150):  # and any words at all inside the bounds: the arithmetic does not care whether a frame has them
        n = int(rng.integers(2, 2 ** 32))
        cov_cases.append((n, int(rng.integers(0, 255 * n + 1)), int(rng.integers(0, 255 * n + 1)), int(rng.integers(0, 65025 * n + 1))))
    mean_cases = [(0, 0), (1, 0), (1, 255), (2, 255), (big, 255 * big), (big, 1), (big, 255 * big - 1)]
    for _ in range(100):
        n = int(rng.integers(1, 2 ** 32))
        mean_cases.append((n, int(rng.integers(0, 255 * n + 1))))
    lines = ["C %d %d %d %d" % c for c in cov_cases] + ["A %d %d" % m for m in mean_cases]
    out = program(lines)
    for c, line in zip(cov_cases, out[:len(cov_cases)]):
        kind, h = line.split()
        assert kind == "C" and _within_2_ulp(_f64(h), R.exact_cov(*c)), (c, _f64(h), float(R.exact_cov(*c)))
    for m, line in zip(mean_cases, out[len(cov_cases):]):
        kind, h = line.split()
        assert kind == "A" and _within_2_ulp(_f64(h), R.exact_mean(*m)), (m, _f64(h))
    # n <= 1 is the reference's early return (stats.zig:290, :303), whatever the sums
    assert _f64(out[0].split()[1]) == 0.0 and _f64(out[1].split()[1]) == 0.0


def test_the_librarys_host_forms_run_the_same_header():
    """zg_fdm_target_host / zg_fdm_transform_host (the header compiled by hipcc's host pass, -ffp-contract=off) against the restatement."""
    from zignal_amd import _lib as L
    from zignal_amd import fdm
    for pixel, gray, tmean, tcov, smean, scov in K.solve_cases()[::3]:
        target = R.make_target(list(tmean), tcov.tolist(), bool(gray))
        t = fdm.target_host(pixel, tmean, tcov, bool(gray))
        assert t.status == 0 and t.pixel == pixel and bool(t.is_gray) == bool(gray)
        assert [_hex(v) for v in t.u] + [_hex(v) for v in t.s] == [_hex(v) for row in target["u"] for v in row] + [_hex(v) for v in target["s"]]
        want = R.make_transform(pixel == 0, target, list(smean), scov.tolist())
        x = fdm.transform_host(pixel, t, smean, scov)
        assert (x.route, x.status) == (want["route"], 0)
        assert [_hex(v) for v in x.w] + [_hex(v) for v in x.bias] + [_hex(x.scale), _hex(x.offset)] == \
            [_hex(v) for row in want["w"] for v in row] + [_hex(v) for v in want["bias"]] + [_hex(want["scale"]), _hex(want["offset"])]
    with pytest.raises(L.ZignalError):
        fdm.target_host(L.PIXEL_RGB_F32, [0, 0, 0], np.zeros((3, 3)), False)
    t = fdm.target_host(L.PIXEL_RGB_U8, [0, 0, 0], np.zeros((3, 3)), False)
    with pytest.raises(L.InvalidArgument):
        fdm.transform_host(L.PIXEL_RGBA_U8, t, [0, 0, 0], np.zeros((3, 3)))  # not the target's type

"""tests/transform_ref.py, the restatement of the reference's three find functions that the host program, the library's host forms and
through them the device kernels are held to, pinned to the reference's own tests (src/geometry/transforms.zig:294-520) at the reference's
tolerances, and its generic SVD pinned to the 3 x 3 restatement tests/fdm_ref.py already holds. The same file checks that the header, the
Python binding and the Zig shim declare the same symbols."""
import math
import os
import re

import numpy as np
import pytest

from tests import fdm_cases
from tests import fdm_ref
from tests import transform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = R.F64


def test_the_three_rank_deficient_errors_and_the_collinear_error():
    with pytest.raises(R.RankDeficient):
        R.find_similarity(T, [(0, 0), (0, 0)], [(1, 1), (1, 1)])
    line3 = [(0, 0), (1, 0), (2, 0)]
    with pytest.raises(R.RankDeficient):
        R.find_affine(T, line3, line3)
    line4 = [(0, 0), (1, 0), (2, 0), (3, 0)]
    with pytest.raises(R.RankDeficient):
        R.find_projective(T, line4, line4)
    destination = [(50, 20), (150, 40), (30, 120), (130, 140)]
    with pytest.raises(R.RankDeficient):
        R.find_projective(T, [(0, 0), (1, 1), (2, 2), (3, 3)], destination)


def _project_affine(matrix, bias, p):
    m = [matrix[0][0], matrix[0][1], matrix[1][0], matrix[1][1], bias[0], bias[1], 0.0, 0.0, 0.0]
    return R.project(T, R.AFFINE, m, p)


def test_affine3_and_additional_correspondences():
    for from_points, to_points in (([(0, 0), (0, 1), (1, 1)], [(0, 1), (1, 1), (1, 0)]),
                                   ([(0, 0), (0, 1), (1, 1), (1, 0)], [(0, 1), (1, 1), (1, 0), (0, 0)])):
        matrix, bias = R.find_affine(T, from_points, to_points)
        want_m, want_b = [[0, 1], [-1, 0]], [0, 1]
        for r in range(2):
            for c in range(2):
                assert abs(matrix[r][c] - want_m[r][c]) <= 1e-9
            assert abs(bias[r] - want_b[r]) <= 1e-9
        inv_m, inv_b = R.find_affine(T, to_points, from_points)
        for f, t in zip(from_points, to_points):
            fx, fy = _project_affine(matrix, bias, f)
            assert abs(fx - t[0]) <= 1e-9 and abs(fy - t[1]) <= 1e-9
            bx, by = _project_affine(inv_m, inv_b, t)
            assert abs(bx - f[0]) <= 1e-9 and abs(by - f[1]) <= 1e-9


def _rel(a, b, tol):
    return abs(a - b) <= tol * max(abs(a), abs(b))


def _flat(rows):
    return [v for row in rows for v in row]


def test_projection4_against_the_dlib_matrix():
    tol = 1e-5
    from_points = [(199.67754364, 200.17905235), (167.90229797, 175.55920601), (270.33649445, 207.96521187), (267.53637314, 188.24442387)]
    to_points = [(440.68012238, 275.45248032), (429.62512970, 262.64307976), (484.23328400, 279.44332123), (488.08315277, 272.79547691)]
    m = R.find_projective(T, from_points, to_points)
    dlib = [[-5.9291612941280800e-03, 7.0341614664190845e-03, -8.9922894648198459e-01],
            [-2.8361695646354147e-03, 2.9060176209597761e-03, -4.3735741833190661e-01],
            [-1.0156215756801098e-05, 1.3270311721030187e-05, -2.1603199531972065e-03]]
    scale = dlib[2][2] / m[2][2]
    for r in range(3):
        for c in range(3):
            assert abs(scale * m[r][c] - dlib[r][c]) <= 1e-3
    for f, t in zip(from_points, to_points):
        px, py = R.project(T, R.PROJECTIVE, _flat(m), f)
        assert _rel(px, t[0], tol) and _rel(py, t[1], tol)
    m_inv = R.inv3(T, m)
    assert m_inv is not None
    t_inv = R.find_projective(T, to_points, from_points)
    for f in from_points:
        p = R.project(T, R.PROJECTIVE, _flat(m), f)
        for back in (t_inv, m_inv):
            bx, by = R.project(T, R.PROJECTIVE, _flat(back), p)
            assert _rel(f[0], bx, tol) and _rel(f[1], by, tol)


def test_projection8_against_the_dlib_matrix():
    from_points = [(319.48406982, 240.21486282), (268.64367676, 210.67104721), (432.53839111, 249.55825424), (428.05819702, 225.89330864),
                   (687.00787354, 240.97020721), (738.32287598, 208.32876205), (574.62890625, 250.60971451), (579.63378906, 225.37580109)]
    to_points = [(330.48120117, 408.22596359), (317.55538940, 393.26282501), (356.74267578, 411.06428146), (349.94784546, 400.26379395),
                 (438.15582275, 411.75442886), (452.01367188, 398.08815765), (398.66107178, 413.83139420), (395.29974365, 401.73685455)]
    m = R.find_projective(T, from_points, to_points)
    dlib = [[7.9497770144471079e-05, 8.6315632819330035e-04, -6.3240797603906806e-01],
            [3.9739851020393160e-04, 6.4356336568222570e-04, -7.7463154396817901e-01],
            [1.0207719920241196e-06, 2.6961794891002063e-06, -2.1907681782918601e-03]]
    tol = math.sqrt(R.eps_of(T))
    for r in range(3):
        for c in range(3):
            assert abs(m[r][c] - dlib[r][c]) <= tol
    for f, t in zip(from_points, to_points):
        px, py = R.project(T, R.PROJECTIVE, _flat(m), f)
        assert _rel(px, t[0], 1e-2) and _rel(py, t[1], 1e-2)


def test_the_exact_four_point_round_trip():
    source = [(0, 0), (100, 0), (0, 100), (100, 100)]
    destination = [(50, 20), (150, 40), (30, 120), (130, 140)]
    forward = R.find_projective(T, source, destination)
    for s, d in zip(source, destination):
        px, py = R.project(T, R.PROJECTIVE, _flat(forward), s)
        assert abs(d[0] - px) <= 1e-9 and abs(d[1] - py) <= 1e-9
    backward = R.find_projective(T, destination, source)
    rx, ry = R.project(T, R.PROJECTIVE, _flat(backward), R.project(T, R.PROJECTIVE, _flat(forward), (33, 71)))
    assert abs(33 - rx) <= 1e-9 and abs(71 - ry) <= 1e-9


def test_generic_svd_at_3x3_equals_the_fdm_restatement_bit_for_bit():
    cases = fdm_cases.solve_cases()
    assert len(cases) >= 300
    for _, _, _, tcov, _, scov in cases:
        for cov in (tcov, scov):
            a = cov.tolist()
            u, q, _, converged = R.svd(T, a, False, R.SKINNY_U)
            fu, fq, fconv = fdm_ref.svd3(a)
            assert converged == fconv
            assert np.array(u, np.float64).tobytes() == np.array(fu, np.float64).tobytes()
            assert np.array(q, np.float64).tobytes() == np.array(fq, np.float64).tobytes()


def test_f32_restatement_rounds_every_operation_in_f32():
    """The f32 path never leaves numpy.float32: a fit's values are float32 scalars, and differ from the f64 fit rounded afterwards."""
    rng = np.random.default_rng(2)
    f = rng.uniform(0, 640, size=(9, 2)).astype(np.float32)
    t = rng.uniform(0, 480, size=(9, 2)).astype(np.float32)
    pts = lambda a, S: [(S(p[0]), S(p[1])) for p in a.tolist()]  # noqa: E731
    differs = 0
    for kind in (R.SIMILARITY, R.AFFINE, R.PROJECTIVE):
        status, m32 = R.fit(R.F32, kind, pts(f, R.F32), pts(t, R.F32))
        assert status == R.OK and all(type(v) is np.float32 for v in m32[:6])
        _, m64 = R.fit(R.F64, kind, pts(f, R.F64), pts(t, R.F64))
        differs += sum(1 for a, b in zip(m32, m64) if np.float32(b) != a)
    assert differs > 0


def test_header_python_binding_and_zig_shim_declare_the_same_symbols():
    from zignal_amd import _lib as L
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert main.count('#include "zignal_hip_transform.h"') == 1
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_transform.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert sorted(name for name, _ in protos) == sorted(L.TRANSFORM_EXPORTED_SYMBOLS) and len(protos) == 11
    for name, args in protos:
        args = args.strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert len(L._TRANSFORM_SIGNATURES[name]) == n, name
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_transform.zig")).read()
    assert set(re.findall(r"pub extern fn (zg_\w+)\(", shim)) == set(L.TRANSFORM_EXPORTED_SYMBOLS)
    others = (set(L.EXPORTED_SYMBOLS) | set(L.ORB_EXPORTED_SYMBOLS) | set(L.MATCH_EXPORTED_SYMBOLS) | set(L.HOUGH_EXPORTED_SYMBOLS) | set(L.FLOOD_EXPORTED_SYMBOLS)
              | set(L.METRICS_EXPORTED_SYMBOLS) | set(L.QUANTIZE_EXPORTED_SYMBOLS) | set(L.CANVAS_EXPORTED_SYMBOLS) | set(L.TEXT_EXPORTED_SYMBOLS)
              | set(L.FDM_EXPORTED_SYMBOLS) | set(L.TRACER_EXPORTED_SYMBOLS) | set(L.QR_EXPORTED_SYMBOLS))
    assert not set(L.TRANSFORM_EXPORTED_SYMBOLS) & others
    import ctypes
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in L.TRANSFORM_EXPORTED_SYMBOLS:
        assert hasattr(raw, name), name
    assert raw.zg_transform_sizeof_fit() == ctypes.sizeof(L.ZgTransformFit) == 128

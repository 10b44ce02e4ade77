"""tests/fdm_ref.py, the restatement of FeatureDistributionMatching the device tests compare with, against properties the reference's code
implies. No GPU and no library call apart from the binding tables.

The restated Golub-Reinsch SVD against numpy.linalg.svd: over tests/fdm_cases.py's covariance_matrices() (random SPD, rank 2, rank 1,
zero, diagonal, nearly equal singular values) the largest |s - s_numpy| measured was 44.8 * eps * s_max; the bound below is 4 times that,
180 * eps * s_max."""
import os
import re

import numpy as np

from tests import fdm_cases as K
from tests import fdm_ref as R
from zignal_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SVD_BOUND = 180.0


def test_svd_is_orthonormal_reconstructs_and_is_sorted():
    worst = 0.0
    for family, c in K.covariance_matrices():
        u, s, converged = R.svd3(c.tolist())
        assert converged == 0, family
        u, s = np.array(u), np.array(s)
        assert s[0] >= s[1] >= s[2] >= 0.0, (family, s)
        ref = np.linalg.svd(c, compute_uv=False)
        s_max = max(float(ref[0]), 1e-300)
        err = float(np.max(np.abs(s - ref))) / (EPS * s_max)
        worst = max(worst, err)
        assert err <= SVD_BOUND, (family, err)
        # U diag(s) U^T is the covariance again: for a symmetric positive semi-definite matrix V = U on every non-zero singular value
        assert np.max(np.abs(u @ np.diag(s) @ u.T - c)) <= 64 * EPS * s_max, family
        if family in ("spd", "near_equal") or (family == "diagonal" and np.all(np.diag(c) > 0)):
            assert np.max(np.abs(u.T @ u - np.eye(3))) <= 64 * EPS, family
    print("largest |s - numpy| / (eps * s_max):", worst)


def test_zero_matrix_gives_identity_and_zero_values():
    u, s, converged = R.svd3([[0.0] * 3] * 3)
    assert converged == 0 and s == [0.0, 0.0, 0.0] and u == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def test_constant_frame_has_exactly_zero_m2():
    for value in (0, 1, 77, 255):
        v = value / 255.0
        count, mean, m2 = R.welford([(v, v, v)] * 500)
        assert count == 500 and mean == [v, v, v] and m2 == [[0.0] * 3] * 3
    frame = np.empty((9, 11, 3), np.uint8)
    frame[...] = (3, 200, 41)
    mean, cov = R.image_stats(frame)
    assert cov == [[0.0] * 3] * 3 and mean == [3 / 255.0, 200 / 255.0, 41 / 255.0]


def test_the_references_own_test_passes_on_the_restatement():
    """fdm.zig:325-420 on its 50 x 50 pattern: every channel mean within 2.0 of the target's, every variance within 1."""
    i = np.arange(2500)
    x, y = i % 50, i // 50
    src = np.stack([100 + x % 20, 150 + y % 15, 80 + (x + y) % 25], -1).astype(np.uint8).reshape(50, 50, 3)
    tgt = np.stack([50 + x % 30, 70 + y % 20, 90 + (x + y) % 35], -1).astype(np.uint8).reshape(50, 50, 3)
    out = R.match(src, tgt).astype(np.float64)
    t = tgt.astype(np.float64)
    for c in range(3):
        assert abs(out[..., c].mean() - t[..., c].mean()) <= 2.0
        assert abs(out[..., c].var() - t[..., c].var()) <= 1.0


def test_the_references_scalar_and_gray_target_tests_pass():
    src = np.arange(100, dtype=np.uint8).reshape(1, 100)
    tgt = (100 + np.arange(100)).astype(np.uint8).reshape(1, 100)
    assert R.match(src, tgt).astype(np.float64).mean() == 149.5  # fdm.zig:429-464
    idx = np.arange(144)
    x, y = idx % 12, idx // 12
    csrc = np.stack([(x * 30 + y * 5) % 255, (x * 15 + y * 40) % 255, (x * 50 + y * 25) % 255], -1).astype(np.uint8).reshape(12, 12, 3)
    gray = (40 + idx % 160).astype(np.uint8).reshape(12, 12)
    out = R.match(csrc, np.repeat(gray[..., None], 3, 2))  # fdm.zig:531-581
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 1], out[..., 2])
    assert abs(out[..., 0].astype(np.float64).mean() - gray.astype(np.float64).mean()) <= 2.0
    assert abs(out[..., 0].astype(np.float64).var() - gray.astype(np.float64).var()) <= 2.0


def test_matching_a_frame_to_itself_returns_it_unchanged():
    for name, src, tgt in K.end_to_end_cases():
        if name.endswith("source_is_target"):
            assert np.array_equal(R.match(src, tgt), src), name
    rng = np.random.default_rng(5)
    rgba = np.dstack([K.correlated_rgb(rng, 20, 24), rng.integers(0, 256, size=(20, 24, 1), dtype=np.uint8)])
    assert np.array_equal(R.match(rgba, rgba), rgba)  # alpha kept on the colour route


def test_gray_target_route_zeroes_alpha_and_round_is_half_away():
    rng = np.random.default_rng(6)
    rgba = np.dstack([K.correlated_rgb(rng, 8, 9), np.full((8, 9, 1), 200, np.uint8)])
    gray = np.repeat(rng.integers(30, 220, size=(8, 9, 1), dtype=np.uint8), 3, 2)
    out = R.match(rgba, np.dstack([gray, np.full((8, 9, 1), 9, np.uint8)]))
    assert np.all(out[..., 3] == 0) and np.array_equal(out[..., 0], out[..., 2])
    # @round: 0.5 -> 1, 254.5 -> 255, and the f64 just under 0.5 stays 0 (floor(x + 0.5) would say 1)
    res = np.array([0.5 / 255.0, 254.5 / 255.0, 0.49999999999999994 / 255.0, -3.0, 7.0, float("nan")])
    got, pre = R._round_unit(res)
    want = [int(p) + (1 if p - int(p) >= 0.5 else 0) for p in pre.tolist()]
    assert got.tolist() == want and got[3] == 0 and got[4] == 255 and got[5] == 255


def test_header_python_binding_and_zig_shim_declare_the_same_symbols():
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert '#include "zignal_hip_fdm.h"' in main
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_fdm.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert sorted(name for name, _ in protos) == sorted(L.FDM_EXPORTED_SYMBOLS) and len(protos) == 19
    for name, args in protos:
        args = args.strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert len(L._FDM_SIGNATURES[name]) == n, name
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_fdm.zig")).read()
    assert set(re.findall(r"pub extern fn (zg_\w+)\(", shim)) == set(L.FDM_EXPORTED_SYMBOLS)
    others = (set(L.EXPORTED_SYMBOLS) | set(L.ORB_EXPORTED_SYMBOLS) | set(L.MATCH_EXPORTED_SYMBOLS) | set(L.HOUGH_EXPORTED_SYMBOLS) | set(L.FLOOD_EXPORTED_SYMBOLS)
              | set(L.METRICS_EXPORTED_SYMBOLS) | set(L.QUANTIZE_EXPORTED_SYMBOLS) | set(L.CANVAS_EXPORTED_SYMBOLS) | set(L.TEXT_EXPORTED_SYMBOLS))
    assert not set(L.FDM_EXPORTED_SYMBOLS) & others
    import ctypes
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in L.FDM_EXPORTED_SYMBOLS:
        assert hasattr(raw, name), name

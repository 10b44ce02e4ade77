"""CPU checks of ORB (reference src/features/orb.zig): the two CPU restatements of tests/orb_ref.py agree byte for byte, the
reference's own unit tests hold for them, the host arithmetic of the C ABI equals them, the C ABI rejects bad arguments before
touching a device, and the inputs of the GPU suite reach every branch the restatements count. No GPU needed."""
import ctypes

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import fast_ref as F
from tests import orb_ref as R
from tests.test_fast_oracle import KINDS, small_image

SHAPES = ((64, 80), (48, 97), (120, 90), (75, 75))
# n_features, n_levels, scale_factor, first_level, edge_threshold
CONFIGS = ((60, 4, 1.2, 0, 15), (500, 3, 1.5, 0, 15), (20, 8, 1.2, 2, 31), (1, 2, 2.0, 0, 0), (5, 4, 1.2, 1, 7),
           (100000, 5, 1.3, 0, 15), (37, 1, 1.2, 0, 3))


def sweep_cases(seed=0):
    """(image, Params, name): every kind of small image x both score types x every configuration, 56 cases."""
    rng = np.random.default_rng(seed)
    cases, i = [], 0
    for kind in KINDS:
        for harris in (False, True):
            for nf, nl, sf, fl, et in CONFIGS:
                shape = SHAPES[i % len(SHAPES)]
                i += 1
                p = R.Params(n_features=nf, n_levels=nl, scale_factor=sf, first_level=fl, edge_threshold=et, harris=harris)
                cases.append((small_image(rng, shape, kind), p, f"{kind}{shape} harris={harris} nf={nf} nl={nl} sf={sf} first={fl} edge={et}"))
    return cases


def tiny_weights() -> np.ndarray:
    """The library's orientation table scaled so that a full patch of mid-grey (127.5) sums to exactly the m00 < 0.001 guard
    (orb.zig:422): patches of noise then fall on both sides of it. A caller's table is the one way to that branch, since a FAST
    corner always has a bright pixel under a weight of at least exp(-2)."""
    w = R.orientation_weights()
    return (w * np.float32(0.001 / (127.5 * float(w.sum())))).astype(np.float32)


def plateau_image(seed, shape):
    return small_image(np.random.default_rng(seed), shape, "plateau")


def named_cases(oracle):
    """The larger inputs of the GPU suite that the coverage counters lean on."""
    noise = oracle.synth_u8(7, (240, 320))
    return [(noise, R.Params(), "noise 240x320 defaults"),
            (noise, R.Params(harris=True), "noise 240x320 harris"),
            (plateau_image(3, (200, 300)), R.Params(), "plateau 200x300 defaults"),
            (F.photo_like(oracle.synth_u8(5, (480, 640))), R.Params(), "photo-like 480x640 defaults"),
            (noise, R.Params(weights=tiny_weights(), n_features=200), "noise 240x320 tiny weights")]


def test_dtypes_and_defaults_follow_the_reference():
    assert zg.BINARY_DESCRIPTOR_DTYPE.itemsize == ctypes.sizeof(L.ZgBinaryDescriptor) == 32  # BinaryDescriptor.zig:10
    assert zg.BinaryDescriptor is zg.BINARY_DESCRIPTOR_DTYPE
    o = zg.Orb()  # orb.zig:87-109
    assert (o.n_features, o.n_levels, o.edge_threshold, o.first_level, o.wta_k, o.fast_threshold, o.score_type) == (500, 8, 15, 0, 2, 20, "fast_score")
    assert np.float32(o.scale_factor) == np.float32(1.2)
    o = zg.Orb(n_features=1000, scale_factor=1.5, n_levels=6)  # "ORB initialization" (:520-530)
    assert (o.n_features, o.scale_factor, o.n_levels) == (1000, 1.5, 6)
    d = L.ZgOrbParams()
    zg.lib().zg_orb_default_params(ctypes.byref(d))
    assert (d.n_features, d.n_levels, d.edge_threshold, d.first_level, d.wta_k, d.fast_threshold, d.score_type, d.orientation_weights) == (
        500, 8, 15, 0, 2, 20, L.ORB_FAST_SCORE, None)
    assert np.float32(d.scale_factor) == np.float32(1.2)


def test_pair_table_is_the_published_one():
    assert R.PAIRS.shape == (256, 4) and R.PAIRS.dtype == np.int8
    assert R.pairs_sha256() == "2164181aea6ff9ac426ca512d5130d15e1f6e3cd47b1cbdd568bbe1e55d49023"
    assert (int(R.PAIRS.min()), int(R.PAIRS.max()), int(R.PAIRS.astype(np.int64).sum())) == (-13, 12, -406)


def test_weight_table_shape():
    w = R.orientation_weights().reshape(31, 31)
    assert int((w != 0).sum()) == 709 and w[15, 15] == 1.0 and w[0, 0] == 0.0
    assert w[15, 0] == w[0, 15] == w[30, 15] == w[15, 30] == R.expf(np.float32(-2.0))
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1])


def test_literal_and_vectorised_restatements_agree():
    cases = sweep_cases()
    assert len(cases) >= 50
    nonempty = 0
    for img, p, what in cases:
        ka, da, ca = R.detect_and_compute_literal(img, p)
        kb, db, cb = R.detect_and_compute_fast(img, p)
        assert ka.dtype == kb.dtype == zg.KEYPOINT_DTYPE and da.dtype == db.dtype == zg.BINARY_DESCRIPTOR_DTYPE, what
        assert ka.tobytes() == kb.tobytes(), f"{what}: literal {len(ka)} keypoints, vectorised {len(kb)}"
        assert da.tobytes() == db.tobytes(), f"{what}: descriptors differ"
        assert ca == cb, f"{what}: {ca} vs {cb}"
        assert len(ka) == len(da) <= p.n_features
        nonempty += len(ka) > 0
    assert nonempty > len(cases) // 3


def test_compute_restatements_agree_on_hand_made_keypoints():
    img = small_image(np.random.default_rng(9), (90, 110), "noise")
    p = R.Params(n_levels=4)
    kps = hand_made_keypoints(img.shape)
    a, b = R.compute_literal(img, kps, p), R.compute_fast(img, kps, p)
    assert a.tobytes() == b.tobytes()
    assert not a["bits"][-1].any()  # far outside the image: every bit stays 0


def hand_made_keypoints(shape) -> np.ndarray:
    """Keypoints no detector returns: octaves below 0 and past the pyramid, fractional positions, positions at and outside the
    borders, angles all round the circle."""
    rows, cols = shape
    rows_ = [(10.5, 12.25, 0.0, 0), (cols - 1.0, rows - 1.0, 45.0, 0), (0.0, 0.0, -135.0, 0), (cols / 2, rows / 2, 179.5, -3), (cols / 2, rows / 2, -179.5, 1),
             (cols / 3, rows / 3, 90.0, 99), (cols + 5.0, rows / 2, 10.0, 2), (-7.5, -2.5, 300.0, 0), (cols * 0.7, rows * 0.2, 360.0, 3),
             (cols * 50.0, rows * 50.0, 33.0, 1)]
    kps = np.zeros(len(rows_), zg.KEYPOINT_DTYPE)
    for k, (x, y, angle, octave) in zip(kps, rows_):
        k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = x, y, 7.0, angle, 1.0, octave, -1
    return kps


# ---- the reference's own unit tests (orb.zig:520-663) ------------------------------------------------------------------
def test_reference_feature_distribution():
    per = R.features_per_level(R.Params(n_features=500, n_levels=4, scale_factor=1.2))
    assert len(per) == 4 and 490 <= sum(per) <= 510 and per[0] > per[1]
    per = R.features_per_level(R.Params(n_features=5, n_levels=4, scale_factor=1.2))
    assert all(n <= 5 for n in per) and sum(per) == 5
    assert R.features_per_level(R.Params(n_features=10, n_levels=1)) == [10]  # the even split (:287-300)


def test_reference_adaptive_threshold():
    p = R.Params(fast_threshold=20, scale_factor=1.2, n_levels=12)
    assert R.adaptive_threshold(p, 0) == 20
    assert R.adaptive_threshold(p, 10) >= 5 and R.adaptive_threshold(p, 11) >= 5


def reference_synthetic_image() -> np.ndarray:
    """orb.zig:561-595: grey 100, a white square, a black square and a checkered patch."""
    img = np.full((100, 100), 100, np.uint8)
    img[15:35, 15:35] = 250
    img[55:75, 55:75] = 10
    r, c = np.mgrid[40:50, 20:30]
    img[40:50, 20:30] = np.where((r + c) % 2 == 0, 200, 50)
    return img


def test_reference_detect_and_compute_on_synthetic_image():
    img = reference_synthetic_image()
    p = R.Params(n_features=50, n_levels=3, fast_threshold=10)
    for run in (R.detect_and_compute_literal, R.detect_and_compute_fast):
        kps, des, _ = run(img, p)
        assert len(kps) > 0 and len(kps) == len(des)
        assert ((kps["x"] >= 0) & (kps["x"] < 100) & (kps["y"] >= 0) & (kps["y"] < 100)).all()
        assert ((kps["angle"] >= -180) & (kps["angle"] <= 180)).all()
        assert ((kps["octave"] >= 0) & (kps["octave"] < 3)).all()
        assert des["bits"].any()


# ---- the host arithmetic of the C ABI ----------------------------------------------------------------------------------
def test_features_per_level_and_adaptive_threshold_equal_the_restatement():
    for nf in (0, 1, 5, 37, 500, 1000, 100000):
        for nl in (1, 2, 3, 4, 8, 12, 32):
            for sf in (1.05, 1.2, 1.3, 1.5, 2.0, 3.7):
                orb = zg.Orb(n_features=nf, n_levels=nl, scale_factor=sf)
                assert orb.features_per_level() == R.features_per_level(R.Params(n_features=nf, n_levels=nl, scale_factor=sf)), (nf, nl, sf)
    for ft in (0, 1, 5, 10, 20, 100, 255):
        for sf in (1.05, 1.2, 1.5, 2.0):
            orb = zg.Orb(fast_threshold=ft, scale_factor=sf, n_levels=12)
            p = R.Params(fast_threshold=ft, scale_factor=sf, n_levels=12)
            assert [orb.adaptive_threshold(l) for l in range(12)] == [R.adaptive_threshold(p, l) for l in range(12)], (ft, sf)


def _img(rows, cols, pixel=L.PIXEL_U8, data=0x1000):
    return L.ZgImage(data, cols, rows, cols, pixel)


def _params(**kw):
    p = L.ZgOrbParams()
    zg.lib().zg_orb_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_orb_arguments_without_a_gpu():
    lib = zg.lib()
    n = ctypes.c_uint32(7)
    img = _img(480, 640)
    kp, cnt = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)

    def dev(image, params, keypoints=kp, cap=4):
        return lib.zg_orb_detect_and_compute(ctypes.byref(image), ctypes.byref(params), keypoints, None, cap, cnt, None)

    def host(image, params):
        return lib.zg_orb_detect_and_compute_host(ctypes.byref(image), ctypes.byref(params), None, None, 0, ctypes.byref(n))

    bad = [_params(n_levels=0), _params(n_levels=256), _params(scale_factor=1.0), _params(scale_factor=0.5), _params(edge_threshold=256),
           _params(first_level=256), _params(fast_threshold=256), _params(wta_k=3), _params(wta_k=300), _params(score_type=2)]
    for p in bad:
        assert dev(img, p) == L.ERR_INVALID_ARGUMENT
        assert host(img, p) == L.ERR_INVALID_ARGUMENT
        assert lib.zg_orb_compute(ctypes.byref(img), ctypes.byref(p), kp, 1, cnt, None) == L.ERR_INVALID_ARGUMENT
        assert lib.zg_orb_compute_host(ctypes.byref(img), ctypes.byref(p), kp, 1, cnt) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_orb_features_per_level(ctypes.byref(_params(n_levels=0)), (ctypes.c_uint32 * 4)()) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_orb_adaptive_threshold(ctypes.byref(_params(scale_factor=1.0)), 0) < 0
    # the pyramid stops before n_levels: 30 / 1.2^7 = 8.4 rows is fine, 28 / 1.2^7 = 7.8 is not
    assert dev(_img(28, 640), _params()) == L.ERR_INVALID_ARGUMENT
    assert b"pyramid" in lib.zg_last_error()
    assert host(_img(640, 28), _params()) == L.ERR_INVALID_ARGUMENT
    assert dev(_img(7, 640), _params(n_levels=1)) == L.ERR_INVALID_ARGUMENT  # Fast.detect's assert
    for pixel in (L.PIXEL_F32, L.PIXEL_RGB_U8, L.PIXEL_RGBA_U8):
        assert dev(_img(480, 640, pixel), _params()) == L.ERR_UNSUPPORTED
    assert dev(img, _params(n_levels=33, scale_factor=1.01)) == L.ERR_UNSUPPORTED  # more levels than one launch carries
    assert dev(img, _params(), keypoints=None) == L.ERR_INVALID_ARGUMENT  # no buffer for 4 keypoints
    assert lib.zg_orb_detect_and_compute(ctypes.byref(img), ctypes.byref(_params()), kp, None, 4, None, None) == L.ERR_INVALID_ARGUMENT  # no count
    assert lib.zg_orb_detect_and_compute(ctypes.byref(img), None, kp, None, 4, cnt, None) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_orb_compute(ctypes.byref(img), ctypes.byref(_params()), None, 3, cnt, None) == L.ERR_INVALID_ARGUMENT
    assert n.value == 7  # nothing written


def test_python_binding_raises_before_device_work():
    with pytest.raises(zg.InvalidArgument):
        zg.Orb(wta_k=3).detect(np.zeros((100, 100), np.uint8))
    with pytest.raises(zg.InvalidArgument):
        zg.Orb().detect(np.zeros((20, 100), np.uint8))  # level 7 would be 5 rows
    with pytest.raises(zg.InvalidArgument):
        zg.Orb(n_levels=0).features_per_level()
    with pytest.raises(ValueError):
        zg.Orb(score_type="best")
    with pytest.raises(ValueError):
        zg.Orb(orientation_weights=np.zeros(10, np.float32))


# ---- the ORB module's boundary: include/zignal_hip_orb.h, _lib._ORB_SIGNATURES and zig/zignal_hip_orb.zig in step ----------------
def _orb_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "zignal_hip_orb.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return root, dict(protos)


def test_orb_header_bindings_and_zig_file_declare_the_same_symbols():
    """What tests/test_abi.py holds include/zignal_hip.h to, for the ORB module's header: exported, bound with the same arity,
    declared by the Zig file; and the main header pulls the module in."""
    import os
    import re
    root, protos = _orb_header()
    assert sorted(protos) == sorted(L.ORB_EXPORTED_SYMBOLS) and len(protos) == 7
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in protos.items():
        assert hasattr(raw, name), f"{name} declared in include/zignal_hip_orb.h but not exported"
        assert len(L._ORB_SIGNATURES[name]) == len(args.split(",")), name
    assert not set(L.ORB_EXPORTED_SYMBOLS) & set(L.EXPORTED_SYMBOLS)
    shim = open(os.path.join(root, "zig", "zignal_hip_orb.zig")).read()
    assert set(re.findall(r"pub extern fn (zg_\w+)\(", shim)) == set(protos)
    assert '#include "zignal_hip_orb.h"' in open(os.path.join(root, "include", "zignal_hip.h")).read()
    assert ctypes.sizeof(L.ZgOrbParams) == 40 and L.ZgOrbParams.orientation_weights.offset == 32


def test_every_orb_entry_point_has_a_graph_replay_test_or_a_reason():
    """The rule of tests/test_gpu_graph_replay.py for this module: an asynchronous entry point is replayed from a graph on changed
    inputs somewhere, here in tests/test_gpu_orb.py; the rest are host-only or synchronous by contract."""
    import os
    root, protos = _orb_header()
    replayed = {"zg_orb_detect_and_compute", "zg_orb_compute"}
    host_math = {"zg_orb_default_params", "zg_orb_features_per_level", "zg_orb_adaptive_threshold"}
    missing = [ep for ep in protos if ep not in replayed and ep not in host_math and not ep.endswith("_host")]
    assert not missing, missing
    child = open(os.path.join(root, "tests", "test_gpu_orb.py")).read()
    assert "zg_graph_launch" in child and "detect_and_compute_into" in child and "lib.zg_orb_compute(" in child


# ---- the GPU suite's inputs reach every branch ----------------------------------------------------------------------------
def test_gpu_suite_inputs_cover_every_counter(oracle):
    total = dict.fromkeys(R.COUNTERS, 0)
    for img, p, what in sweep_cases()[::3] + named_cases(oracle):
        _, _, c = R.detect_and_compute_fast(img, p)
        for k in R.COUNTERS:
            total[k] += c[k]
    assert all(total[k] > 0 for k in R.COUNTERS), total
    # the named inputs, one by one: what each of them is in the suite for
    noise = oracle.synth_u8(7, (240, 320))
    p = R.Params()
    per = R.features_per_level(p)
    levels = oracle.pyramid(noise, 8, 1.2, 1.6)
    kept = [len(F.detect_fast(levels[l], R.adaptive_threshold(p, l), 9, True)) for l in range(8)]
    assert [k > n for k, n in zip(kept, per)] == [True] * 7 + [False], (kept, per)  # levels 0 .. 6 are cut and sorted, level 7 is not
    _, _, c = R.detect_and_compute_fast(noise, p)
    assert c["sorted_levels"] == 7 and c["unsorted_levels"] == 1 and c["margin_dropped"] > 0 and c["bounds_checked"] > 0 and c["oob_bits"] > 0
    _, _, c = R.detect_and_compute_fast(plateau_image(3, (200, 300)), p)
    assert c["ties_at_cut"] > 0
    photo = F.photo_like(oracle.synth_u8(5, (480, 640)))
    levels = oracle.pyramid(photo, 8, 1.2, 1.6)
    kept = [len(F.detect_fast(levels[l], R.adaptive_threshold(p, l), 9, True)) for l in range(8)]
    assert 0 in kept and any(kept), kept  # empty levels beside levels with corners
    k, _, c = R.detect_and_compute_fast(noise, R.Params(weights=tiny_weights(), n_features=200))
    assert 0 < c["m00_small"] < len(k)

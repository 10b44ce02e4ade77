"""CPU checks of the FAST detector (reference src/features/Fast.zig): the two CPU restatements agree byte for byte, the
reference's own tests hold for them, and the C ABI rejects bad arguments before touching a device. No GPU needed."""
import ctypes

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import fast_ref as F

THRESHOLDS = (0, 1, 20, 40, 254, 255)
MIN_CONTIGUOUS = (0, 1, 5, 8, 9, 12, 15, 16, 17, 32, 33)
# 8 x 8 and 9 x 9 (the smallest images), cells cut at the right and bottom edges (candidates are 6 narrower than the image)
SHAPES = ((8, 8), (9, 9), (8, 13), (17, 9), (26, 26), (27, 31), (33, 47), (46, 52), (47, 53), (64, 40))


def small_image(rng, shape, kind):
    rows, cols = shape
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "flat":
        return np.full(shape, rng.integers(0, 256), np.uint8)
    if kind == "plateau":  # few grey levels in blocks: many corners with equal scores
        levels = rng.choice(np.array([0, 60, 128, 200, 255], np.uint8), size=(rows // 3 + 1, cols // 3 + 1))
        return np.repeat(np.repeat(levels, 3, 0), 3, 1)[:rows, :cols].copy()
    if kind == "extremes":  # 0 / 255 and their neighbours: the saturating thresholds on both sides
        return rng.choice(np.array([0, 1, 2, 253, 254, 255], np.uint8), size=shape)
    raise ValueError(kind)


KINDS = ("noise", "flat", "plateau", "extremes")


def sweep_cases(seed=0):
    """Every (threshold, min_contiguous, nms) of the sweep twice, each on its own random small image: 264 cases."""
    rng = np.random.default_rng(seed)
    cases = []
    i = 0
    for t in THRESHOLDS:
        for mc in MIN_CONTIGUOUS:
            for nms in (True, False):
                for _ in range(2):
                    shape = SHAPES[i % len(SHAPES)]
                    kind = KINDS[(i // len(SHAPES)) % len(KINDS)]
                    cases.append((small_image(rng, shape, kind), t, mc, nms, f"{kind}{shape} t={t} mc={mc} nms={nms}"))
                    i += 1
    return cases


def test_keypoint_dtype_is_zg_keypoint():
    assert zg.KEYPOINT_DTYPE.itemsize == ctypes.sizeof(L.ZgKeypoint) == 28
    assert zg.KEYPOINT_DTYPE.names == ("x", "y", "size", "angle", "response", "octave", "class_id")  # KeyPoint.zig:9-28
    assert [zg.KEYPOINT_DTYPE.fields[n][1] for n in zg.KEYPOINT_DTYPE.names] == [getattr(L.ZgKeypoint, n).offset for n in zg.KEYPOINT_DTYPE.names]


def test_fast_defaults_follow_the_reference():
    f = zg.Fast()  # Fast.zig:16-24
    assert (f.threshold, f.nonmax_suppression, f.min_contiguous) == (20, True, 9)
    f = zg.Fast(threshold=25, nonmax_suppression=False, min_contiguous=12)  # "FAST detector initialization" (:256-267)
    assert (f.threshold, f.nonmax_suppression, f.min_contiguous) == (25, False, 12)


def test_literal_and_vectorised_restatements_agree():
    cases = sweep_cases()
    assert len(cases) >= 250
    nonempty = 0
    for img, t, mc, nms, what in cases:
        a = F.detect_literal(img, t, mc, nms)
        b = F.detect_fast(img, t, mc, nms)
        assert a.dtype == b.dtype == zg.KEYPOINT_DTYPE, what
        assert a.tobytes() == b.tobytes(), f"{what}: literal {len(a)} keypoints, vectorised {len(b)}"
        nonempty += len(a) > 0
    assert nonempty > len(cases) // 4  # the sweep is not all empty lists


def test_semantics_pinned_by_hand():
    # a full bright circle has arc length 32 (the walk goes round twice): min_contiguous 17 .. 32 accept it, 33 does not
    img = np.full((9, 9), 10, np.uint8)
    for dx, dy in F.CIRCLE:
        img[4 + dy, 4 + dx] = 200
    for mc in (16, 17, 32):
        k = F.detect_literal(img, 20, mc, False)
        assert [(p["y"], p["x"], p["response"]) for p in k] == [(4, 4, 16 * 190)], mc
        assert F.detect_fast(img, 20, mc, False).tobytes() == k.tobytes()
    assert len(F.detect_literal(img, 20, 33, False)) == 0 and len(F.detect_fast(img, 20, 33, False)) == 0
    # the quick reject applies to every min_contiguous: a 5-pixel bright arc on 0..4 covers only cardinals 0 and 4
    img = np.full((9, 9), 10, np.uint8)
    for i in range(5):
        dx, dy = F.CIRCLE[i]
        img[4 + dy, 4 + dx] = 200
    assert len(F.detect_literal(img, 20, 5, False)) == 0 and len(F.detect_fast(img, 20, 5, False)) == 0
    # min_contiguous 0 accepts whatever passes the quick reject; centre 250 with t = 20 saturates bright at 255 (nothing is brighter)
    img = np.full((9, 9), 250, np.uint8)
    for i in (0, 4, 8):
        dx, dy = F.CIRCLE[i]
        img[4 + dy, 4 + dx] = 255
    assert len(F.detect_fast(img, 20, 0, False)) == 0
    img[4, 4] = 200  # now 0, 4, 8 are bright: 3 cardinal pixels pass; score 3 x 55 + 13 x 50 (every term above t counts)
    k = F.detect_literal(img, 20, 0, False)
    assert (4, 4, 815) in [(p["y"], p["x"], p["response"]) for p in k]
    assert F.detect_fast(img, 20, 0, False).tobytes() == k.tobytes()


def test_equal_scores_do_not_suppress_and_suppressed_corners_still_suppress():
    rng = np.random.default_rng(5)
    for _ in range(20):
        img = small_image(rng, (40, 44), "plateau")
        a = F.detect_literal(img, 30, 9, True)
        assert a.tobytes() == F.detect_fast(img, 30, 9, True).tobytes()
        # the definition directly: kept iff no pre-suppression corner within d^2 < 25 scores strictly higher
        s = F.score_map(img, 30, 9)
        ys, xs = np.nonzero(s)
        kept = {(int(p["y"]) - 3, int(p["x"]) - 3) for p in a}
        for y, x in zip(ys, xs):
            higher = any(s[y + dy, x + dx] > s[y, x] for dy in range(-4, 5) for dx in range(-4, 5)
                         if (dx or dy) and dx * dx + dy * dy < 25 and 0 <= y + dy < s.shape[0] and 0 <= x + dx < s.shape[1])
            assert ((y, x) in kept) == (not higher)


def test_reference_synthetic_corner():
    """Fast.zig:269-317: grey 128, a dark 3 x 3 block at 7..9 and a bright one at 11..13; t = 40, no NMS: a corner within 3 of (10, 10)."""
    img = np.full((20, 20), 128, np.uint8)
    img[7:10, 7:10] = 50
    img[11:14, 11:14] = 200
    for detect in (F.detect_literal, F.detect_fast):
        k = detect(img, 40, 9, False)
        assert any(np.sqrt((p["x"] - 10) ** 2 + (p["y"] - 10) ** 2) < 3.0 for p in k)


def test_reference_nonmax_suppression():
    """Fast.zig:319-365: a (r + c) % 256 gradient with a 255 block at 20..24 and a 0 block at 30..34; NMS gives fewer keypoints."""
    r, c = np.mgrid[0:50, 0:50]
    img = ((r + c) % 256).astype(np.uint8)
    img[20:25, 20:25] = 255
    img[30:35, 30:35] = 0
    for detect in (F.detect_literal, F.detect_fast):
        assert len(detect(img, 20, 9, True)) < len(detect(img, 20, 9, False))
    assert F.detect_literal(img, 20, 9, True).tobytes() == F.detect_fast(img, 20, 9, True).tobytes()


# ---- argument checks happen before any device work -------------------------------------------------------------------
def _img(rows, cols, pixel, data=0x1000):
    return L.ZgImage(data, cols, rows, cols, pixel)


def test_fast_arguments_without_a_gpu():
    lib = zg.lib()
    n = ctypes.c_uint32(7)
    u8 = _img(32, 32, L.PIXEL_U8)
    host = lib.zg_fast_detect_host
    assert host(ctypes.byref(_img(7, 32, L.PIXEL_U8)), 20, 9, 1, None, 0, ctypes.byref(n)) == L.ERR_INVALID_ARGUMENT  # rows <= 7 (:39)
    assert host(ctypes.byref(_img(32, 7, L.PIXEL_U8)), 20, 9, 1, None, 0, ctypes.byref(n)) == L.ERR_INVALID_ARGUMENT  # cols <= 7
    assert host(ctypes.byref(u8), 256, 9, 1, None, 0, ctypes.byref(n)) == L.ERR_INVALID_ARGUMENT  # threshold: u8
    assert b"threshold" in lib.zg_last_error()
    assert host(ctypes.byref(u8), 20, 256, 1, None, 0, ctypes.byref(n)) == L.ERR_INVALID_ARGUMENT  # min_contiguous: u8
    for pixel in (L.PIXEL_F32, L.PIXEL_RGB_U8, L.PIXEL_RGBA_U8, L.PIXEL_RGBA_F32):  # Fast.detect takes Image(u8) only
        assert host(ctypes.byref(_img(32, 32, pixel)), 20, 9, 1, None, 0, ctypes.byref(n)) == L.ERR_UNSUPPORTED
    assert host(ctypes.byref(u8), 20, 9, 1, None, 4, ctypes.byref(n)) == L.ERR_INVALID_ARGUMENT  # no buffer for 4 keypoints
    assert host(ctypes.byref(u8), 20, 9, 1, None, 0, None) == L.ERR_INVALID_ARGUMENT  # no count
    assert n.value == 7  # nothing written
    # the device and batch entry points check the same before launching anything
    dev = lib.zg_fast_detect
    assert dev(ctypes.byref(_img(8, 7, L.PIXEL_U8)), 20, 9, 1, None, 0, ctypes.c_void_p(0x2000), None) == L.ERR_INVALID_ARGUMENT
    assert dev(ctypes.byref(_img(32, 32, L.PIXEL_F32)), 20, 9, 1, None, 0, ctypes.c_void_p(0x2000), None) == L.ERR_UNSUPPORTED
    assert dev(ctypes.byref(u8), 300, 9, 1, None, 0, ctypes.c_void_p(0x2000), None) == L.ERR_INVALID_ARGUMENT
    imgs = (L.ZgImage * 2)(u8, _img(6, 32, L.PIXEL_U8))
    th = (ctypes.c_uint32 * 2)(20, 17)
    caps = (ctypes.c_uint32 * 2)(0, 0)
    offs = (ctypes.c_uint64 * 2)(0, 0)
    assert lib.zg_fast_detect_batch(imgs, 2, th, 9, 1, None, caps, offs, ctypes.c_void_p(0x2000), None) == L.ERR_INVALID_ARGUMENT
    th[1] = 256
    imgs[1] = u8
    assert lib.zg_fast_detect_batch(imgs, 2, th, 9, 1, None, caps, offs, ctypes.c_void_p(0x2000), None) == L.ERR_INVALID_ARGUMENT


def test_python_binding_raises_before_device_work():
    with pytest.raises(zg.InvalidArgument):
        zg.Fast().detect(np.zeros((7, 20), np.uint8))
    with pytest.raises(zg.InvalidArgument):
        zg.Fast(threshold=300).detect(np.zeros((20, 20), np.uint8))
    with pytest.raises(zg.ZignalError):
        zg.Fast().detect(np.zeros((20, 20), np.float32))

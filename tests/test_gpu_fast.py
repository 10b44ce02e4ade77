"""FAST on the MI355X (zg_fast_detect / _host / _batch) against the CPU restatement of Fast.detect (tests/fast_ref.py): every
comparison is of the whole keypoint array's bytes, order included."""
import ctypes as C

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import fast_ref as F
from tests.test_fast_oracle import sweep_cases

torch = pytest.importorskip("torch")
KP = zg.KEYPOINT_DTYPE.itemsize


def _dev(a: np.ndarray) -> "zg.Image":
    return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def _same(got: np.ndarray, want: np.ndarray, what: str):
    assert got.dtype == want.dtype == zg.KEYPOINT_DTYPE, what
    if got.tobytes() != want.tobytes():
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i].tobytes() != want[i].tobytes()), n)
        raise AssertionError(f"{what}: {len(got)} keypoints vs {len(want)} expected; first difference at {first}: "
                             f"{got[first] if first < len(got) else None} vs {want[first] if first < len(want) else None}")


def _orb_thresholds(n_levels, fast_threshold=20, scale_factor=1.2):
    """Orb.computeAdaptiveThreshold (orb.zig:511-517): round(clamp(t / scale_factor^level, 5, 255)) per level."""
    out = []
    for level in range(n_levels):
        v = np.float32(fast_threshold) * (np.float32(1.0) / np.float32(scale_factor) ** np.float32(level))
        out.append(int(np.round(np.clip(v, np.float32(5), np.float32(255)))))
    return out


@pytest.mark.gpu
def test_small_sweep_device_and_host():
    for i, (img, t, mc, nms, what) in enumerate(sweep_cases()):
        want = F.detect_fast(img, t, mc, nms)
        fast = zg.Fast(t, nms, mc)
        _same(fast.detect(_dev(img)), want, "device " + what)
        if i % 4 == 0:
            _same(fast.detect(img), want, "host " + what)


@pytest.mark.gpu
def test_odd_shapes_and_strided_views():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (300, 517), dtype=np.uint8)
    base_dev = torch.from_numpy(base).cuda()
    for (t0, l0, rows, cols) in ((1, 3, 131, 257), (5, 1, 8, 200), (0, 7, 299, 9), (17, 11, 64, 64), (3, 5, 201, 421)):
        view = zg.Image(base_dev[t0:t0 + rows, l0:l0 + cols])  # unaligned first pixel, pitch 517
        assert view.stride == 517 and not view.is_contiguous()
        host = base[t0:t0 + rows, l0:l0 + cols]
        for t, nms in ((20, True), (40, False), (5, True)):
            want = F.detect_fast(host, t, 9, nms)
            _same(zg.Fast(t, nms).detect(view), want, f"view {t0},{l0} {rows}x{cols} t={t} nms={nms}")
            _same(zg.Fast(t, nms).detect(zg.Image(host)), want, f"host view {rows}x{cols}")


@pytest.mark.gpu
def test_frames(oracle):
    frames = [("1080p", oracle.synth_u8(41, (1080, 1920)))]
    noise = oracle.synth_u8(32, (4096, 4096))
    frames += [("4096 photo-like", F.photo_like(noise)), ("4096 noise", noise)]
    for name, img in frames:
        d = _dev(img)
        for nms in (True, False):
            want = F.detect_fast(img, 20, 9, nms)
            got = zg.Fast(20, nms).detect(d)
            _same(got, want, f"{name} nms={nms}")


@pytest.mark.gpu
def test_capacity_below_count_and_no_corners(oracle):
    img = oracle.synth_u8(7, (257, 389))
    for nms in (True, False):
        want = F.detect_fast(img, 20, 9, nms)
        assert len(want) > 100
        for cap in (0, 1, len(want) // 3, len(want) - 1, len(want)):
            kps = torch.full(((cap + 1) * KP,), 0xAB, dtype=torch.uint8, device="cuda")
            count = torch.zeros(1, dtype=torch.int32, device="cuda")
            zg.Fast(20, nms).detect_into(_dev(img), kps, count, cap)
            torch.cuda.synchronize()
            assert int(count.item()) == len(want)
            got = kps.cpu().numpy()
            _same(got[:cap * KP].view(zg.KEYPOINT_DTYPE), want[:cap], f"prefix {cap} nms={nms}")
            assert (got[cap * KP:] == 0xAB).all(), "nothing written past capacity"
    flat = _dev(np.full((100, 120), 77, np.uint8))
    for nms in (True, False):
        count = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
        zg.Fast(20, nms).detect_into(flat, torch.empty(64 * KP, dtype=torch.uint8, device="cuda"), count)
        assert int(count.item()) == 0
        assert len(zg.Fast(20, nms).detect(flat)) == 0


@pytest.mark.gpu
def test_batch_over_the_default_pyramid(oracle):
    noise = oracle.synth_u8(32, (1024, 1536))
    src = _dev(F.photo_like(noise))
    pyr = zg.ImagePyramid.build_default(src)
    torch.cuda.synchronize()
    thresholds = _orb_thresholds(pyr.n_levels)
    assert pyr.n_levels == 8 and thresholds == [20, 17, 14, 12, 10, 8, 7, 6]
    for nms in (True, False):
        fast = zg.Fast(20, nms)
        got = fast.detect_batch(pyr.levels, thresholds)
        assert len(got) == pyr.n_levels
        for lvl, (g, t) in enumerate(zip(got, thresholds)):
            single = zg.Fast(t, nms).detect(pyr.levels[lvl])
            _same(g, single, f"batch level {lvl} vs zg_fast_detect nms={nms}")
            _same(g, F.detect_fast(pyr.levels[lvl].to_numpy(), t, 9, nms), f"batch level {lvl} vs oracle nms={nms}")
        # capacities below the counts: every level's prefix and full count
        small = fast.detect_batch(pyr.levels, thresholds, capacity=3)  # reruns with the exact lengths
        for a, b in zip(small, got):
            _same(a, b, "batch rerun")


@pytest.mark.gpu
def test_graph_capture_replays_on_changed_input(oracle):
    lib = L.lib()
    a = oracle.synth_u8(3, (300, 400))
    b = F.photo_like(oracle.synth_u8(4, (300, 400)))
    src = _dev(a)
    cap = 20000
    kps = torch.zeros(cap * KP, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    d = src._desc()
    with torch.cuda.stream(stream):
        assert lib.zg_graph_begin_capture(C.c_void_p(stream.cuda_stream)) == 0
        rc = lib.zg_fast_detect(C.byref(d), 20, 9, 1, C.c_void_p(kps.data_ptr()), cap, C.c_void_p(count.data_ptr()), C.c_void_p(stream.cuda_stream))
        g = C.c_void_p()
        assert lib.zg_graph_end_capture(C.c_void_p(stream.cuda_stream), C.byref(g)) == 0, lib.zg_last_error()
        assert rc == 0
    try:
        for frame in (b, a, b):
            with torch.cuda.stream(stream):
                src.data.copy_(torch.from_numpy(frame))
                kps.fill_(0)
                count.fill_(-1)
            assert lib.zg_graph_launch(g, C.c_void_p(stream.cuda_stream)) == 0
            stream.synchronize()
            want = F.detect_fast(frame, 20, 9, True)
            n = int(count.item())
            assert n == len(want)
            _same(kps.cpu().numpy()[:n * KP].view(zg.KEYPOINT_DTYPE), want, "graph replay")
    finally:
        assert lib.zg_graph_destroy(g) == 0


@pytest.mark.gpu
def test_host_layer_count_query_then_fetch(oracle):
    lib = L.lib()
    img = np.ascontiguousarray(oracle.synth_u8(9, (211, 173)))
    d = zg.Image(img)._desc()
    want = F.detect_fast(img, 20, 9, True)
    n = C.c_uint32(0)
    assert lib.zg_fast_detect_host(C.byref(d), 20, 9, 1, None, 0, C.byref(n)) == 0
    assert n.value == len(want)
    out = np.zeros(n.value, zg.KEYPOINT_DTYPE)
    m = C.c_uint32(0)
    assert lib.zg_fast_detect_host(C.byref(d), 20, 9, 1, out.ctypes.data, n.value, C.byref(m)) == 0
    assert m.value == n.value
    _same(out, want, "host fetch")

"""ORB on the MI355X (zg_orb_detect_and_compute / zg_orb_compute and their _host forms) against the CPU restatement of
Orb.detectAndCompute (tests/orb_ref.py): every comparison is of the whole keypoint and descriptor arrays' bytes, order included."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import fast_ref as F
from tests import orb_ref as R
from tests.test_orb_oracle import hand_made_keypoints, named_cases, plateau_image, reference_synthetic_image, sweep_cases, tiny_weights

torch = pytest.importorskip("torch")
KP = zg.KEYPOINT_DTYPE.itemsize
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a: np.ndarray) -> "zg.Image":
    return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def _same(got, want, what: str):
    """got / want: (keypoints, descriptors); descriptors may be None on both sides."""
    gk, gd = got
    wk, wd = want
    assert gk.dtype == wk.dtype == zg.KEYPOINT_DTYPE, what
    if gk.tobytes() != wk.tobytes():
        n = min(len(gk), len(wk))
        first = next((i for i in range(n) if gk[i].tobytes() != wk[i].tobytes()), n)
        raise AssertionError(f"{what}: {len(gk)} keypoints vs {len(wk)} expected; first difference at {first}: "
                             f"{gk[first] if first < len(gk) else None} vs {wk[first] if first < len(wk) else None}")
    if wd is None:
        assert gd is None, what
        return
    assert gd.dtype == wd.dtype == zg.BINARY_DESCRIPTOR_DTYPE and len(gd) == len(wd), what
    if gd.tobytes() != wd.tobytes():
        first = next(i for i in range(len(wd)) if gd[i].tobytes() != wd[i].tobytes())
        raise AssertionError(f"{what}: descriptor {first} of {len(wd)} differs for {wk[first]}: {gd['bits'][first]} vs {wd['bits'][first]}")


def _orb(p: R.Params, **extra) -> "zg.Orb":
    return zg.Orb(**p.kwargs(), **extra)


def _raw(img_dev, orb, cap, with_descriptors=True, fill=0xAB):
    """zg_orb_detect_and_compute into buffers of cap + 1 entries pre-filled with `fill`; returns (count, keypoint bytes, descriptor bytes)."""
    kps = torch.full(((cap + 1) * KP,), fill, dtype=torch.uint8, device="cuda")
    des = torch.full(((cap + 1) * 32,), fill, dtype=torch.uint8, device="cuda") if with_descriptors else None
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    orb.detect_and_compute_into(img_dev, kps, des, count, cap)
    torch.cuda.synchronize()
    return int(count.item()), kps.cpu().numpy(), None if des is None else des.cpu().numpy()


@pytest.mark.gpu
def test_small_sweep_device_and_host():
    for i, (img, p, what) in enumerate(sweep_cases()):
        k, d, _ = R.detect_and_compute_fast(img, p)
        _same(_orb(p).detect_and_compute(_dev(img)), (k, d), "device " + what)
        if i % 4 == 0:
            _same(_orb(p).detect_and_compute(img), (k, d), "host " + what)
            _same((_orb(p).detect(img), None), (k, None), "host detect " + what)


@pytest.mark.gpu
def test_named_inputs_and_the_reference_synthetic_image(oracle):
    for img, p, what in named_cases(oracle):
        k, d, _ = R.detect_and_compute_fast(img, p)
        extra = {} if np.array_equal(p.weights, R.orientation_weights()) else {"orientation_weights": p.weights}
        _same(_orb(p, **extra).detect_and_compute(_dev(img)), (k, d), what)
    img = reference_synthetic_image()
    p = R.Params(n_features=50, n_levels=3, fast_threshold=10)
    k, d, _ = R.detect_and_compute_fast(img, p)
    assert len(k) > 0 and d["bits"].any()
    _same(_orb(p).detect_and_compute(_dev(img)), (k, d), "orb.zig:561-630")


@pytest.mark.gpu
def test_frames(oracle):
    """1080p noise with both score types; 4096^2 photo-like and 4096^2 noise at the defaults (one configuration each: the CPU
    restatement of a 4096^2 pyramid and its FAST lists takes the better part of a minute)."""
    hd = oracle.synth_u8(41, (1080, 1920))
    noise = oracle.synth_u8(32, (4096, 4096))
    runs = [("1080p", hd, R.Params()), ("1080p harris", hd, R.Params(harris=True)), ("1080p first_level 2", hd, R.Params(first_level=2, n_features=2000)),
            ("4096 photo-like", F.photo_like(noise), R.Params()), ("4096 noise", noise, R.Params())]
    for name, img, p in runs:
        k, d, _ = R.detect_and_compute_fast(img, p)
        assert len(k) > 0, name
        _same(_orb(p).detect_and_compute(_dev(img)), (k, d), name)


@pytest.mark.gpu
def test_strided_and_unaligned_views():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (300, 517), dtype=np.uint8)
    base_dev = torch.from_numpy(base).cuda()
    for (t0, l0, rows, cols) in ((1, 3, 131, 257), (0, 7, 299, 40), (17, 11, 64, 64), (3, 5, 201, 421)):
        view = zg.Image(base_dev[t0:t0 + rows, l0:l0 + cols])  # unaligned first pixel, pitch 517
        assert view.stride == 517 and not view.is_contiguous()
        host = base[t0:t0 + rows, l0:l0 + cols]
        for p in (R.Params(n_features=150, n_levels=4), R.Params(n_features=80, n_levels=3, scale_factor=1.5, harris=True)):
            k, d, _ = R.detect_and_compute_fast(host, p)
            _same(_orb(p).detect_and_compute(view), (k, d), f"view {t0},{l0} {rows}x{cols} harris={p.harris}")
            _same(_orb(p).detect_and_compute(zg.Image(host)), (k, d), f"host view {rows}x{cols} harris={p.harris}")


@pytest.mark.gpu
def test_budgets_of_1_5_and_beyond_every_level(oracle):
    img = oracle.synth_u8(7, (240, 320))
    for harris in (False, True):
        for nf in (1, 5, 1_000_000):
            p = R.Params(n_features=nf, harris=harris)
            k, d, c = R.detect_and_compute_fast(img, p)
            if nf == 1_000_000:
                assert c["sorted_levels"] == 0 and c["unsorted_levels"] == 8  # no level is cut: FAST's order throughout
            _same(_orb(p).detect_and_compute(_dev(img)), (k, d), f"n_features={nf} harris={harris}")
    for fl in (1, 3, 7):
        p = R.Params(first_level=fl)
        k, d, _ = R.detect_and_compute_fast(img, p)
        assert len(k) and int(k["octave"].min()) >= fl
        _same(_orb(p).detect_and_compute(_dev(img)), (k, d), f"first_level={fl}")


@pytest.mark.gpu
def test_capacity_below_count_descriptors_null_and_no_corners(oracle):
    img = oracle.synth_u8(7, (240, 320))
    p = R.Params()
    k, d, _ = R.detect_and_compute_fast(img, p)
    assert len(k) > 100
    src = _dev(img)
    for cap in (0, 1, len(k) // 3, len(k) - 1, len(k), len(k) + 7):
        n, gk, gd = _raw(src, _orb(p), cap)
        assert n == len(k)
        m = min(cap, n)
        _same((gk[:m * KP].view(zg.KEYPOINT_DTYPE), gd[:m * 32].view(zg.BINARY_DESCRIPTOR_DTYPE)), (k[:m], d[:m]), f"prefix {cap}")
        assert (gk[m * KP:] == 0xAB).all() and (gd[m * 32:] == 0xAB).all(), "nothing written past capacity or count"
    n, gk, gd = _raw(src, _orb(p), len(k), with_descriptors=False)  # Orb.detect
    assert n == len(k) and gd is None
    _same((gk[:n * KP].view(zg.KEYPOINT_DTYPE), None), (k, None), "descriptors = NULL")
    _same((_orb(p).detect(src), None), (k, None), "Orb.detect")
    flat = _dev(np.full((100, 120), 77, np.uint8))
    n, gk, _ = _raw(flat, zg.Orb(n_levels=4), 16)
    assert n == 0 and (gk == 0xAB).all()
    k0, d0 = zg.Orb(n_levels=4).detect_and_compute(flat)
    assert len(k0) == 0 and len(d0) == 0
    assert _raw(src, zg.Orb(n_features=0), 4)[0] == 0  # no level has a share


@pytest.mark.gpu
def test_compute_on_reference_and_hand_made_keypoints(oracle):
    img = oracle.synth_u8(7, (240, 320))
    for p in (R.Params(), R.Params(n_levels=4, scale_factor=1.5)):
        k, d, _ = R.detect_and_compute_fast(img, R.Params())
        want = d if p.n_levels == 8 else R.compute_fast(img, k, p)  # octaves past a shorter pyramid clamp to its last level
        for image in (_dev(img), img):
            got = _orb(p).compute(image, k)
            assert got.tobytes() == want.tobytes(), f"compute on the detector's keypoints, n_levels={p.n_levels}"
        hand = hand_made_keypoints(img.shape)
        want = R.compute_fast(img, hand, p)
        assert want["bits"].any() and not want["bits"][-1].any()
        for image in (_dev(img), img):
            got = _orb(p).compute(image, hand)
            bad = [i for i in range(len(hand)) if got[i].tobytes() != want[i].tobytes()]
            assert not bad, f"hand-made keypoints {bad} differ (n_levels={p.n_levels}): {hand[bad[0]]}"
    assert len(zg.Orb().compute(_dev(img), np.zeros(0, zg.KEYPOINT_DTYPE))) == 0


@pytest.mark.gpu
def test_weight_table_override(oracle):
    img = oracle.synth_u8(7, (240, 320))
    src = _dev(img)
    default = zg.Orb().detect_and_compute(src)
    _same(zg.Orb(orientation_weights=R.orientation_weights()).detect_and_compute(src), default, "the default table passed in")
    _same(zg.Orb(orientation_weights=R.orientation_weights()).detect_and_compute(img), default, "the default table passed in, host form")
    w = tiny_weights()
    p = R.Params(weights=w, n_features=200)
    k, d, c = R.detect_and_compute_fast(img, p)
    assert 0 < c["m00_small"] < len(k)
    _same(_orb(p, orientation_weights=w).detect_and_compute(src), (k, d), "tiny weights: m00 < 0.001 gives angle 0")
    # a caller's table is a synchronous upload: refused under capture, and the stream is left usable
    lib = L.lib()
    stream = torch.cuda.Stream()
    kps = torch.zeros(500 * KP, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        assert lib.zg_graph_begin_capture(C.c_void_p(stream.cuda_stream)) == 0
        with pytest.raises(zg.ZignalError):
            zg.Orb(orientation_weights=w).detect_and_compute_into(src, kps, None, count)
        g = C.c_void_p()
        assert lib.zg_graph_end_capture(C.c_void_p(stream.cuda_stream), C.byref(g)) == 0, lib.zg_last_error()
        assert lib.zg_graph_destroy(g) == 0


_CHILD = r"""
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import zignal_amd as zg
from zignal_amd import _lib as L
from oracle import pyoracle as oracle
from tests import fast_ref as F
from tests import orb_ref as R
from tests.test_orb_oracle import plateau_image

KP = zg.KEYPOINT_DTYPE.itemsize
lib = L.lib()
frames = [oracle.synth_u8(3, (300, 400)), F.photo_like(oracle.synth_u8(4, (300, 400))), plateau_image(8, (300, 400))]
for harris in (False, True):
    orb = zg.Orb(score_type="harris_score" if harris else "fast_score")
    src = zg.Image(torch.from_numpy(frames[0]).cuda())
    cap = 500
    kps = torch.zeros(cap * KP, dtype=torch.uint8, device="cuda")
    des = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):  # harris = False: the process's first ORB call is this recorded one
        assert lib.zg_graph_begin_capture(C.c_void_p(stream.cuda_stream)) == 0
        try:
            orb.detect_and_compute_into(src, kps, des, count, cap)
        finally:
            g = C.c_void_p()
            rc = lib.zg_graph_end_capture(C.c_void_p(stream.cuda_stream), C.byref(g))
        assert rc == 0, lib.zg_last_error()
    for i in (1, 0, 2, 1):
        with torch.cuda.stream(stream):
            src.data.copy_(torch.from_numpy(frames[i]))
            kps.fill_(0)
            des.fill_(0)
            count.fill_(-1)
        assert lib.zg_graph_launch(g, C.c_void_p(stream.cuda_stream)) == 0
        stream.synchronize()
        k, d, _ = R.detect_and_compute_fast(frames[i], R.Params(harris=harris))
        n = int(count.item())
        assert n == len(k), (harris, i, n, len(k))
        assert kps.cpu().numpy()[:n * KP].tobytes() == k.tobytes(), ("replayed keypoints", harris, i)
        assert des.cpu().numpy()[:n * 32].tobytes() == d.tobytes(), ("replayed descriptors", harris, i)
        ek, ed = orb.detect_and_compute(zg.Image(torch.from_numpy(frames[i]).cuda()))  # eager, same input
        assert ek.tobytes() == k.tobytes() and ed.tobytes() == d.tobytes(), ("eager", harris, i)
    assert lib.zg_graph_destroy(g) == 0

# zg_orb_compute recorded once, replayed on changed pixels and changed keypoints in the same buffers
p = L.ZgOrbParams()
lib.zg_orb_default_params(C.byref(p))
src = zg.Image(torch.from_numpy(frames[0]).cuda())
n = 64
lists = []
for f in frames:  # n keypoints per frame: the detector's own, repeated where a frame has fewer
    k = R.detect_and_compute_fast(f, R.Params())[0]
    assert len(k) > 0
    k = np.resize(k, n)
    lists.append((k, R.compute_fast(f, k, R.Params())))
dk = torch.zeros(n * KP, dtype=torch.uint8, device="cuda")
dd = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
stream = torch.cuda.Stream()
torch.cuda.synchronize()
d = src._desc()
with torch.cuda.stream(stream):
    assert lib.zg_graph_begin_capture(C.c_void_p(stream.cuda_stream)) == 0
    rc = lib.zg_orb_compute(C.byref(d), C.byref(p), C.c_void_p(dk.data_ptr()), n, C.c_void_p(dd.data_ptr()), C.c_void_p(stream.cuda_stream))
    g = C.c_void_p()
    assert lib.zg_graph_end_capture(C.c_void_p(stream.cuda_stream), C.byref(g)) == 0, lib.zg_last_error()
    assert rc == 0, lib.zg_last_error()
for i in (1, 0, 2):
    k, want = lists[i]
    with torch.cuda.stream(stream):
        src.data.copy_(torch.from_numpy(frames[i]))
        dk.copy_(torch.from_numpy(k[:n].view(np.uint8).reshape(-1).copy()))
        dd.fill_(0xAB)
    assert lib.zg_graph_launch(g, C.c_void_p(stream.cuda_stream)) == 0
    stream.synchronize()
    assert dd.cpu().numpy().tobytes() == want[:n].tobytes(), ("replayed zg_orb_compute", i)
assert lib.zg_graph_destroy(g) == 0
print("graph ok")
"""


@pytest.mark.gpu
def test_graph_capture_as_the_first_orb_call_of_a_process(tmp_path):
    """A fresh child process (started, not exec'ed into) whose first ORB call is recorded into a graph, replayed on changed inputs of
    the same shape and compared with the restatement and with eager calls. The child has ten minutes."""
    script = tmp_path / "orb_graph_child.py"
    script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "graph ok" in r.stdout, f"child exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.gpu
def test_two_streams_on_different_images(oracle):
    imgs = [oracle.synth_u8(21, (480, 640)), plateau_image(5, (360, 500))]
    params = [R.Params(), R.Params(harris=True, n_features=300)]
    want = [R.detect_and_compute_fast(i, p)[:2] for i, p in zip(imgs, params)]
    srcs = [_dev(i) for i in imgs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [(torch.zeros(500 * KP, dtype=torch.uint8, device="cuda"), torch.zeros(500 * 32, dtype=torch.uint8, device="cuda"),
             torch.zeros(1, dtype=torch.int32, device="cuda")) for _ in imgs]
    torch.cuda.synchronize()
    for _ in range(6):  # both streams stay busy: each call is enqueued behind the other stream's, none is waited for
        for s, src, p, (kps, des, count) in zip(streams, srcs, params, bufs):
            with torch.cuda.stream(s):
                _orb(p).detect_and_compute_into(src, kps, des, count, 500)
    torch.cuda.synchronize()
    for (kps, des, count), (k, d), name in zip(bufs, want, ("noise on stream 0", "plateau, harris on stream 1")):
        n = int(count.item())
        assert n == len(k), name
        _same((kps.cpu().numpy()[:n * KP].view(zg.KEYPOINT_DTYPE), des.cpu().numpy()[:n * 32].view(zg.BINARY_DESCRIPTOR_DTYPE)), (k, d), name)


@pytest.mark.gpu
def test_host_layer_count_query_then_fetch(oracle):
    lib = L.lib()
    img = np.ascontiguousarray(oracle.synth_u8(9, (211, 273)))
    d = zg.Image(img)._desc()
    k, de, _ = R.detect_and_compute_fast(img, R.Params())
    p = L.ZgOrbParams()
    lib.zg_orb_default_params(C.byref(p))
    n = C.c_uint32(0)
    assert lib.zg_orb_detect_and_compute_host(C.byref(d), C.byref(p), None, None, 0, C.byref(n)) == 0
    assert n.value == len(k)
    ok, od = np.zeros(n.value, zg.KEYPOINT_DTYPE), np.zeros(n.value, zg.BINARY_DESCRIPTOR_DTYPE)
    m = C.c_uint32(0)
    assert lib.zg_orb_detect_and_compute_host(C.byref(d), C.byref(p), ok.ctypes.data, od.ctypes.data, n.value, C.byref(m)) == 0
    assert m.value == n.value
    _same((ok, od), (k, de), "host fetch")

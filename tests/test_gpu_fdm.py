"""Feature distribution matching on the device (include/zignal_hip_fdm.h) stage by stage, each against what pins it:
  moments   numpy uint64 sums, by equality
  solve     the device kernels against the library's host forms fed the statistics the device derives (bitwise); the host forms
            themselves are held to tests/fdm_ref.py by tests/test_fdm_solve_host.py
  apply     tests/fdm_ref.py's bytes for transforms computed from Welford statistics and uploaded
  chains    tests/fdm_ref.py end to end (Welford statistics) by plain byte equality, on inputs guarded as follows.
The device takes its statistics from exact moments, the reference from Welford's recurrence. On the end-to-end frames below the two paths
move 255 * clamp(res), the value before @round, by at most 5.4e-13 (measured with the restatement and zg_fdm_stats_from_moments_host;
profiles/fdm_bench.txt). The tie guard DELTA is 100 times that. Every end-to-end case first asserts on the CPU that the restatement alone
has no value within DELTA of a half-integer and no variance or singular value within a factor 10 of the 1e-10 guards, and that the
restatement fed exact-moment statistics (host arithmetic) gives the same bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fdm_cases as K
from tests import fdm_ref as R

torch = pytest.importorskip("torch")

import zignal_amd as zg  # noqa: E402
from zignal_amd import _lib as L  # noqa: E402
from zignal_amd import fdm  # noqa: E402

DELTA = 100 * 5.4e-13
PIXEL_OF = {1: L.PIXEL_U8, 3: L.PIXEL_RGB_U8, 4: L.PIXEL_RGBA_U8}
ROW_GROUPS = 2048  # fdm.hip's TARGET_BLOCKS: a frame of one strip is cut into min(rows, 2048) row groups, a lane taking every 2048th row


def dev(a):
    return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def host(image):
    return image.data.cpu().numpy()


def pixel_of(a):
    return L.PIXEL_U8 if a.ndim == 2 else PIXEL_OF[a.shape[2]]


def random_frame(rng, rows, cols, ch):
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def moments_equal(rec, a):
    want = R.moments(a)
    got = {"n": rec.n, "sum": list(rec.sum), "prod": list(rec.prod), "lum_sum": rec.lum_sum, "lum_sq": rec.lum_sq, "not_gray": rec.not_gray}
    assert got == want and rec.pixel == pixel_of(a)


# ---- moments ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_moments_equal_numpy_sums(ch):
    rng = np.random.default_rng(100 + ch)
    for rows, cols in ((1, 1), (1, 7), (3, 5), (64, 64), (257, 300)):  # 257 x 300: a workgroup a row, more than one wave, a partial last group
        a = random_frame(rng, rows, cols, ch)
        moments_equal(fdm.moments_to_host(fdm.compute_moments(dev(a)))[0], a)
    wide = random_frame(rng, 3, 4100 if ch == 1 else 1030, ch)  # a second strip of 256 groups
    moments_equal(fdm.moments_to_host(fdm.compute_moments(dev(wide)))[0], wide)


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_moments_of_a_view_read_the_rectangle_only(ch):
    rng = np.random.default_rng(110 + ch)
    big = random_frame(rng, 40, 61, ch)
    image = dev(big).view((5, 3, 5 + 33, 3 + 17))  # 17 x 33 at (3, 5): rows start at every alignment
    assert (image.rows, image.cols, image.stride) == (17, 33, 61)
    moments_equal(fdm.moments_to_host(fdm.compute_moments(image))[0], big[3:20, 5:38])


@pytest.mark.gpu
def test_moments_flush_the_lane_partials_before_they_wrap():
    """A lane adds 16 bytes of a u8 row a step and widens its u32 partial sums every zg_fdm_lane_run() steps. A 16-column frame is one group
    wide, so one lane of each of the 2048 row groups walks rows / 2048 steps: 2 * run + 104 = 4200 steps flush twice inside the loop, and
    4200 * 16 * 255^2 is past 2^32, so a partial that was never widened would wrap."""
    run = zg.lib().zg_fdm_lane_run()
    steps = 2 * run + 104
    assert run * 16 * 65025 < 2 ** 32 < steps * 16 * 65025
    rows = ROW_GROUPS * steps
    frame = zg.Image(torch.full((rows, 16), 255, dtype=torch.uint8, device="cuda"))
    rec = fdm.moments_to_host(fdm.compute_moments(frame))[0]
    n = rows * 16
    assert (rec.n, rec.lum_sum, rec.lum_sq, rec.not_gray) == (n, 255 * n, 65025 * n, 0)
    del frame
    # the same for a colour lane: 4 pixels a step, 4 * 255^2 a step into each product
    rows = ROW_GROUPS * (2 * run + 8)
    frame = zg.Image(torch.full((rows, 4, 3), 255, dtype=torch.uint8, device="cuda"))
    rec = fdm.moments_to_host(fdm.compute_moments(frame))[0]
    n = rows * 4
    assert rec.n == n and list(rec.sum) == [255 * n] * 3 and list(rec.prod) == [65025 * n] * 6 and (rec.lum_sum, rec.lum_sq) == (255 * n, 65025 * n)


@pytest.mark.gpu
def test_moments_product_sums_pass_2_to_32():
    frame = zg.Image(torch.full((2048, 2048, 4), 255, dtype=torch.uint8, device="cuda"))
    rec = fdm.moments_to_host(fdm.compute_moments(frame))[0]
    n = 2048 * 2048
    assert 65025 * n > 2 ** 32
    assert rec.n == n and list(rec.sum) == [255 * n] * 3 and list(rec.prod) == [65025 * n] * 6 and (rec.lum_sum, rec.lum_sq) == (255 * n, 65025 * n)
    assert rec.not_gray == 0


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [3, 4])
def test_not_gray_word(ch):
    rng = np.random.default_rng(120 + ch)
    plane = rng.integers(0, 256, size=(37, 53), dtype=np.uint8)
    a = np.repeat(plane[..., None], ch, 2)
    if ch == 4:
        a[..., 3] = rng.integers(0, 256, size=(37, 53), dtype=np.uint8)  # alpha takes no part
    assert fdm.moments_to_host(fdm.compute_moments(dev(a)))[0].not_gray == 0
    a[-1, -1, 2] ^= 1  # grey but for its last pixel
    rec = fdm.moments_to_host(fdm.compute_moments(dev(a)))[0]
    assert rec.not_gray != 0
    moments_equal(rec, a)


@pytest.mark.gpu
def test_moments_frames_of_different_sizes_and_types():
    rng = np.random.default_rng(130)
    frames = [random_frame(rng, 19, 23, 3), random_frame(rng, 64, 70, 4), random_frame(rng, 5, 1100, 1)]
    recs = fdm.moments_to_host(fdm.compute_moments([dev(f) for f in frames]), 3)
    for rec, f in zip(recs, frames):
        moments_equal(rec, f)


# ---- solve -----------------------------------------------------------------------------------------------------------------------------

def moments_record(pixel, n, sums, prod, lum=(0, 0), not_gray=1):
    rec = L.ZgFdmMoments()
    rec.n = n
    for i in range(3):
        rec.sum[i] = sums[i]
    for i in range(6):
        rec.prod[i] = prod[i]
    rec.lum_sum, rec.lum_sq = lum
    rec.not_gray = not_gray
    rec.pixel = pixel
    return rec


def host_solve(target_rec, source_recs):
    """The library's host forms on the statistics the device derives from the same moments."""
    pixel = target_rec.pixel
    gray = pixel == L.PIXEL_U8 or target_rec.not_gray == 0
    tm, tc = fdm.stats_from_moments(target_rec, pixel == L.PIXEL_U8)
    t = fdm.target_host(pixel, tm, tc, gray)
    xs = []
    for rec in source_recs:
        sm, sc = fdm.stats_from_moments(rec, pixel == L.PIXEL_U8 or gray)
        xs.append(fdm.transform_host(pixel, t, sm, sc))
    return t, xs


def device_solve(target_rec, source_recs):
    n = len(source_recs)
    arr = (L.ZgFdmMoments * (n + 1))(*source_recs, target_rec)
    m = fdm.upload(arr)
    t = torch.zeros(C.sizeof(L.ZgFdmTarget), dtype=torch.uint8, device="cuda")
    x = torch.zeros(n * C.sizeof(L.ZgFdmTransform), dtype=torch.uint8, device="cuda")
    size = C.sizeof(L.ZgFdmMoments)
    lib = zg.lib()
    L.check(lib.zg_fdm_target_from_moments(C.c_void_p(m.data_ptr() + n * size), C.c_void_p(t.data_ptr()), stream()))
    L.check(lib.zg_fdm_transform_from_moments_frames(C.c_void_p(m.data_ptr()), n, C.c_void_p(t.data_ptr()), C.c_void_p(x.data_ptr()), stream()))
    return fdm._to_host(t, L.ZgFdmTarget, 1)[0], fdm._to_host(x, L.ZgFdmTransform, n), m, t


@pytest.mark.gpu
def test_device_solve_is_bitwise_the_host_forms_over_the_covariance_families():
    """Moments built to produce each family's covariance (tests/fdm_cases.py: moments_for) go through k_target and k_transform; the host
    forms get the statistics zg_fdm_stats_from_moments_host derives from the same words."""
    mats = K.covariance_matrices()
    sources = [moments_record(L.PIXEL_RGB_U8, *K.moments_for(c)) for _, c in mats]
    families = sorted({f for f, _ in mats})
    seen = set()
    for family in families:
        picks = [c for f, c in mats if f == family][:2]
        for c in picks:
            target = moments_record(L.PIXEL_RGB_U8, *K.moments_for(c, n=1777, s=200000))
            want_t, want_x = host_solve(target, sources)
            got_t, got_x, _, _ = device_solve(target, sources)
            assert bytes(got_t) == bytes(want_t), family
            for i, (g, w) in enumerate(zip(got_x, want_x)):
                assert bytes(g) == bytes(w), (family, i)
                seen.add(w.route)
    assert seen == {L.FDM_ROUTE_COLOR}


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", [L.PIXEL_U8, L.PIXEL_RGB_U8, L.PIXEL_RGBA_U8])
def test_device_solve_scalar_routes_are_bitwise_the_host_forms(pixel):
    rng = np.random.default_rng(140 + pixel)
    recs = []
    for k in range(40):
        n = int(rng.integers(2, 100000)) if k else 1
        v = rng.integers(0, 256, size=min(n, 4000)).astype(object)
        scale = n // len(v)
        s, ss = int(v.sum()) * scale, int((v * v).sum()) * scale  # any words inside the bounds do
        n = len(v) * scale
        recs.append(moments_record(pixel, n, [s, s, s], [ss] * 6, lum=(s, ss), not_gray=0))
    recs.append(moments_record(pixel, 500, [500 * 77] * 3, [500 * 77 * 77] * 6, lum=(500 * 77, 500 * 77 * 77), not_gray=0))  # a constant frame: scale = 1
    want_t, want_x = host_solve(recs[3], recs)
    got_t, got_x, _, _ = device_solve(recs[3], recs)
    assert bytes(got_t) == bytes(want_t) and got_t.is_gray == 1
    route = L.FDM_ROUTE_SCALAR if pixel == L.PIXEL_U8 else L.FDM_ROUTE_GRAY_TARGET
    for g, w in zip(got_x, want_x):
        assert bytes(g) == bytes(w) and g.route == route and g.status == 0
    assert got_x[-1].scale == 1.0


@pytest.mark.gpu
def test_nonzero_status_leaves_the_frame_untouched():
    rng = np.random.default_rng(150)
    a = random_frame(rng, 37, 53, 3)
    image = dev(a)
    x = L.ZgFdmTransform()
    x.route, x.status, x.scale = L.FDM_ROUTE_COLOR, 2, 1.0  # as after error.NotConverged: W is all zeros
    fdm.apply(image, fdm.upload(x))
    assert np.array_equal(host(image), a)
    # a target of another pixel type: the transform kernel says so in the status, and apply does nothing
    target = moments_record(L.PIXEL_RGBA_U8, *K.moments_for(np.diag([0.02, 0.01, 0.03])))
    source = moments_record(L.PIXEL_RGB_U8, *K.moments_for(np.diag([0.01, 0.01, 0.01])))
    _, xs, m, t = device_solve(target, [source])
    assert xs[0].status == L.FDM_STATUS_TYPE_MISMATCH
    xd = torch.zeros(C.sizeof(L.ZgFdmTransform), dtype=torch.uint8, device="cuda")
    L.check(zg.lib().zg_fdm_transform_from_moments(C.c_void_p(m.data_ptr()), L.PIXEL_RGB_U8, C.c_void_p(t.data_ptr()), C.c_void_p(xd.data_ptr()), stream()))
    fdm.apply(image, xd)
    assert np.array_equal(host(image), a)


# ---- apply -----------------------------------------------------------------------------------------------------------------------------

def transform_record(x):
    rec = L.ZgFdmTransform()
    rec.route, rec.status = x["route"], 0
    for i in range(3):
        for j in range(3):
            rec.w[i * 3 + j] = x["w"][i][j]
        rec.bias[i] = x["bias"][i]
    rec.scale, rec.offset = x["scale"], x["offset"]
    return rec


_APPLY = {}


def apply_case(route, ch, shape):
    """(source, transform, expected) for a route and pixel type, the transform from Welford statistics; computed once."""
    key = (route, ch, shape)
    if key not in _APPLY:
        rng = np.random.default_rng(200 + 10 * route + ch + shape[0])
        rows, cols = shape
        if ch == 1:
            src = np.clip(np.rint(rng.normal(128, 50, size=shape)), 0, 255).astype(np.uint8)
            tgt = np.clip(np.rint(rng.normal(100, 25, size=(20, 20))), 0, 255).astype(np.uint8)
        else:
            src = K.correlated_rgb(rng, rows, cols, spread=60.0)
            tgt = K.correlated_rgb(rng, 24, 20, base=(100, 90, 160), spread=25.0)
            if route == R.ROUTE_GRAY_TARGET:
                tgt = np.repeat(tgt[..., :1], 3, 2)
            if ch == 4:
                src = np.dstack([src, rng.integers(1, 256, size=(rows, cols, 1), dtype=np.uint8)])
                tgt = np.dstack([tgt, rng.integers(0, 256, size=tgt.shape[:2] + (1,), dtype=np.uint8)])
        x = R.source_transform(src, R.prepare_target(tgt))
        assert x["route"] == route
        _APPLY[key] = (src, x, R.apply(src, x))
    return _APPLY[key]


ROUTES = [(R.ROUTE_SCALAR, 1), (R.ROUTE_COLOR, 3), (R.ROUTE_COLOR, 4), (R.ROUTE_GRAY_TARGET, 3), (R.ROUTE_GRAY_TARGET, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("route,ch", ROUTES)
@pytest.mark.parametrize("shape", [(64, 64), (37, 53)])
def test_apply_equals_the_restatement_on_every_pixel(route, ch, shape):
    src, x, want = apply_case(route, ch, shape)
    image = dev(src)
    fdm.apply(image, fdm.upload(transform_record(x)))
    got = host(image)
    assert np.array_equal(got, want)
    if ch == 4:
        assert np.array_equal(got[..., 3], src[..., 3]) if route == R.ROUTE_COLOR else not got[..., 3].any()
        assert src[..., 3].all()  # so a zeroed alpha is a written one


@pytest.mark.gpu
@pytest.mark.parametrize("route,ch", ROUTES)
def test_apply_clamps_at_both_ends(route, ch):
    src, x, _ = apply_case(route, ch, (37, 53))
    wide = dict(x)
    wide["w"] = [[5.0 * v for v in row] for row in x["w"]]  # res -> 5 res - 2: below 0 under 0.4, above 1 over 0.6
    wide["scale"] = 5.0 * x["scale"]
    wide["bias"] = [5.0 * b - 2.0 for b in x["bias"]]
    wide["offset"] = 5.0 * x["offset"] - 2.0
    want = R.apply(src, wide)
    colour = want if ch == 1 else want[..., :3]
    assert (colour == 0).any() and (colour == 255).any()
    image = dev(src)
    fdm.apply(image, fdm.upload(transform_record(wide)))
    assert np.array_equal(host(image), want)


@pytest.mark.gpu
@pytest.mark.parametrize("route,ch", ROUTES)
def test_apply_on_a_view_writes_nothing_outside(route, ch):
    src, x, _ = apply_case(route, ch, (37, 53))
    rng = np.random.default_rng(260 + ch)
    big = random_frame(rng, 50, 70, ch)
    big[6:43, 9:62] = src
    want = big.copy()
    want[6:43, 9:62] = R.apply(src, x)
    image = dev(big)
    fdm.apply(image.view((9, 6, 62, 43)), fdm.upload(transform_record(x)))
    assert np.array_equal(host(image), want)


@pytest.mark.gpu
def test_apply_frames_takes_a_transform_a_frame():
    cases = [apply_case(R.ROUTE_COLOR, 3, (37, 53)), apply_case(R.ROUTE_SCALAR, 1, (64, 64)), apply_case(R.ROUTE_GRAY_TARGET, 4, (37, 53))]
    images = [dev(c[0]) for c in cases]
    arr = (L.ZgFdmTransform * 3)(*[transform_record(c[1]) for c in cases])
    fdm.apply(images, fdm.upload(arr))
    for image, c in zip(images, cases):
        assert np.array_equal(host(image), c[2])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

_E2E = {}


def e2e(name):
    """(source, target, expected) of an end-to-end case, after the CPU guards."""
    if not _E2E:
        for case_name, src, tgt in K.end_to_end_cases():
            target = R.prepare_target(tgt)
            x = R.source_transform(src, target)
            want, pre = R.apply(src, x, return_pre=True)
            assert float(np.min(np.abs((pre - np.floor(pre)) - 0.5))) > DELTA, case_name
            guarded = list(target["s"]) + list(x.get("source_s", []))
            if x["route"] != R.ROUTE_COLOR:
                guarded.append(R.image_stats(src, as_luminance=src.ndim == 3)[1][0][0])
            assert all(v == 0.0 or not (1e-11 < v < 1e-9) for v in guarded), (case_name, guarded)
            # one guard more than the tie and the 1e-10 ones: no sign decision of the SVD (svd.zig:216, :244) hangs on Welford's rounding
            # noise. It does where a covariance is exactly 0, as between the r and g of fdm.zig's own 50 x 50 test pattern: the recurrence
            # leaves 1.6e-19 there, whose sign then decides the sign of a column of U, and the two statistics paths give different images.
            assert np.array_equal(K.match_with_exact_statistics(src, tgt), want), case_name
            _E2E[case_name] = (src, tgt, want)
    return _E2E[name]


E2E_NAMES = [name for name, _, _ in K.end_to_end_cases()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", E2E_NAMES)
def test_match_equals_the_welford_restatement(name):
    src, tgt, want = e2e(name)
    a, t = dev(src), dev(tgt)
    da, dt = a._desc(), t._desc()
    L.check(zg.lib().zg_fdm_match(C.byref(da), C.byref(dt), stream()))
    assert np.array_equal(host(a), want)
    assert np.array_equal(host(t), tgt)
    b = dev(src)
    assert zg.FeatureDistributionMatching().match(b, dev(tgt)) is b and np.array_equal(host(b), want)
    c = dev(src)
    m = zg.FeatureDistributionMatching().set_target(dev(tgt))
    m.set_source(c)
    m.update()
    assert np.array_equal(host(c), want)
    h = src.copy()  # the host form
    zg.FeatureDistributionMatching().match(zg.Image(h), zg.Image(tgt.copy()))
    assert np.array_equal(h, want)


@pytest.mark.gpu
def test_match_frames_equals_single_matches():
    rng = np.random.default_rng(300)
    _, tgt, _ = e2e("rgb_to_rgb")
    frames = [K.correlated_rgb(rng, rows, cols, base=base) for rows, cols, base in
              ((33, 47, (100, 100, 100)), (64, 64, (60, 150, 90)), (7, 300, (200, 80, 120)), (50, 21, (90, 90, 160)), (1, 5, (128, 128, 128)))]
    single = []
    for f in frames:
        image = dev(f)
        zg.FeatureDistributionMatching().match(image, dev(tgt))
        single.append(host(image))
    batch = [dev(f) for f in frames]
    zg.FeatureDistributionMatching().match_frames(batch, dev(tgt))
    for got, want, f in zip(batch, single, frames):
        assert np.array_equal(host(got), want) and not np.array_equal(want, f)
    # the C entry with the target as an image, and more frames than one launch serves
    many = [dev(frames[k % 5]) for k in range(zg.lib().zg_fdm_frames_per_launch() + 3)]
    descs = fdm._descs(many)
    t = dev(tgt)
    td = t._desc()
    L.check(zg.lib().zg_fdm_match_frames(descs, len(many), C.byref(td), None, stream()))
    for k, image in enumerate(many):
        assert np.array_equal(host(image), single[k % 5]), k


# ---- graph capture and replay, two streams ----------------------------------------------------------------------------------------------

def graph_replay():
    """Captures the match chain as the first library call of the process on one pair of frames, and replays it on changed contents."""
    for name in ("rgb_to_rgb", "u8_to_u8"):
        src, tgt, want = e2e(name)
        a = torch.zeros(src.shape, dtype=torch.uint8, device="cuda")
        t = torch.zeros(tgt.shape, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        a.copy_(torch.from_numpy(src))
        t.copy_(torch.from_numpy(tgt))
        torch.cuda.synchronize()
        matcher = zg.FeatureDistributionMatching()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            matcher.match(zg.Image(a), zg.Image(t))
        # the second contents: the frames' bytes change, their shapes cannot
        src2 = np.ascontiguousarray(np.flip(src, 0))
        tgt2 = (255 - tgt).astype(np.uint8)
        want2 = R.match(src2, tgt2)
        assert not np.array_equal(want2, np.flip(want, 0))
        for s_np, t_np, w in ((src, tgt, want), (src2, tgt2, want2), (src, tgt, want)):
            a.copy_(torch.from_numpy(s_np))
            t.copy_(torch.from_numpy(t_np))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(a.cpu().numpy(), w), name
        del graph
        torch.cuda.synchronize()
        assert zg.lib().zg_release_graph_scratch() == 0


@pytest.mark.gpu
def test_match_is_captured_as_a_fresh_process_first_call_and_replays_on_changed_contents():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_fdm import graph_replay; graph_replay(); print('ok')"], capture_output=True, text=True,
                         timeout=300, cwd=root)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_two_streams_match_at_once():
    cases = [e2e("rgb_to_rgb"), e2e("rgba_gray_target")]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    images = [[dev(c[0]) for _ in range(6)] for c in cases]
    targets = [dev(c[1]) for c in cases]
    torch.cuda.synchronize()
    for k in range(6):
        for s, c, row, t in zip(streams, cases, images, targets):
            with torch.cuda.stream(s):
                zg.FeatureDistributionMatching().match(row[k], t)
    torch.cuda.synchronize()
    for c, row in zip(cases, images):
        for image in row:
            assert np.array_equal(host(image), c[2])


# ---- errors --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals():
    f32 = zg.Image(torch.zeros((4, 4, 3), dtype=torch.float32, device="cuda"))
    u8 = dev(np.zeros((4, 4), np.uint8))
    rgb = dev(np.zeros((4, 4, 3), np.uint8))
    lib = zg.lib()
    for a, b, status in ((f32, f32, L.ERR_UNSUPPORTED), (rgb, f32, L.ERR_UNSUPPORTED), (rgb, u8, L.ERR_INVALID_ARGUMENT), (u8, rgb, L.ERR_INVALID_ARGUMENT)):
        da, db = a._desc(), b._desc()
        assert lib.zg_fdm_match(C.byref(da), C.byref(db), stream()) == status
    m = torch.zeros(C.sizeof(L.ZgFdmMoments), dtype=torch.uint8, device="cuda")
    d = f32._desc()
    assert lib.zg_fdm_compute_moments(C.byref(d), C.c_void_p(m.data_ptr()), stream()) == L.ERR_UNSUPPORTED
    assert lib.zg_fdm_apply(C.byref(d), C.c_void_p(m.data_ptr()), stream()) == L.ERR_UNSUPPORTED
    matcher = zg.FeatureDistributionMatching()
    with pytest.raises(zg.NoTargetSet):
        matcher.update()
    with pytest.raises(L.ZignalError):
        matcher.set_target(f32)
    matcher.set_target(rgb)
    with pytest.raises(zg.NoSourceSet):
        matcher.update()
    matcher.set_source(u8)
    with pytest.raises(zg.InvalidArgument):
        matcher.update()
    matcher.set_source(rgb)
    matcher.update()
    torch.cuda.synchronize()
    assert not host(rgb).any()  # a constant frame against itself

"""ImagePyramid.build and Image.sobel. Oracle pins (CPU) cite the reference's tests; the GPU
tests compare the product with the oracle bit for bit."""
import numpy as np
import pytest

import zignal_amd as zg
from tests.util import ALL_TYPES, assert_bits_equal, synth


# ---- oracle pins (reference src/image/tests/filters.zig:548-570, src/image/pyramid.zig:176-276) ----------------
def test_oracle_sobel_vertical_edge(oracle):
    img = np.zeros((5, 5), np.uint8)
    img[:, 2:] = 255
    e = oracle.sobel(img)
    assert e[2, 2] > 200 and e[2, 0] < 50
    assert e[2, 2] == 255  # |gx| = 4 * 255 at the edge -> 1020 / 4 = 255


def test_oracle_pyramid_basic(oracle):
    r, c = np.mgrid[0:640, 0:480]
    img = ((r + c) % 256).astype(np.uint8)
    levels = oracle.pyramid(img, 5, 1.5, 1.0)
    assert len(levels) == 5 and levels[0].shape == (640, 480)
    for i in range(1, 5):
        assert levels[i].shape[0] < levels[i - 1].shape[0] and levels[i].shape[1] < levels[i - 1].shape[1]
        scale = 1.5 ** i
        assert abs(640 / levels[i].shape[0] - scale) < 1.0 and abs(480 / levels[i].shape[1] - scale) < 1.0


def test_oracle_pyramid_truncation_and_size(oracle):
    levels = oracle.pyramid(np.zeros((32, 32), np.uint8), 10, 2.0, 1.0)
    assert len(levels) < 10 and min(levels[-1].shape) >= 8
    levels = oracle.pyramid(np.zeros((256, 256), np.uint8), 4, 1.5, 1.0)
    total = sum(l.shape[0] * l.shape[1] for l in levels)
    assert 65536 < total < 2 * 65536
    l = oracle.lib()
    l.zo_pyramid_scale.restype = __import__("ctypes").c_float
    for lvl, want in ((0, 1.0), (1, 1.2), (2, 1.44), (3, 1.728)):
        assert abs(l.zo_pyramid_scale(__import__("ctypes").c_float(1.2), lvl) - want) < 0.01


def test_library_pyramid_arithmetic_matches_oracle(oracle):
    import ctypes as C
    lib, l = zg.lib(), oracle.lib()
    l.zo_pyramid_scale.restype = C.c_float
    for sf in (1.2, 1.5, 2.0, 1.1):
        for lvl in range(0, 12):
            a, b = lib.zg_pyramid_scale(C.c_float(sf), lvl), l.zo_pyramid_scale(C.c_float(sf), lvl)
            assert a == b
            r1, c1, s1, r2, c2, s2 = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_uint32(), C.c_uint32(), C.c_float()
            lib.zg_pyramid_level(1080, 1920, C.c_float(a), C.c_float(1.6), C.byref(r1), C.byref(c1), C.byref(s1))
            l.zo_pyramid_level(1080, 1920, C.c_float(b), C.c_float(1.6), C.byref(r2), C.byref(c2), C.byref(s2))
            assert (r1.value, c1.value) == (r2.value, c2.value) and (s1.value == s2.value or (s1.value != s1.value and s2.value != s2.value))


# ---- GPU parity ----------------------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")


def dev(a):
    return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ALL_TYPES)
def test_sobel_parity(oracle, kind):
    for shape in ((1, 1), (5, 5), (3, 70), (67, 129), (256, 300)):
        src = synth(oracle, kind, 80, *shape)
        if src.dtype == np.float32 and kind == "f32":
            src = src * np.float32(255)
        out = dev(src).sobel()
        torch.cuda.synchronize()
        assert_bits_equal(out.to_numpy(), oracle.sobel(src), f"sobel {kind} {shape}")
    img = np.zeros((5, 5), np.uint8)
    img[:, 2:] = 255
    e = zg.Image(img).sobel().data  # host layer; tests/filters.zig:548-570
    assert e[2, 2] > 200 and e[2, 0] < 50
    with pytest.raises(zg.DimensionMismatch):
        zg.Image(img).sobel(out=zg.Image(np.zeros((5, 6), np.uint8)))


@pytest.mark.gpu
def test_sobel_register_stream_kernel(oracle):
    """k_sobel_stream (sobel_stream.hip): u8 and Rgba(u8) sources whose rows are multiples of 16 bytes — one and several strips across
    and down, rows that end inside a strip, saturated patterns (the largest gradients: |gx| = |gy| = 1020), a view with the parent's
    pitch, and a batch through the pipeline's edges step."""
    rng = np.random.default_rng(12)
    for kind, shapes in (("u8", [(16, 64), (33, 1040), (50, 2064), (130, 4096)]), ("rgba_u8", [(16, 64), (40, 300), (97, 260), (64, 1028), (300, 516)])):
        for shape in shapes:
            full = shape + ((4,) if kind == "rgba_u8" else ())
            for what in ("random", "checker", "steps"):
                if what == "random":
                    src = rng.integers(0, 256, full, dtype=np.uint8)
                elif what == "checker":
                    yy, xx = np.indices(shape)
                    src = np.broadcast_to((((yy // 3 + xx // 2) & 1) * 255).astype(np.uint8).reshape(shape + ((1,) if kind == "rgba_u8" else ())), full).copy()
                else:
                    src = np.zeros(full, np.uint8)
                    src[shape[0] // 2:, ...] = 255
                    src[:, shape[1] // 3:, ...] ^= 255
                out = dev(src).sobel()
                torch.cuda.synchronize()
                assert_bits_equal(out.to_numpy(), oracle.sobel(src), f"sobel stream {kind} {shape} {what}")
    parent = rng.integers(0, 256, (90, 400, 4), dtype=np.uint8)
    out = torch.full((90, 400), 9, dtype=torch.uint8, device="cuda")
    zg.Image(torch.from_numpy(parent).cuda()).view((8, 5, 264, 65)).sobel(out=zg.Image(out).view((16, 7, 272, 67)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert_bits_equal(got[7:67, 16:272], oracle.sobel(np.ascontiguousarray(parent[5:65, 8:264])), "sobel stream view")
    got[7:67, 16:272] = 9
    assert (got == 9).all()
    frames = rng.integers(0, 256, (5, 48, 128, 4), dtype=np.uint8)
    got = zg.Pipeline([zg.Step.edges_sobel()]).run(torch.from_numpy(frames).cuda()).cpu().numpy()
    for f in range(5):
        assert np.array_equal(got[f][..., 0], oracle.sobel(frames[f])) and (got[f][..., 3] == 255).all()


@pytest.mark.gpu
def test_sobel_4k(oracle):
    src = oracle.synth_u8(81, (2048, 4096, 4))
    out = dev(src).sobel()
    torch.cuda.synchronize()
    assert_bits_equal(out.to_numpy(), oracle.sobel(src), "sobel 2048x4096 rgba")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u8", "rgba_u8", "f32", "rgb_u8"))
def test_pyramid_parity(oracle, kind):
    src = synth(oracle, kind, 82, 480, 640)
    for n, sf, sigma in ((5, 1.5, 1.0), (8, 1.2, 1.6), (10, 2.0, 1.0)):
        want = oracle.pyramid(src, n, sf, sigma)
        pyr = zg.ImagePyramid.build(dev(src), n, sf, sigma)
        torch.cuda.synchronize()
        assert pyr.n_levels == len(want)
        for i, (g, w) in enumerate(zip(pyr.levels, want)):
            assert_bits_equal(g.to_numpy(), w, f"pyramid {kind} ({n},{sf},{sigma}) level {i}")
    assert zg.ImagePyramid.build(dev(np.zeros((32, 32), np.uint8)), 10, 2.0, 1.0).n_levels < 10  # pyramid.zig:236-252


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((33, 256), (31, 272), (32, 256), (64, 1040), (95, 1024), (500, 2064), (1080, 1920), (20, 640)))
def test_pyramid_u8_fused_levels(oracle, shape):
    """Image(u8) levels come from the tile kernel, k_pyr_tile (pyramid_tile.hip: blur and bilinear resize of one tile in LDS, every level reduced by
    1.3 to 3.9 whose taps fit, up to 8 jobs). Round 5's route is the fallback for what the tile kernel leaves (ratios below 1.3 or from 3.9, longer
    taps, more jobs, unaligned sources; all levels with ZIGNAL_HIP_NO_PYRAMID_TILE set): try_pyramid_levels_u8 with the multi-job kernels
    k_rows_u8f_multi, then k_cols_bilinear_u8_multi (the column pass evaluated at the resize's taps, 31-row bands). The shapes cover tile and band
    seams, the anchored last band, planes shorter than a band, mirrored right / bottom taps, scale 1 (a blurred copy) and both band-loop forms
    (inside / edge); the scale factors put levels on both routes (1.05 and 1.2 below the tile kernel's ratio, 1.5 to 2.1 inside it)."""
    src = oracle.synth_u8(90 + shape[0], shape)
    for n, sf, sigma in ((4, 1.2, 1.6), (6, 1.5, 1.0), (3, 1.05, 0.8), (3, 2.0, 3.0), (3, 2.1, 2.91), (9, 1.2, 1.6)):
        want = oracle.pyramid(src, n, sf, sigma)
        pyr = zg.ImagePyramid.build(dev(src), n, sf, sigma)
        torch.cuda.synchronize()
        assert pyr.n_levels == len(want)
        for i, (g, w) in enumerate(zip(pyr.levels, want)):
            assert_bits_equal(g.to_numpy(), w, f"pyramid u8 {shape} ({n},{sf},{sigma}) level {i}")


@pytest.mark.gpu
def test_pyramid_u8_fused_levels_full_size_and_views(oracle):
    """The default pyramid (8 levels, 1.2, 1.6) of a 2048 x 4096 Image(u8): levels reduced by 1.3 and more come from the tile kernel (k_pyr_tile),
    the first level (1.2) from round 5's fallback route (k_rows_u8f_multi + k_cols_bilinear_u8_multi). Then two source views: one whose pitch is
    not its width, which the tile kernel takes, and one that starts at an odd column, which it refuses (pyramid_tile.hip: origin & 3) and the
    fallback builds."""
    src = oracle.synth_u8(93, (2048, 4096))
    want = oracle.pyramid(src, 8, 1.2, 1.6)
    pyr = zg.ImagePyramid.build_default(dev(src))
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(pyr.levels, want)):
        assert_bits_equal(g.to_numpy(), w, f"default pyramid of 2048x4096 level {i}")
    # a view whose pitch is not its width (stride 4096, 2048 columns) and one the fused path must refuse (unaligned start): same bits either way
    for view in (src[100:900, 1024:3072], src[5:700, 3:1027]):
        want = oracle.pyramid(np.ascontiguousarray(view), 4, 1.3, 1.2)
        whole = dev(src)
        r0, c0 = (100, 1024) if view.shape[1] == 2048 else (5, 3)
        pyr = zg.ImagePyramid.build(whole.view((c0, r0, c0 + view.shape[1], r0 + view.shape[0])), 4, 1.3, 1.2)
        torch.cuda.synchronize()
        for i, (g, w) in enumerate(zip(pyr.levels, want)):
            assert_bits_equal(g.to_numpy(), w, f"pyramid of a view level {i}")


@pytest.mark.gpu
def test_u8_blur_whose_rounded_taps_sum_to_257_clamps_like_divClampU8(oracle):
    """sigma = 1.6 sqrt(1.2^8 - 1) (ORB's level 4): the taps round to a sum of 257, so a saturated neighbourhood reaches (257 * 65535 + 32768) >> 16 = 257
    and divClampU8 clamps it. The f32 column pass holds those sums with its accumulators started 2^23 lower (conv_sep_bytes2.hip, WIDE)."""
    sigma = 1.6 * float(np.sqrt(1.2 ** 8 - 1))
    img = oracle.synth_u8(97, (200, 1024))
    img[40:120, 100:700] = 255
    img[150:, :] = 255
    want = oracle.gaussian_blur(img, sigma)
    assert want.max() == 255
    got = dev(img).gaussian_blur(sigma)
    torch.cuda.synchronize()
    assert_bits_equal(got.to_numpy(), want, "blur with a tap sum of 257 on saturated pixels")
    rgba = np.repeat(img[:, :256, None], 4, axis=2).copy()
    got = dev(rgba).gaussian_blur(sigma)
    torch.cuda.synchronize()
    assert_bits_equal(got.to_numpy(), oracle.gaussian_blur(rgba, sigma), "rgba, same taps")
    want = oracle.pyramid(img, 3, 2.1, 2.91)  # the fused level kernel with the same taps
    for g, w in zip(zg.ImagePyramid.build(dev(img), 3, 2.1, 2.91).levels, want):
        torch.cuda.synchronize()
        assert_bits_equal(g.to_numpy(), w, "pyramid level with a tap sum of 257")


# ---- Canny (image.zig:1047-1063 -> edges.zig:212-277) ---------------------------------------------------------------
def test_canny_reference_known_answers_oracle(oracle):  # tests/filters.zig:1182-1300
    img = np.zeros((10, 10), np.uint8)
    img[:, 5:] = 255
    edges = oracle.canny(img, 1.0, 50, 100)
    assert edges.shape == img.shape and (edges[:, 4:7] > 0).any()
    assert set(np.unique(edges).tolist()) <= {0, 255}
    rgb = np.zeros((8, 8, 3), np.uint8)
    rgb[:, :4] = (255, 0, 0)
    rgb[:, 4:] = (0, 255, 0)
    assert (oracle.canny(rgb, 1.0, 30, 90)[:, 3:6] > 0).any()
    ramp = (np.arange(5)[:, None] * 10 + np.arange(5)[None, :]).astype(np.uint8)
    oracle.canny(ramp, 0, 50, 100)  # sigma == 0 is valid (no blur)
    for bad in ((-1, 50, 100), (1.0, -1, 100), (1.0, 50, -1), (1.0, 100, 50), (float("nan"), 50, 100), (1.0, float("nan"), 100),
                (1.0, 50, float("nan")), (float("inf"), 50, 100), (1.0, float("inf"), 100), (1.0, 50, float("inf")), (float("-inf"), 50, 100)):
        with pytest.raises(RuntimeError):
            oracle.canny(ramp, *bad)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u8", "f32", "rgb_u8", "rgba_u8", "rgb_f32", "rgba_f32"))
def test_canny_gpu_parity(oracle, kind):
    import torch
    import zignal_amd as zg
    from tests.util import assert_bits_equal, synth

    def blobs(rows, cols, seed):  # smooth structure with long connected edges, so hysteresis has chains to follow across tiles
        rng = np.random.default_rng(seed)
        y, x = np.mgrid[0:rows, 0:cols].astype(np.float32)
        f = np.zeros((rows, cols), np.float32)
        for _ in range(12):
            cy, cx, s = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(8, 60)
            f += rng.uniform(-1, 1) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
        f = (f - f.min()) / (f.max() - f.min() + 1e-9)
        return f

    for (rows, cols, sigma, lo, hi) in ((10, 10, 1.0, 50, 100), (97, 211, 1.4, 10, 30), (300, 517, 0.0, 5, 12), (2, 9, 1.0, 5, 10), (130, 70, 2.5, 2, 6),
                                         (180, 512, 1.4, 10, 30), (70, 260, 0.8, 8, 20)):  # the last two: rows of whole 16-byte chunks — u8 / Rgba(u8) sources give the blur's row pass their grey directly
        base = blobs(rows, cols, rows + cols)
        if kind == "u8":
            img = (base * 255).astype(np.uint8)
        elif kind == "f32":
            img = base
        else:
            noise = synth(oracle, kind, 3, rows, cols)
            ch = noise.shape[2]
            if noise.dtype == np.uint8:
                img = np.clip(base[..., None] * 255 * np.array([1.0, 0.8, 0.6, 1.0])[:ch] + noise * 0.02, 0, 255).astype(np.uint8)
            else:
                img = (base[..., None] * np.array([1.0, 0.8, 0.6, 1.0], np.float32)[:ch] + noise * np.float32(0.02)).astype(np.float32)
        want = oracle.canny(img, sigma, lo, hi)
        got = zg.Image(torch.from_numpy(np.ascontiguousarray(img)).cuda()).canny(sigma, lo, hi)
        torch.cuda.synchronize()
        assert_bits_equal(got.to_numpy(), want, f"canny {kind} {rows}x{cols} sigma={sigma}")
        if rows >= 97:
            assert want.any(), "test image produced no edges"
    host = zg.Image(img).canny(sigma, lo, hi).data
    assert_bits_equal(host, want, "canny host layer")
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img).canny(-1, 5, 10)
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img).canny(1, 10, 5)
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img).canny(float("nan"), 5, 10)
    with pytest.raises(zg.DimensionMismatch):
        zg.Image(img).canny(1, 5, 10, out=zg.Image(np.zeros((3, 3), np.uint8)))


@pytest.mark.gpu
def test_hysteresis_on_narrow_frames_whose_tile_roots_sit_left_of_the_tile(oracle):
    """Found by tests/fuzz_parity.py (canny rgb_f32 511x67): k_cc_emit_tile decides from a pixel's label whether its root is a pixel of the same
    64 x 64 tile; on frames narrower than two tiles a root in the tile to the LEFT, one row further down, has the same offset from the tile's
    corner as a pixel inside it. Noise and blobs on widths 65 .. 127 (and one wide frame), several tile rows, both detectors."""
    import torch
    import zignal_amd as zg
    from tests.util import assert_bits_equal
    rng = np.random.default_rng(4004)
    for rows, cols in ((511, 67), (200, 100), (130, 65), (257, 127), (300, 96), (140, 700)):
        noise = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        yy, xx = np.mgrid[0:rows, 0:cols]
        blobs = ((np.sin(yy / 9.0) + np.cos(xx / 7.0) + np.sin((xx + yy) / 13.0)) * 40 + 128 + noise * 0.1).clip(0, 255).astype(np.uint8)
        for name, img in (("noise", noise), ("blobs", blobs)):
            d = zg.Image(torch.from_numpy(img).cuda())
            for sg, lo, hi in ((1.4, 27.8, 95.5), (0.0, 20.0, 60.0), (1.0, 5.0, 12.0)):
                assert_bits_equal(d.canny(sg, lo, hi).to_numpy(), oracle.canny(img, sg, lo, hi), f"canny {name} {rows}x{cols} {sg}")
            for kw in (dict(), dict(smooth=0.7, high_ratio=0.8, low_rel=0.3), dict(use_nms=True, high_ratio=0.9), dict(window_size=3), dict(window_size=5, high_ratio=0.9),
                       dict(window_size=15, high_ratio=0.95)):  # windows 3 / 5 / 7: the streamed count; 15: the general one
                assert_bits_equal(d.shen_castan(**kw).to_numpy(), oracle.shen_castan(img, **kw), f"shen {name} {rows}x{cols} {kw}")


@pytest.mark.gpu
def test_detectors_at_frame_sizes(oracle):
    """Canny and Shen-Castan on whole frames (1080p Rgba(u8), 2048 x 4096 u8): every stage at the sizes its tiling is written for — dozens of ISEF
    segments per chain, thousands of hysteresis tiles with components crossing them, the integral images past 2^24 — against the oracle."""
    import torch
    import zignal_amd as zg
    from tests.util import assert_bits_equal
    for shape, seed in (((1080, 1920, 4), 31), ((2048, 4096), 32)):
        noise = oracle.synth_u8(seed, shape)
        rows, cols = shape[:2]
        yy, xx = np.mgrid[0:rows, 0:cols]
        field = ((np.sin(yy / 37.0) * np.cos(xx / 53.0) + (((xx // 160) + (yy // 120)) % 2)) * 70 + 90).astype(np.float32)
        field = field[..., None] if len(shape) == 3 else field
        img = (field + noise.astype(np.float32) * 0.08).clip(0, 255).astype(np.uint8)  # shapes with hard edges, a little sensor noise
        for name, frame in (("photo-like", img), ("noise", noise)):
            d = zg.Image(torch.from_numpy(np.ascontiguousarray(frame)).cuda())
            assert_bits_equal(d.canny(1.4, 50, 150).to_numpy(), oracle.canny(frame, 1.4, 50, 150), f"canny {name} {shape}")
            assert_bits_equal(d.shen_castan().to_numpy(), oracle.shen_castan(frame), f"shenCastan {name} {shape}")
        assert_bits_equal(zg.Image(torch.from_numpy(img).cuda()).shen_castan(smooth=0.7, use_nms=True).to_numpy(), oracle.shen_castan(img, smooth=0.7, use_nms=True), f"shenCastan nms {shape}")
    # 4096^2 = 2^24 pixels exactly: the largest frame on which the mask's window count is taken directly (every value of its f32 integral image is
    # still an exact integer), and BASELINE's frame size
    big = oracle.synth_u8(33, (4096, 4096))
    assert_bits_equal(zg.Image(torch.from_numpy(big).cuda()).shen_castan().to_numpy(), oracle.shen_castan(big), "shenCastan noise 4096x4096")


@pytest.mark.gpu
def test_canny_long_chain_across_tiles(oracle):
    """A one-pixel spiral whose only strong pixel is at one end: hysteresis must follow it through every tile."""
    import torch
    import zignal_amd as zg
    from tests.util import assert_bits_equal
    n = 256
    img = np.zeros((n, n), np.uint8)
    lo_v, hi_v = 40, 255
    r0, r1, c0, c1 = 4, n - 5, 4, n - 5
    while r1 - r0 > 16:
        img[r0, c0:c1] = lo_v; img[r0:r1, c1] = lo_v; img[r1, c0 + 8:c1 + 1] = lo_v; img[r0 + 8:r1 + 1, c0 + 8] = lo_v
        r0 += 8; c0 += 8; r1 -= 8; c1 -= 8
        img[r0, c0:c0 + 1] = lo_v
    img[4, 4:12] = hi_v
    want = oracle.canny(img, 0.0, 20, 600)
    got = zg.Image(torch.from_numpy(img).cuda()).canny(0.0, 20, 600)
    torch.cuda.synchronize()
    assert_bits_equal(got.to_numpy(), want, "canny spiral")
    assert (want > 0).sum() > 500


@pytest.mark.gpu
def test_edge_detectors_are_graph_capturable(oracle):
    """Neither detector synchronises its stream: both record into one HIP graph, and the replay is still bit-exact."""
    import torch
    import zignal_amd as zg
    from tests.util import assert_bits_equal
    host = synth(oracle, "rgba_u8", 5, 150, 203)
    src = zg.Image(torch.from_numpy(host).cuda())
    out_c = zg.Image(torch.zeros((150, 203), dtype=torch.uint8, device="cuda"))
    out_s = zg.Image(torch.zeros((150, 203), dtype=torch.uint8, device="cuda"))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        src.canny(1.0, 40, 120, out=out_c)  # warm the scratch pool outside the capture
        src.shen_castan(out=out_s)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            src.canny(1.0, 40, 120, out=out_c)
            src.shen_castan(out=out_s)
    out_c.data.zero_(); out_s.data.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert_bits_equal(out_c.to_numpy(), oracle.canny(host, 1.0, 40, 120), "captured canny")
    assert_bits_equal(out_s.to_numpy(), oracle.shen_castan(host), "captured shen-castan")


# ---- motion blur (image.zig:1077-1091 -> motion_blur.zig), SURVEY §8f rank 4 ------------------------------------------
def test_motion_blur_reference_known_answers_oracle(oracle):  # tests/filters.zig:969-1160
    import math
    img = np.zeros((5, 7), np.uint8)
    img[:, 3:] = 255
    b = oracle.motion_blur_linear(img, 0.0, 3)
    assert 0 < b[2, 3] < 255 and abs(int(b[0, 3]) - int(b[4, 3])) < 10
    img = np.zeros((7, 5), np.uint8)
    img[3:, :] = 255
    b = oracle.motion_blur_linear(img, math.pi / 2, 3)
    assert 0 < b[3, 2] < 255 and abs(int(b[3, 0]) - int(b[3, 4])) < 10
    spot = np.zeros((5, 5), np.uint8)
    spot[2, 2] = 255
    b = oracle.motion_blur_linear(spot, math.pi / 4, 3)
    assert b[1, 1] > 0 and b[2, 2] > 0 and b[3, 3] > 0
    pat = np.arange(9, dtype=np.uint8).reshape(3, 3)
    assert (oracle.motion_blur_linear(pat, 0.0, 0) == pat).all()
    assert (oracle.motion_blur_radial(pat, 0.5, 0.5, 0.0, False) == pat).all()
    rgb = np.zeros((5, 5, 3), np.uint8)
    rgb[2, 2] = (255, 128, 64)
    b = oracle.motion_blur_linear(rgb, 0.0, 3)
    assert b[2, 2, 0] > b[2, 2, 1] > b[2, 2, 2] and b[2, 1, 0] > 0
    r, c = np.mgrid[0:7, 0:7]
    d = np.sqrt((c - 3.0) ** 2 + (r - 3.0) ** 2)
    ring = np.where((d > 1.5) & (d < 2.5), 255, 0).astype(np.uint8)
    z = oracle.motion_blur_radial(ring, 0.5, 0.5, 0.5, False)
    assert abs(int(ring[3, 3]) - int(z[3, 3])) < 20
    pt = np.zeros((7, 7), np.uint8)
    pt[2, 4] = 255
    sp = oracle.motion_blur_radial(pt, 0.5, 0.5, 0.5, True)
    assert sp[2, 4] > 0 and (sp > 0).sum() > 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ALL_TYPES)
def test_motion_blur_gpu_parity(oracle, kind):
    import math
    import torch

    def dev(a):
        return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())

    img = synth(oracle, kind, 21, 61, 93)
    for angle, distance in ((0.0, 3), (0.0, 10), (math.pi / 2, 7), (math.pi / 4, 3), (0.3, 8), (2.0, 30), (-1.1, 5), (0.7, 1), (0.0, 0), (0.0005, 4)):
        want = oracle.motion_blur_linear(img, angle, distance)
        got = dev(img).motion_blur_linear(angle, distance)
        torch.cuda.synchronize()
        assert_bits_equal(got.to_numpy(), want, f"linear {kind} angle={angle} d={distance}")
    for cx, cy, strength, spin in ((0.5, 0.5, 0.5, False), (0.5, 0.5, 0.5, True), (0.2, 0.9, 1.0, False), (0.2, 0.9, 0.3, True), (0.0, 0.0, 0.7, False),
                                   (0.0, 0.0, 0.7, True), (1.3, -0.2, 2.5, False), (0.5, 0.5, 0.0, True), (0.4, 0.6, -0.5, False)):
        want = oracle.motion_blur_radial(img, cx, cy, strength, spin)
        got = dev(img).motion_blur_radial(cx, cy, strength, spin)
        torch.cuda.synchronize()
        assert_bits_equal(got.to_numpy(), want, f"radial {kind} c=({cx},{cy}) s={strength} spin={spin}")
    host = zg.Image(img).motion_blur_linear(0.3, 8).data
    assert_bits_equal(host, oracle.motion_blur_linear(img, 0.3, 8), "motion blur host layer")
    with pytest.raises(zg.DimensionMismatch):
        zg.Image(img).motion_blur_linear(0.3, 8, out=zg.Image(np.zeros((3, 3) + img.shape[2:], img.dtype)))


# ---- Shen-Castan (image.zig:1015-1027 -> edges.zig:83-196) --------------------------------------------------------------
def _sc_square():
    img = np.tile((np.arange(50) * 2).astype(np.uint8), (50, 1))
    img[15:35, 15:35] = 200
    return img


@pytest.mark.gpu
def test_isef_segments_equal_the_sequential_recursions(oracle):
    """isefFilter2D (edges.zig:283-349) is two dependent recursions per row and per column; the device cuts them into overlapping segments
    (k_isef_spec) and proves every segment's start against its predecessor (the repair launch). The smoothed plane itself, bit for bit, for
    noise, a ramp, constants and signed values, for smoothing factors on both sides of the point where the warm-up outgrows a window (then the
    sequential kernel runs), for shapes with partial windows, partial chain groups and rows the 16-byte loads exclude."""
    rng = np.random.default_rng(77)
    for rows, cols in ((1, 4), (3, 8), (64, 64), (65, 132), (130, 516), (257, 1028), (700, 900), (1080, 1920), (33, 30), (200, 131)):
        planes = {
            "noise": rng.integers(0, 256, (rows, cols)).astype(np.float32),
            "signed": ((rng.random((rows, cols), dtype=np.float32) - 0.5) * 1e3).astype(np.float32),
            "ramp": (np.arange(rows * cols, dtype=np.float32).reshape(rows, cols) % 251),
            "zeros": np.zeros((rows, cols), np.float32),
        }
        for what, plane in planes.items():
            for smooth in (0.9, 0.7, 0.97, 0.3):
                got = zg.Image(torch.from_numpy(plane).cuda()).isef_smooth(smooth).to_numpy()
                assert_bits_equal(got, oracle.isef_plane(plane, smooth), f"isef {what} {rows}x{cols} smooth {smooth}")
        # the detector's own form: the grey as bytes, converted as the row pass loads it
        grey = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        for smooth in (0.9, 0.6, 0.2):
            got = zg.Image(torch.from_numpy(grey).cuda()).isef_smooth(smooth).to_numpy()
            assert_bits_equal(got, oracle.isef_plane(grey.astype(np.float32), smooth), f"isef bytes {rows}x{cols} smooth {smooth}")


@pytest.mark.gpu
def test_isef_smooth_into_a_destination_that_is_not_16_byte_aligned(oracle):
    """A u8 source whose f32 destination starts 4 bytes into an allocation: the segmented kernels want 16-byte aligned planes, so the call
    takes the transposing route — which reads the grey as f32, and that plane has to be made first (it was a null pointer)."""
    rng = np.random.default_rng(78)
    for rows, cols in ((64, 64), (130, 516), (33, 32)):
        grey = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        buf = torch.zeros(rows * cols + 4, dtype=torch.float32, device="cuda")
        out = zg.Image(buf[1:1 + rows * cols].view(rows, cols))
        assert out.data.data_ptr() % 16 == 4
        zg.Image(torch.from_numpy(grey).cuda()).isef_smooth(0.9, out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.to_numpy(), oracle.isef_plane(grey.astype(np.float32), 0.9), f"isef bytes -> unaligned f32 {rows}x{cols}")
        f32 = rng.random((rows, cols), dtype=np.float32)
        zg.Image(torch.from_numpy(f32).cuda()).isef_smooth(0.7, out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.to_numpy(), oracle.isef_plane(f32, 0.7), f"isef f32 -> unaligned f32 {rows}x{cols}")


@pytest.mark.gpu
@pytest.mark.parametrize("w", (8, 12, 16))
def test_isef_repair_launch_when_only_some_groups_start_wrong(oracle, w):
    """ZIGNAL_HIP_ISEF_W forces a warm-up shorter than the contraction needs: with W = 4 every segment fails its check; with 8 - 16 steps and
    a mild smoothing factor only SOME 64-chain groups do (a rough region beside flat ones), so the repair launch redoes a subset — rows
    and, in place on the column pass, columns — and the rest keeps the segmented result. A child process: the hook is read once."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
import zignal_amd as zg
from oracle import pyoracle as o
o.lib()
rng = np.random.default_rng(5)
for rows, cols in ((256, 1024), (300, 772)):
    plane = np.full((rows, cols), 100.0, np.float32)
    plane[64:128, 200:600] = rng.integers(0, 256, (64, 400)).astype(np.float32) * 1e3   # rough block: its neighbours' short warm-ups cannot settle
    plane[200:, cols - 100:] = rng.random((rows - 200, 100), dtype=np.float32)
    for smooth in (0.4, 0.6):
        got = zg.Image(torch.from_numpy(plane).cuda()).isef_smooth(smooth).to_numpy()
        want = o.isef_plane(plane, smooth)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rows, cols, smooth)
print("ok")
''' % root
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZIGNAL_HIP_ISEF_W=str(w)))
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-300:], out.stderr[-1200:])


def test_shen_castan_reference_known_answers_oracle(oracle):  # tests/shen_castan.zig:10-130, 60-86
    e = oracle.shen_castan(_sc_square(), 0.8, 7, 0.9, 0.3)
    assert 0 < (e > 0).sum() < 500 and set(np.unique(e).tolist()) <= {0, 255}
    img = np.zeros((50, 50), np.uint8)
    for c in range(25):
        img[:, c] = min(c * 10, 200)
    img[:, 25:] = 240
    e = oracle.shen_castan(img, 0.85, 7, 0.8, 0.3)
    assert (e[10:40, 24:27] > 0).any()
    r, c = np.mgrid[0:40, 0:40]
    circ = np.where(np.sqrt((r - 20.0) ** 2 + (c - 20.0) ** 2) <= 10, 200, 50 + (r + c) // 2).astype(np.uint8)
    assert (oracle.shen_castan(circ, 0.7, 7, 0.9) > 0).any() and (oracle.shen_castan(circ, 0.9, 7, 0.9) > 0).any()
    for bad in (dict(smooth=0.0), dict(smooth=1.0), dict(smooth=-0.5), dict(high_ratio=0.0), dict(high_ratio=1.0), dict(low_rel=0.0),
                dict(window_size=6), dict(window_size=1)):
        with pytest.raises(RuntimeError):
            oracle.shen_castan(img, **bad)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u8", "f32", "rgb_u8", "rgba_u8", "rgba_f32"))
def test_shen_castan_gpu_parity(oracle, kind):
    import torch

    def frame(rows, cols, seed):
        rng = np.random.default_rng(seed)
        y, x = np.mgrid[0:rows, 0:cols].astype(np.float32)
        f = np.zeros((rows, cols), np.float32)
        for _ in range(10):
            cy, cx, s = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(4, 40)
            f += rng.uniform(-1, 1) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
        f += (x > cols * 0.6) * 0.4
        f = (f - f.min()) / (f.max() - f.min() + 1e-9)
        if kind == "u8":
            return (f * 255).astype(np.uint8)
        if kind == "f32":
            return f.astype(np.float32)
        ch = 3 if kind.startswith("rgb_") else 4
        w = np.array([1.0, 0.7, 0.4, 1.0], np.float32)[:ch]
        if kind.endswith("u8"):
            return (f[..., None] * 255 * w).astype(np.uint8)
        return (f[..., None] * w).astype(np.float32)

    cases = [((50, 50), dict(smooth=0.8, window_size=7, high_ratio=0.9, low_rel=0.3)),
             ((97, 211), dict()),
             ((97, 211), dict(use_nms=True, high_ratio=0.9)),
             ((130, 70), dict(hysteresis=False, high_ratio=0.8, window_size=3)),
             ((300, 517), dict(smooth=0.7, window_size=11, high_ratio=0.95, low_rel=0.2, use_nms=True)),
             ((2, 9), dict(high_ratio=0.5)), ((2, 9), dict(high_ratio=0.5, use_nms=True)), ((1, 1), dict())]
    for (rows, cols), opts in cases:
        img = _sc_square() if (rows, cols) == (50, 50) and kind == "u8" else frame(rows, cols, rows * 7 + cols)
        want = oracle.shen_castan(img, **opts)
        got = zg.Image(torch.from_numpy(np.ascontiguousarray(img)).cuda()).shen_castan(**opts)
        torch.cuda.synchronize()
        assert_bits_equal(got.to_numpy(), want, f"shenCastan {kind} {rows}x{cols} {opts}")
    assert_bits_equal(zg.Image(img).shen_castan().data, oracle.shen_castan(img), "shenCastan host layer")
    for bad in (dict(smooth=0.0), dict(smooth=1.0), dict(high_ratio=1.0), dict(low_rel=0.0), dict(window_size=6), dict(window_size=1)):
        with pytest.raises(zg.InvalidArgument):
            zg.Image(img).shen_castan(**bad)


# ---- binary.zig: Otsu / adaptive-mean thresholds, binary morphology (image.zig:845-914) ---------------------------------
def test_binary_reference_known_answers_oracle(oracle):  # tests/binary.zig:7-175
    out, t = oracle.threshold_otsu(np.array([[10, 10, 10, 10], [200, 200, 200, 200]], np.uint8))
    assert 5 <= t <= 50 and out.tolist() == [[0] * 4, [255] * 4]
    img = np.array([[50, 50, 50], [50, 200, 50], [50, 50, 50]], np.uint8)
    assert oracle.threshold_adaptive_mean(img, 1, 10.0).tolist() == [[0, 0, 0], [0, 255, 0], [0, 0, 0]]
    with pytest.raises(RuntimeError):
        oracle.threshold_adaptive_mean(img, 0, 0.0)  # error.InvalidRadius
    box = np.ones((3, 3), np.uint8)
    block = np.zeros((5, 5), np.uint8)
    block[1:4, 1:4] = 255
    dot = np.zeros((5, 5), np.uint8)
    dot[2, 2] = 255
    assert (oracle.morph(dot, box, 1, oracle.MORPH_DILATE) == block).all()
    noisy = block.copy()
    noisy[1, 4] = 255
    assert (oracle.morph(noisy, box, 1, oracle.MORPH_OPEN) == block).all()
    holed = block.copy()
    holed[2, 2] = 0
    assert (oracle.morph(holed, box, 1, oracle.MORPH_CLOSE) == block).all()
    big = np.zeros((7, 7), np.uint8)
    big[1:6, 1:6] = 255
    e1, e2 = oracle.morph(big, box, 1, oracle.MORPH_ERODE), oracle.morph(big, box, 2, oracle.MORPH_ERODE)
    assert e1[2:5, 2:5].all() and e1.sum() == 9 * 255 and e2.sum() == 255 and e2[3, 3] == 255
    with pytest.raises(RuntimeError):
        oracle.morph(big, np.ones((2, 3), np.uint8), 1, oracle.MORPH_DILATE)  # error.InvalidKernelSize


@pytest.mark.gpu
def test_binary_gpu_parity(oracle):
    import torch

    def dev(a):
        return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())

    rng = np.random.default_rng(70)
    for (rows, cols) in ((2, 4), (37, 53), (130, 517), (64, 64)):
        img = synth(oracle, "u8", 71 + rows, rows, cols)
        if rows > 30:  # a bimodal frame so that Otsu has something to find
            img = np.where(synth(oracle, "u8", 5, rows, cols) > 128, 180 + img // 4, img // 3).astype(np.uint8)
        want, wt = oracle.threshold_otsu(img)
        got, gt = dev(img).threshold_otsu()
        torch.cuda.synchronize()
        assert gt == wt
        assert_bits_equal(got.to_numpy(), want, f"otsu {rows}x{cols}")
        for radius, c in ((1, 10.0), (3, -2.5), (50, 0.0)):
            got = dev(img).threshold_adaptive_mean(radius, c)
            torch.cuda.synchronize()
            assert_bits_equal(got.to_numpy(), oracle.threshold_adaptive_mean(img, radius, c), f"adaptive {rows}x{cols} r={radius}")
        mask = (img > 150).astype(np.uint8) * 255
        for kshape in ((3, 3), (1, 5), (7, 3), (15, 15)):
            k = (rng.random(kshape) > 0.3).astype(np.uint8)
            k[kshape[0] // 2, kshape[1] // 2] = 1
            for op in range(4):
                for it in (0, 1, 2, 3):
                    got = dev(mask)._morph(k, it, op, None)
                    torch.cuda.synchronize()
                    assert_bits_equal(got.to_numpy(), oracle.morph(mask, k, it, op), f"morph op={op} it={it} k={kshape} {rows}x{cols}")
        # in place (the reference's tests call openBinary(image, ...) onto itself)
        d = dev(mask)
        d.open_binary(np.ones((3, 3), np.uint8), 1, out=d)
        torch.cuda.synchronize()
        assert_bits_equal(d.to_numpy(), oracle.morph(mask, np.ones((3, 3), np.uint8), 1, oracle.MORPH_OPEN), "open in place")
        d = dev(mask)
        d.erode_binary(np.ones((3, 3), np.uint8), 1, out=d)
        torch.cuda.synchronize()
        assert_bits_equal(d.to_numpy(), oracle.morph(mask, np.ones((3, 3), np.uint8), 1, oracle.MORPH_ERODE), "erode in place")
    host, ht = zg.Image(img).threshold_otsu()
    assert ht == wt and (host.data == want).all()
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img).threshold_adaptive_mean(0, 0.0)
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img).dilate_binary(np.ones((2, 3), np.uint8))
    with pytest.raises(zg.ZignalError):
        zg.Image(np.zeros((4, 4, 3), np.uint8)).threshold_otsu()


# ---- enhancement.zig: autocontrast / equalize (image.zig:804-829) ------------------------------------------------------
def test_enhancement_oracle_hand_checked(oracle):
    """No known answers in the reference for these two; the expected values below are worked by hand from
    enhancement.zig:11-80 / :84-131 and histogram.zig:123-162."""
    assert oracle.autocontrast(np.array([[50, 100], [150, 200]], np.uint8)).tolist() == [[0, 85], [170, 255]]
    assert oracle.equalize(np.array([[10, 10], [20, 30]], np.uint8)).tolist() == [[0, 0], [127, 255]]  # cdf 2,3,4; (cdf-2)*255/2
    flat = np.full((3, 3), 77, np.uint8)
    assert (oracle.equalize(flat.copy()) == 77).all()  # denominator 0: identity table
    assert (oracle.autocontrast(flat.copy()) == 0).all()  # min == max: range 1, clamped - min == 0
    rgba = np.array([[[10, 20, 30, 40], [110, 220, 130, 140]]], np.uint8)
    assert oracle.autocontrast(rgba.copy())[..., 3].tolist() == [[40, 140]]  # alpha untouched
    with pytest.raises(RuntimeError):
        oracle.autocontrast(flat.copy(), 0.5)  # error.InvalidCutoff


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u8", "rgb_u8", "rgba_u8"))
def test_enhancement_gpu_parity(oracle, kind):
    import torch
    for (rows, cols) in ((1, 1), (5, 7), (130, 517), (64, 256)):
        img = synth(oracle, kind, 81 + rows, rows, cols)
        img = (img.astype(np.float32) * 0.6 + 30).astype(np.uint8)  # leave both tails empty so the cut-offs matter
        for cutoff in (0.0, 0.02, 0.3, 0.49):
            got = zg.Image(torch.from_numpy(img.copy()).cuda()).autocontrast(cutoff)
            torch.cuda.synchronize()
            assert_bits_equal(got.to_numpy(), oracle.autocontrast(img.copy(), cutoff), f"autocontrast {kind} {rows}x{cols} cutoff={cutoff}")
        got = zg.Image(torch.from_numpy(img.copy()).cuda()).equalize()
        torch.cuda.synchronize()
        assert_bits_equal(got.to_numpy(), oracle.equalize(img.copy()), f"equalize {kind} {rows}x{cols}")
    assert_bits_equal(zg.Image(img.copy()).equalize().data, oracle.equalize(img.copy()), "equalize host layer")
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img.copy()).autocontrast(0.5)
    with pytest.raises(zg.ZignalError):
        zg.Image(np.zeros((4, 4), np.float32)).equalize()


# ---- order_statistic_blur.zig: median / percentile / min / max / midpoint / alpha-trimmed mean (image.zig:653-783) ------
def test_order_statistic_reference_known_answers_oracle(oracle):  # tests/filters.zig:817-960
    z = np.zeros((5, 5), np.uint8)
    z[2, 2] = 255
    m = oracle.order_statistic_blur(z, 1, oracle.OS_PERCENTILE, 0.5, oracle.MIRROR)
    assert m[2, 2] == 0 and m[2, 1] == 0 and m[1, 2] == 0
    a = np.arange(9, dtype=np.uint8).reshape(3, 3)
    mx = oracle.order_statistic_blur(a, 1, oracle.OS_PERCENTILE, 1.0, oracle.ZERO)
    assert mx[1, 1] == 8 and mx[0, 0] == 4
    rgb = np.tile(np.array([32, 64, 96], np.uint8), (3, 3, 1))
    rgb[1, 1] = (255, 0, 0)
    med = oracle.order_statistic_blur(rgb, 1, oracle.OS_PERCENTILE, 0.5, oracle.MIRROR)
    assert med[1, 1].tolist() == [32, 64, 96] and med[0, 0].tolist() == [32, 64, 96]
    assert oracle.order_statistic_blur(a, 1, oracle.OS_MIDPOINT, 0, oracle.REPLICATE)[1, 1] == 4
    assert oracle.order_statistic_blur(a, 1, oracle.OS_ALPHA_TRIMMED, 0.12, oracle.REPLICATE)[1, 1] == 4
    for bad in ((oracle.OS_ALPHA_TRIMMED, 0.5), (oracle.OS_ALPHA_TRIMMED, -0.1), (oracle.OS_PERCENTILE, 1.5)):
        with pytest.raises(RuntimeError):
            oracle.order_statistic_blur(a, 1, bad[0], bad[1], oracle.REPLICATE)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u8", "rgb_u8", "rgba_u8"))
def test_order_statistic_gpu_parity(oracle, kind):
    import torch

    def dev(a):
        return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())

    for (rows, cols) in ((1, 1), (3, 3), (37, 53), (20, 140)):
        img = synth(oracle, kind, 91 + rows, rows, cols)
        for border in (0, 1, 2, 3):
            for radius in (0, 1, 2, 4):
                for op, param in ((0, 0.5), (0, 0.0), (0, 1.0), (0, 0.37), (1, 0.0), (2, 0.12), (2, 0.0), (2, 0.49)):
                    if radius == 4 and (border in (0, 3)) and op == 0 and param == 0.37:
                        continue
                    want = oracle.order_statistic_blur(img, radius, op, param, border)
                    got = dev(img)._order_stat(radius, op, param, border, None)
                    torch.cuda.synchronize()
                    assert_bits_equal(got.to_numpy(), want, f"order-stat {kind} {rows}x{cols} r={radius} op={op} p={param} border={border}")
    d = dev(img)
    d.median_blur(1, out=d)  # in place
    torch.cuda.synchronize()
    assert_bits_equal(d.to_numpy(), oracle.order_statistic_blur(img, 1, 0, 0.5, oracle.MIRROR), "median in place")
    assert_bits_equal(zg.Image(img).median_blur(2).data, oracle.order_statistic_blur(img, 2, 0, 0.5, oracle.MIRROR), "median host layer")
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img).percentile_blur(1, 1.5)
    with pytest.raises(zg.InvalidArgument):
        zg.Image(img).alpha_trimmed_mean_blur(1, 0.5)
    with pytest.raises(zg.ZignalError):
        zg.Image(np.zeros((4, 4), np.float32)).median_blur(1)

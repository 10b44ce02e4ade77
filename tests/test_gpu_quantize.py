"""The quantisation module on the device against tests/quantize_ref.py, byte for byte: the colour histogram with its first-pixel
indices, median cut, the lookup table, the three dither modes on shapes on both sides of every constant of the error-diffusion kernel
(zg_dither_geometry), views, a batch, mapImageToPalette, and the whole chain captured into a graph and replayed on changed inputs."""
import functools

import numpy as np
import pytest

import zignal_amd as zg
from tests import quantize_ref as R
from zignal_amd import quantize as Q

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

BAND, PHASE, ROWS_PER_LAUNCH = zg.dither_geometry()  # host constants of the library: no GPU needed to read them
TWO_GREYS = np.array([[64, 64, 64], [192, 192, 192]], np.uint8)
MODES = {"floyd_steinberg": R.FLOYD_STEINBERG, "atkinson": R.ATKINSON, "ordered": R.ORDERED}


def noise(seed, rows, cols, ch=3):
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def random_palette(n, seed=0):
    return np.random.default_rng(1000 + n + seed).integers(0, 256, (n, 3), dtype=np.uint8)


PALETTES = {
    "two greys": TWO_GREYS,
    "1 entry": random_palette(1), "15 entries": random_palette(15), "16 entries": random_palette(16), "17 entries": random_palette(17),
    "256 entries": random_palette(256),
    "duplicates": np.array([[30, 60, 90], [200, 180, 40], [30, 60, 90], [200, 180, 40], [128, 128, 128]], np.uint8),  # ties go to the lowest index
    "6x7x6": R.fixed_palette(R.FIXED_6X7X6),
}

# (rows, cols) on both sides of the band height, the phase width and the rows of one launch; Atkinson's c + 2 and r + 2 edges
SHAPES = ([(r, c) for r in (1, 2, 3) for c in (1, 2, 3)]
          + [(BAND - 1, 9), (BAND, 9), (BAND + 1, 9), (2 * BAND, 9), (2 * BAND + 1, 70)]
          + [(5, PHASE - 1), (5, PHASE), (5, PHASE + 1), (5, 2 * PHASE), (BAND + 3, 2 * PHASE + 1)]
          + [(ROWS_PER_LAUNCH + 1, 5)])


@functools.lru_cache(maxsize=None)
def lut_of(name):
    lut = R.palette_lut(PALETTES[name])
    lut.setflags(write=False)
    return lut


@functools.lru_cache(maxsize=None)
def want(rows, cols, seed, palette, mode):
    """The restatement's frame: computed once, shared, never written."""
    out = R.dither(noise(seed, rows, cols), PALETTES[palette], lut_of(palette), mode)
    out.setflags(write=False)
    return out


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_dither(host, palette, mode):
    dev = on_device(host)
    img = zg.Image(dev)
    assert img.dither(PALETTES[palette], on_device(lut_of(palette)), mode) is img
    return dev.cpu().numpy()


# ---- dither --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_dither_equals_the_reference_on_every_shape(shape, mode):
    rows, cols = shape
    got = device_dither(noise(7, rows, cols), "two greys", MODES[mode])
    assert got.tobytes() == want(rows, cols, 7, "two greys", MODES[mode]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("palette", list(PALETTES))
def test_dither_equals_the_reference_on_every_palette(palette, mode):
    rows, cols = BAND + 7, PHASE + 13
    got = device_dither(noise(8, rows, cols), palette, MODES[mode])
    assert got.tobytes() == want(rows, cols, 8, palette, MODES[mode]).tobytes()


@pytest.mark.gpu
def test_dither_builds_the_table_itself_and_none_and_auto_do_nothing():
    host = noise(9, 20, 30)
    dev = on_device(host)
    zg.Image(dev).dither(TWO_GREYS)  # Floyd-Steinberg, the table built by the call
    assert dev.cpu().numpy().tobytes() == R.dither(host, TWO_GREYS, lut_of("two greys"), R.FLOYD_STEINBERG).tobytes()
    for mode in (zg.DitherMode.none, zg.DitherMode.auto):
        dev = on_device(host)
        zg.Image(dev).dither(TWO_GREYS, mode=mode)
        assert dev.cpu().numpy().tobytes() == host.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_dither_of_a_view_leaves_the_bytes_outside_alone(mode):
    rows, cols = BAND + 2, 45
    base = noise(10, rows + 3, cols + 11)
    dev = on_device(base)
    zg.Image(dev).view((4, 2, 4 + cols, 2 + rows)).dither(TWO_GREYS, on_device(lut_of("two greys")), MODES[mode])
    expect = base.copy()
    expect[2:2 + rows, 4:4 + cols] = R.dither(np.ascontiguousarray(base[2:2 + rows, 4:4 + cols]), TWO_GREYS, lut_of("two greys"), MODES[mode])
    assert dev.cpu().numpy().tobytes() == expect.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_a_batch_of_frames_equals_single_calls(mode):
    rows, cols = BAND + 5, 33
    frames = np.stack([noise(20 + i, rows, cols) for i in range(3)])
    lut = on_device(lut_of("two greys"))
    batch = on_device(frames)
    Q.dither(zg.Image(batch[0]), TWO_GREYS, lut, MODES[mode], n_frames=3, frame_bytes=rows * cols * 3)
    for i in range(3):
        single = on_device(frames[i])
        zg.Image(single).dither(TWO_GREYS, lut, MODES[mode])
        assert batch[i].cpu().numpy().tobytes() == single.cpu().numpy().tobytes()
        assert single.cpu().numpy().tobytes() == R.dither(frames[i], TWO_GREYS, lut_of("two greys"), MODES[mode]).tobytes()


# ---- lookup table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("palette", list(PALETTES))
def test_lookup_table_equals_the_reference(palette):
    got = zg.palette_lut(on_device(PALETTES[palette])).cpu().numpy()
    assert got.shape == (R.CELLS,) and got.tobytes() == lut_of(palette).tobytes()


# ---- histogram -----------------------------------------------------------------------------------------------------------------------
def every_cell_once():
    """256 x 128 Rgb pixels, cell k at raster index k."""
    k = np.arange(R.CELLS, dtype=np.uint32).reshape(256, 128)
    return np.stack([(k >> 10) << 3, ((k >> 5) & 31) << 3, (k & 31) << 3], axis=2).astype(np.uint8)


def check_histogram(host, img):
    counts, first = img.color_histogram()
    want_counts, want_first = R.histogram(host)
    assert counts.cpu().numpy().view(np.uint32).tobytes() == want_counts.tobytes()
    assert first.cpu().numpy().view(np.uint32).tobytes() == want_first.tobytes()
    return want_first


@pytest.mark.gpu
def test_histogram_of_one_and_two_colours():
    one = np.full((9, 13, 3), 200, np.uint8)
    check_histogram(one, zg.Image(on_device(one)))
    two = TWO_GREYS[np.random.default_rng(3).integers(0, 2, (31, 17))]
    check_histogram(two, zg.Image(on_device(two)))


@pytest.mark.gpu
def test_histogram_first_follows_the_raster_order():
    cells = every_cell_once()
    first = check_histogram(cells, zg.Image(on_device(cells)))
    assert np.array_equal(first, np.arange(R.CELLS, dtype=np.uint32))
    flipped = np.ascontiguousarray(cells[::-1, ::-1])  # the same cells in reversed raster order
    first_flipped = check_histogram(flipped, zg.Image(on_device(flipped)))
    assert np.array_equal(first_flipped, np.arange(R.CELLS, dtype=np.uint32)[::-1])


@pytest.mark.gpu
def test_histogram_of_a_flat_frame():
    flat = np.full((512, 512, 3), 77, np.uint8)  # every pixel on one counter
    check_histogram(flat, zg.Image(on_device(flat)))


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3, 4], ids=["u8", "rgb_u8", "rgba_u8"])
def test_histogram_of_every_pixel_type_and_of_a_view(ch):
    host = noise(30 + ch, 150, 131, ch)
    check_histogram(host, zg.Image(on_device(host)))
    view = host[5:140, 7:100]
    check_histogram(np.ascontiguousarray(view), zg.Image(on_device(host)).view((7, 5, 100, 140)))


# ---- median cut ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_colors", [2, 16, 256])
def test_median_cut_equals_the_reference_on_noise(max_colors):
    host = noise(40, 64, 64)
    got = zg.Image(on_device(host)).median_cut(max_colors)
    assert got.tobytes() == R.median_cut(host, max_colors).tobytes() and len(got) == max_colors


@pytest.mark.gpu
def test_median_cut_with_fewer_colours_than_max_colors_and_build_palette():
    few = R.fixed_palette(R.FIXED_VGA16)[np.random.default_rng(5).integers(0, 16, (40, 50))]
    img = zg.Image(on_device(few))
    got = img.median_cut(256)
    assert got.tobytes() == R.median_cut(few, 256).tobytes() and len(got) <= 16
    assert zg.build_palette(zg.PaletteMode.adaptive, img, 8).tobytes() == R.median_cut(few, 8).tobytes()
    grey = noise(41, 33, 47, 1)
    assert zg.Image(on_device(grey)).median_cut(32).tobytes() == R.median_cut(grey, 32).tobytes()


# ---- map to palette ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("use_dither", [False, True], ids=["plain", "dither"])
@pytest.mark.parametrize("ch", [1, 3, 4], ids=["u8", "rgb_u8", "rgba_u8"])
def test_map_to_palette_equals_the_reference(ch, use_dither):
    host = noise(50 + ch, BAND + 9, 77, ch)
    palette = PALETTES["17 entries"]
    got = zg.Image(on_device(host)).map_to_palette(palette, use_dither)
    assert got.to_numpy().tobytes() == R.map_to_palette(host, palette, use_dither).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("use_dither", [False, True], ids=["plain", "dither"])
def test_map_to_palette_transparent_index(use_dither):
    host = noise(60, 40, 50, 4)
    host[:, :, 3] = np.where(np.random.default_rng(61).integers(0, 2, (40, 50)) == 0, 127, 128)  # either side of the alpha test
    palette = PALETTES["16 entries"]
    got = zg.Image(on_device(host)).map_to_palette(palette, use_dither, transparent_index=15).to_numpy()
    want_idx = R.map_to_palette(host, palette, use_dither, 15)
    assert got.tobytes() == want_idx.tobytes()
    assert np.all(got[host[:, :, 3] == 127] == 15) and np.all(got[host[:, :, 3] == 128] < 15)  # the last entry is not looked up
    # a source without alpha: the last entry is still left out of the table
    rgb = np.ascontiguousarray(host[:, :, :3])
    got = zg.Image(on_device(rgb)).map_to_palette(palette, use_dither, transparent_index=15).to_numpy()
    assert got.tobytes() == R.map_to_palette(rgb, palette, use_dither, 15).tobytes()


@pytest.mark.gpu
def test_map_to_palette_into_an_index_view():
    host = noise(62, 30, 41)
    palette = PALETTES["15 entries"]
    base = torch.full((36, 50), 0xEE, dtype=torch.uint8, device="cuda")
    out = zg.Image(base).view((3, 2, 3 + 41, 2 + 30))
    assert zg.Image(on_device(host)).map_to_palette(palette, True, out=out) is out
    expect = np.full((36, 50), 0xEE, np.uint8)
    expect[2:32, 3:44] = R.map_to_palette(host, palette, True)
    assert base.cpu().numpy().tobytes() == expect.tobytes()


# ---- the chain under capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_chain_replays_from_a_graph_on_changed_inputs():
    rows, cols = BAND + 6, PHASE + 9
    frame = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
    work = torch.empty_like(frame)
    palette = torch.empty((16, 3), dtype=torch.uint8, device="cuda")
    lut = torch.empty(R.CELLS, dtype=torch.uint8, device="cuda")
    counts = torch.empty(R.CELLS, dtype=torch.int32, device="cuda")
    first = torch.empty(R.CELLS, dtype=torch.int32, device="cuda")
    indices = zg.Image(torch.empty((rows, cols), dtype=torch.uint8, device="cuda"))

    def enqueue():
        zg.Image(frame).color_histogram(counts, first)
        zg.palette_lut(palette, out=lut)
        work.copy_(frame)
        zg.Image(work).dither(palette, lut, zg.DitherMode.atkinson)
        zg.Image(frame).map_to_palette(palette, True, out=indices)

    def load(seed):
        frame.copy_(on_device(noise(seed, rows, cols)))
        palette.copy_(on_device(random_palette(16, seed)))

    def check(seed, what):
        host, pal = noise(seed, rows, cols), random_palette(16, seed)
        want_counts, want_first = R.histogram(host)
        table = R.palette_lut(pal)
        assert counts.cpu().numpy().view(np.uint32).tobytes() == want_counts.tobytes(), what
        assert first.cpu().numpy().view(np.uint32).tobytes() == want_first.tobytes(), what
        assert lut.cpu().numpy().tobytes() == table.tobytes(), what
        assert work.cpu().numpy().tobytes() == R.dither(host, pal, table, R.ATKINSON).tobytes(), what
        assert indices.to_numpy().tobytes() == R.map_to_palette(host, pal, True).tobytes(), what

    side = torch.cuda.Stream()
    load(70)
    with torch.cuda.stream(side):
        enqueue()  # warm-up outside the capture
    side.synchronize()
    check(70, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue()
    for seed in (71, 72):
        load(seed)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(seed, f"replay on frame {seed}")
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0

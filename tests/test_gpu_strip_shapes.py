"""One table of the strip kernels' shape classes through each of the four of them — k_sep_stream, k_conv2d_stream, k_sobel_stream
(the strip walker of zignal_amd/csrc/zg_stream.h) and k_sep_tile_f32 (the same skeleton on f32 tiles) — against the CPU oracle, bit for bit.

A strip is 1024 bytes wide and a lane owns 16 of them, so the row lengths are: 64 pixels (the routes' minimum), 1008 bytes (one lane
short of a strip), 1024, 1056 (a second strip two lanes wide) and 2048 + 512; a pixel type skips a length it cannot make (Rgb rows
are multiples of 48 bytes). Rows: 16 (the minimum, one strip), 17, and 70, which every route cuts into at least three strips, so that
interior strips take the whole-frame (FAST) form of the row loads and stores and the first and last take the per-row (GENERAL) one.
Read from the routes' strip-row policies at these sizes: stream_strip_rows gives 20 rows (4 strips: general, fast, fast, general),
c2s_strip_rows and sobel's policy give 16 (5 strips: general, fast, fast, fast, general), the f32 tile is 8 rows high (9 tiles, the
first and the last general). Every shape satisfies the preconditions of its route's try_* function (takes_strip_route below states
them), so it runs on the stream kernel and not on a fallback."""
import numpy as np
import pytest

import zignal_amd as zg
from tests.util import assert_bits_equal, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BORDERS = (zg.BorderMode.zero, zg.BorderMode.replicate, zg.BorderMode.mirror, zg.BorderMode.wrap)
ROWS = (16, 17, 70)
ROW_BYTES = (None, 1008, 1024, 1056, 2048 + 512)  # None: 64 pixels
PIXEL_BYTES = {"u8": 1, "rgb_u8": 3, "rgba_u8": 4, "f32": 4}

# 5 integer taps per axis, each axis summing to 256, neither symmetric: a swapped axis or a mirrored tap order shows
KX5 = (np.array([16, 64, 100, 52, 24]) / 256.0).astype(np.float32)
KY5 = (np.array([30, 50, 90, 62, 24]) / 256.0).astype(np.float32)
K3X3 = (np.array([[10, -20, 30], [44, 120, -36], [50, 26, 32]]) / 256.0).astype(np.float32)  # 255 * sum |k * 256| < 2^24
KXF = np.array([0.11, -0.23, 0.57, 0.31, 0.19], np.float32)
KYF = np.array([0.07, 0.41, 0.33, -0.12, 0.29], np.float32)


def widths(kind):
    """Pixel counts that give the table's byte lengths for this pixel type."""
    px = PIXEL_BYTES[kind]
    return [64 if rb is None else rb // px for rb in ROW_BYTES if rb is None or rb % px == 0]


def takes_strip_route(op, kind, rows, cols, taps, src_pitch_px=None, dst_pitch_px=None, planes=1, frames=1):
    """The preconditions read from the route's try_* function, for a call whose bases are 16-byte aligned (torch allocations, and
    view origins at multiples of 16 bytes), whose source and destination have the same size, and whose taps are the ones above."""
    px = PIXEL_BYTES[kind]
    src_pitch = (src_pitch_px or cols) * px
    dst_px = 1 if op == "sobel" else px                      # sobel writes one byte per pixel
    dst_pitch = (dst_pitch_px or cols) * dst_px
    rb = cols * px
    # strip_shape_ok: what every strip route asks of the source
    ok = rb % 16 == 0 and src_pitch % 16 == 0 and rb % 1024 != 16 and cols >= 64 and rows >= 16
    ok = ok and rb <= 0x3FFFFFFF and src_pitch <= 0x7FFFFFFF and dst_pitch <= 0x7FFFFFFF
    h = taps // 2
    if op == "separable_u8":    # try_sep_stream: byte pixels, not a lone grey plane, 3..9 equal odd taps in 0..255 summing to <= 257 per axis
        ok = ok and kind in ("u8", "rgb_u8", "rgba_u8") and not (px == 1 and frames == 1) and taps in (3, 5, 7, 9) and (h + 1) * px <= 16
        ok = ok and dst_pitch % 16 == 0
        ok = ok and all(0 <= t <= 255 for k in (KX5, KY5) for t in np.round(k * 256)) and all(np.round(k * 256).sum() <= 257 for k in (KX5, KY5))
    elif op == "convolve_3x3":  # convolve_impl + try_conv2d_stream: square 3 or 5, 255 * sum |round(256 k)| < 2^24, byte pixels
        ok = ok and kind in ("u8", "rgb_u8", "rgba_u8") and taps in (3, 5) and (h + 1) * px <= 16 and dst_pitch % 16 == 0
        ok = ok and 255 * np.abs(np.round(K3X3 * 256)).sum() < 2 ** 24
    elif op == "sobel":         # try_sobel_stream: u8 or Rgba(u8); the destination aligned to the lane's output unit
        ok = ok and kind in ("u8", "rgba_u8") and dst_pitch % (16 if px == 1 else 4) == 0
    else:                       # try_sep_tile_f32: up to 8 equal f32 planes, 3 / 5 / 7 taps, none below the skip threshold
        ok = ok and kind == "f32" and 1 <= planes <= 8 and taps in (3, 5, 7) and dst_pitch % 16 == 0
        ok = ok and all(abs(t) >= 1e-10 for k in (KXF, KYF) for t in k)
    return bool(ok)


def dev(a):
    return zg.Image(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def shapes(op, kind, taps, planes=1):
    for rows in ROWS:
        for cols in widths(kind):
            assert takes_strip_route(op, kind, rows, cols, taps, planes=planes), (op, kind, rows, cols)
            yield rows, cols


@pytest.mark.parametrize("kind", ("rgb_u8", "rgba_u8"))
def test_separable_u8(oracle, kind):
    for rows, cols in shapes("separable_u8", kind, 5):
        img = synth(oracle, kind, 1000 + rows + cols, rows, cols)
        src = dev(img)
        for border in BORDERS:
            got = src.convolve_separable(KX5, KY5, border)
            torch.cuda.synchronize()
            assert_bits_equal(got.to_numpy(), oracle.conv_separable(img, KX5, KY5, border), f"sep {kind} {rows}x{cols} border={border}")


@pytest.mark.parametrize("kind", ("u8", "rgb_u8", "rgba_u8"))
def test_convolve_3x3_u8(oracle, kind):
    for rows, cols in shapes("convolve_3x3", kind, 3):
        img = synth(oracle, kind, 2000 + rows + cols, rows, cols)
        src = dev(img)
        for border in BORDERS:
            got = src.convolve(K3X3, border)
            torch.cuda.synchronize()
            assert_bits_equal(got.to_numpy(), oracle.convolve(img, K3X3, border), f"3x3 {kind} {rows}x{cols} border={border}")


@pytest.mark.parametrize("kind", ("u8", "rgba_u8"))
def test_sobel(oracle, kind):
    for rows, cols in shapes("sobel", kind, 3):
        img = synth(oracle, kind, 3000 + rows + cols, rows, cols)
        got = dev(img).sobel()
        torch.cuda.synchronize()
        assert_bits_equal(got.to_numpy(), oracle.sobel(img), f"sobel {kind} {rows}x{cols}")


@pytest.mark.parametrize("planes", (1, 4))
def test_separable_f32(oracle, planes):
    """One plane (every lane asks for its halo) and four planes through the planes entry (the tile's outer lanes only)."""
    for rows, cols in shapes("separable_f32", "f32", 5, planes):
        imgs = [synth(oracle, "f32", 4000 + rows + cols + p, rows, cols) - np.float32(0.5) for p in range(planes)]
        srcs = [dev(i) for i in imgs]
        for border in BORDERS:
            gots = [srcs[0].convolve_separable(KXF, KYF, border)] if planes == 1 else zg.convolve_separable_planes(srcs, KXF, KYF, border)
            torch.cuda.synchronize()
            for img, got in zip(imgs, gots):
                assert_bits_equal(got.to_numpy(), oracle.conv_separable(img, KXF, KYF, border), f"f32 x{planes} {rows}x{cols} border={border}")


@pytest.mark.parametrize("op", ("separable_u8", "convolve_3x3", "sobel", "separable_f32"))
def test_views_with_a_pitch_past_the_row(oracle, op):
    """Source and destination are 16-byte aligned views of larger frames (70 x 264 pixels inside 80 x 320: the pitch exceeds the row,
    the second strip is two lanes wide for the 4-byte pixels); the bytes around the destination view stay as they were."""
    kind = "f32" if op == "separable_f32" else "rgba_u8"
    rows, cols, border = 70, 264, zg.BorderMode.mirror
    assert takes_strip_route(op, kind, rows, cols, 3 if op in ("convolve_3x3", "sobel") else 5, src_pitch_px=320, dst_pitch_px=320)
    base = synth(oracle, kind, 77, 80, 320)
    img = np.ascontiguousarray(base[6:6 + rows, 16:16 + cols])
    src = zg.Image(torch.from_numpy(base).cuda()).view((16, 6, 16 + cols, 6 + rows))
    if op == "sobel":
        fill, want = 0x55, oracle.sobel(img)
        dst_t = torch.full((80, 320), fill, dtype=torch.uint8, device="cuda")
    else:
        fill = 7.0 if kind == "f32" else 0x55
        dst_t = torch.full(base.shape, fill, dtype=torch.float32 if kind == "f32" else torch.uint8, device="cuda")
    dst = zg.Image(dst_t).view((32, 3, 32 + cols, 3 + rows))
    if op == "separable_u8":
        want = oracle.conv_separable(img, KX5, KY5, border)
        src.convolve_separable(KX5, KY5, border, out=dst)
    elif op == "convolve_3x3":
        want = oracle.convolve(img, K3X3, border)
        src.convolve(K3X3, border, out=dst)
    elif op == "sobel":
        src.sobel(out=dst)
    else:
        want = oracle.conv_separable(img, KXF, KYF, border)
        src.convolve_separable(KXF, KYF, border, out=dst)
    torch.cuda.synchronize()
    got = dst_t.cpu().numpy()
    assert_bits_equal(got[3:3 + rows, 32:32 + cols], want, f"{op} view")
    got[3:3 + rows, 32:32 + cols] = fill
    assert np.all(got == fill), f"{op}: bytes outside the destination view were written"

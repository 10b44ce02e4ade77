"""Frames, views and batches past 2 and 4 GiB, against the oracle bit for bit (the reference's Image(T) has usize rows, cols and stride,
image.zig:97-103). The fast kernels address a frame with 32-bit buffer descriptors or 32-bit voffset / soffset arithmetic, each behind a
host-side size guard that sends larger inputs to a general route or switches a frame-wide fast path off inside the kernel. Every case
here sits on one side of such a guard and asserts which side, from its own shape and pitch:

  * huge-pitch views: a small rows x cols image in the left columns of a buffer whose row pitch puts rows x pitch x pixel bytes between
    2^31 and 2^32 (the fast route, with offsets past 2^31) or past 2^32 (the general route). The buffers hold a sentinel; after each call
    every destination byte outside the view must still hold it, which catches a wrapped offset that writes inside the buffer;
  * large contiguous frames generated on the device, checked by row bands (the first rows, the rows at the 2^31 and 2^32 byte offsets,
    the last rows) against the oracle run on the band padded by the kernel's half-height;
  * batches above 4 GiB through zg_batch_pipeline and zg_batch_blur_resize, checked frame by frame at the 2^31 / 2^32 crossings.

The row-pitch limits of the stream and tile kernels (2^31 - 1 bytes) are crossed by one 16-row view at a time (their minimum height), 30 GiB,
with the other side of the call compact; the pyramid level at a pitch past 2^32 bytes is 28 GiB, the in-place box blur at a 256 MiB pitch
16 GiB. Every other case stays below 9 GiB."""
import ctypes as C

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests.util import assert_bits_equal, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I = zg.Interpolation
GIB = 1 << 30
SENTINEL = 0xA5
SENTINEL64 = int.from_bytes(bytes([SENTINEL]) * 8, "little", signed=True)
LAYOUT = {"u8": (torch.uint8, 1), "rgb_u8": (torch.uint8, 3), "rgba_u8": (torch.uint8, 4),
          "f32": (torch.float32, 1), "rgb_f32": (torch.float32, 3), "rgba_f32": (torch.float32, 4)}
# byte totals of rows x pitch x pixel bytes: below 4 GiB with offsets past 2^31, and past 4 GiB
BANDS = {"2to4g": 3 * GIB, "past4g": 4 * GIB + GIB // 4}
ROWS, COLS = 96, 704  # rows x cols >= 65793: boxBlur / sharpen leave k_box_direct; row bytes % 16 == 0 for every pixel size


def psize(kind):
    dtype, ch = LAYOUT[kind]
    return ch * (1 if dtype == torch.uint8 else 4)


def pitch_for(rows, kind, band):
    """Row pitch in pixels (a multiple of 64) for which rows x pitch x pixel bytes is about BANDS[band]."""
    p = -(-BANDS[band] // (rows * psize(kind)))
    return -(-p // 64) * 64


def frame_bytes(rows, pitch, kind):  # zg_sample.h (buffer gathers), resize_planes.hip (row taps): rows * stride * pixel bytes < 2^32
    return rows * pitch * psize(kind)


def span(rows, pitch, cols, kind):  # the stream and tile kernels' fast_ok: (rows - 1) * pitch + row bytes
    return ((rows - 1) * pitch + cols) * psize(kind)


def assert_band(band, nbytes, limit=1 << 32, inclusive=False):
    """The case is on the side of a `< limit` (or `<= limit`) guard that its band names, with offsets past 2^31 on the fast side."""
    fast = nbytes <= limit if inclusive else nbytes < limit
    assert fast == (band == "2to4g") and nbytes >= (1 << 31), (band, nbytes, limit)


class Pitched:
    """rows x cols pixels of `kind` at a row pitch of `pitch` pixels, in a device buffer of (rows - 1) x pitch + cols pixels (the last row's
    tail is not allocated) filled with the sentinel byte."""

    def __init__(self, kind, rows, cols, pitch):
        dtype, ch = LAYOUT[kind]
        self.kind, self.rows, self.cols, self.pitch = kind, rows, cols, pitch
        nbytes = ((rows - 1) * pitch + cols) * psize(kind)
        self.flat = torch.full(((nbytes + 7) // 8 * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        typed = self.flat[:nbytes].view(dtype)
        shape, strides = ((rows, cols), (pitch, 1)) if ch == 1 else ((rows, cols, ch), (pitch * ch, ch, 1))
        self.view = torch.as_strided(typed, shape, strides)
        self.bytes = torch.as_strided(self.flat, (rows, cols * psize(kind)), (pitch * psize(kind), 1))

    def image(self, c0=0, c1=None):
        return zg.Image(self.view[:, c0:c1])

    def put(self, host):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(host)))

    def take(self, what):
        """The view's pixels, then the view back to the sentinel and every byte of the buffer checked on the device."""
        torch.cuda.synchronize()
        got = self.view.cpu().numpy()
        self.bytes.fill_(SENTINEL)
        # by slices of 2 GiB: a mask of the whole buffer reduced in one go (count_nonzero widens it to int64) costs twice the buffer
        words = self.flat.view(torch.int64)
        for w0 in range(0, words.numel(), 1 << 28):
            bad = words[w0:w0 + (1 << 28)] != SENTINEL64
            if bool(bad.any()):
                stray = torch.nonzero(bad)
                raise AssertionError(f"{what}: {stray.numel()} 8-byte words outside the view were written, the first at byte "
                                     f"{(w0 + int(stray[0])) * 8}")
        return got


def release():
    """After the caller's `del`: the freed blocks go back to the device before the next case allocates."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _release_after_each_case():
    yield
    release()


def pair(oracle, kind, band, seed, rows=ROWS, cols=COLS, dst_kind=None, dst_shape=None):
    host = synth(oracle, kind, seed, rows, cols)
    src = Pitched(kind, rows, cols, pitch_for(rows, kind, band))
    src.put(host)
    dk = dst_kind or kind
    dr, dc = dst_shape or (rows, cols)
    dst = Pitched(dk, dr, dc, pitch_for(dr, dk, band))
    return host, src, dst


def check(dst, want, what):
    assert_bits_equal(dst.take(what), want, what)


# ---- 1. huge-pitch views ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("kind", ("u8", "rgb_u8", "rgba_u8", "f32"))
def test_separable_on_huge_pitch_views(oracle, kind, band):
    """gaussianBlur 0.6 (5 taps) and 1.2 (9 taps) and convolveSeparable. Rgb(u8) / Rgba(u8) 5 taps run k_sep_stream, whose fast_ok is
    span <= 2^32 - 1; Image(f32) 5 taps runs k_sep_tile_f32, whose fast_ok is span <= 2^32 - 256."""
    host, src, dst = pair(oracle, kind, band, 1)
    s = span(ROWS, src.pitch, COLS, kind)
    assert_band(band, s, 0xffffffff, inclusive=True)
    if kind == "f32":
        assert_band(band, s, 0xffffff00, inclusive=True)
    for sigma in (0.6, 1.2):
        src.image().gaussian_blur(sigma, out=dst.image())
        check(dst, oracle.gaussian_blur(host, sigma), f"{kind} {band} gaussianBlur({sigma})")
    kx = np.array([1, 3, 8, 3, 1], np.float32) / 16
    ky = np.array([2, 5, 6, 2, 1], np.float32) / 16
    for border in (zg.BorderMode.mirror, zg.BorderMode.replicate):
        src.image().convolve_separable(kx, ky, border, out=dst.image())
        check(dst, oracle.conv_separable(host, kx, ky, border), f"{kind} {band} convolveSeparable border {border}")
    del src, dst


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_planes_entry_on_huge_pitch_views(oracle, kind, band):
    """zg_gaussian_blur_planes / zg_conv_separable_planes over three planes side by side in one huge-pitch buffer (Image(f32) planes take
    k_sep_tile_f32 with its outer loop, fast_ok span <= 2^32 - 256; Image(u8) planes the tiled k_sep_bytes)."""
    n = 3
    hosts = [synth(oracle, kind, 10 + p, ROWS, COLS) for p in range(n)]
    pitch = pitch_for(ROWS, kind, band)
    assert_band(band, span(ROWS, pitch, COLS, kind), 0xffffff00 if kind == "f32" else 0xffffffff, inclusive=True)
    src, dst = Pitched(kind, ROWS, n * COLS, pitch), Pitched(kind, ROWS, n * COLS, pitch)
    src.put(np.concatenate(hosts, axis=1))
    planes = [src.image(p * COLS, (p + 1) * COLS) for p in range(n)]
    outs = [dst.image(p * COLS, (p + 1) * COLS) for p in range(n)]
    zg.gaussian_blur_planes(planes, 0.6, outs)
    got = dst.take(f"{kind} {band} planes blur")
    for p in range(n):
        assert_bits_equal(got[:, p * COLS:(p + 1) * COLS], oracle.gaussian_blur(hosts[p], 0.6), f"{kind} {band} planes blur, plane {p}")
    kx = np.array([1, 2, 1], np.float32) / 4
    ky = np.array([1, 6, 1], np.float32) / 8
    zg.convolve_separable_planes(planes, kx, ky, zg.BorderMode.wrap, outs)
    got = dst.take(f"{kind} {band} planes convolveSeparable")
    for p in range(n):
        assert_bits_equal(got[:, p * COLS:(p + 1) * COLS], oracle.conv_separable(hosts[p], kx, ky, zg.BorderMode.wrap),
                          f"{kind} {band} planes convolveSeparable, plane {p}")
    del src, dst


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("kind", ("u8", "rgb_u8", "rgba_u8", "f32"))
def test_convolve_on_huge_pitch_views(oracle, kind, band):
    """convolve 3 x 3 and 5 x 5: k_conv2d_stream for the u8 types (fast_ok: span <= 2^32 - 1), k_conv2d for Image(f32)."""
    host, src, dst = pair(oracle, kind, band, 2)
    assert_band(band, span(ROWS, src.pitch, COLS, kind), 0xffffffff, inclusive=True)
    rng = np.random.default_rng(3)
    for n in (3, 5):
        k = rng.normal(0, 1, (n, n)).astype(np.float32)
        k /= np.abs(k).sum()
        src.image().convolve(k, zg.BorderMode.mirror, out=dst.image())
        check(dst, oracle.convolve(host, k, zg.BorderMode.mirror), f"{kind} {band} convolve {n}x{n}")
    del src, dst


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("kind", ("u8", "rgba_u8"))
def test_sobel_on_huge_pitch_views(oracle, kind, band):
    """k_sobel_stream: fast_ok is source and destination span <= 2^32 - 1 (the destination an Image(u8) view of its own pitch)."""
    host, src, dst = pair(oracle, kind, band, 4, dst_kind="u8")
    assert_band(band, span(ROWS, src.pitch, COLS, kind), 0xffffffff, inclusive=True)
    assert_band(band, span(ROWS, dst.pitch, COLS, "u8"), 0xffffffff, inclusive=True)
    src.image().sobel(out=dst.image())
    check(dst, oracle.sobel(host), f"{kind} {band} sobel")
    del src, dst


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("kind", ("u8", "rgba_u8"))
def test_box_blur_and_sharpen_on_huge_pitch_views(oracle, kind, band):
    """Radius 2: k_box_fused while the frame's 32-bit offsets hold (rows x stride x channels + 64 < 2^32, box_fused.hip), the integral-image
    route past that; radius 5: always the integral image (k_box_mean with BUF, the SAT is small). Then the in-place call at radius 2, whose
    source k_box_fused copies to a compact buffer first (the frame guard then counts cols, not the stride)."""
    host, src, dst = pair(oracle, kind, band, 5)
    ch = LAYOUT[kind][1]
    assert_band(band, ROWS * src.pitch * ch + 64)
    assert src.pitch * ch * 16 + COLS * ch < (1 << 32)
    for radius in (2, 5):
        src.image().box_blur(radius, out=dst.image())
        check(dst, oracle.box_blur(host, radius), f"{kind} {band} boxBlur({radius})")
        src.image().sharpen(radius, out=dst.image())
        check(dst, oracle.sharpen(host, radius), f"{kind} {band} sharpen({radius})")
    del dst
    release()
    img = src.image()
    img.box_blur(2, out=img)
    check(src, oracle.box_blur(host, 2), f"{kind} {band} boxBlur(2) in place")
    del src


def test_box_blur_in_place_with_a_256_mib_pitch(oracle):
    """The in-place k_box_fused call counts its frame by cols, so its other guard decides: a wave's sixteen rows need stride x 16 + cols below
    2^32 bytes (box_fused.hip). A 64-row Image(u8) view at a pitch of 2^28 + 64 bytes (16 GiB) is past it and takes the integral image."""
    rows, cols = 64, 1088  # rows x cols >= 65793 (not k_box_direct), rows >= 64
    pitch = (1 << 28) + 64
    assert pitch * 16 + cols >= (1 << 32) and rows * (cols + 3) + 64 < (1 << 32)
    host = synth(oracle, "u8", 6, rows, cols)
    buf = Pitched("u8", rows, cols, pitch)
    buf.put(host)
    img = buf.image()
    img.box_blur(2, out=img)
    check(buf, oracle.box_blur(host, 2), "u8 boxBlur(2) in place, 256 MiB pitch")
    del buf


PITCH_PAST_2_31 = (1 << 31) + 64  # bytes


@pytest.mark.parametrize("side", ("source", "destination"))
@pytest.mark.parametrize("kind", ("rgba_u8", "f32"))
def test_row_pitch_past_2_31_bytes(oracle, kind, side):
    """k_sep_stream, k_conv2d_stream, k_sobel_stream and k_sep_tile_f32 take source and destination pitches up to 2^31 - 1 bytes
    (conv_sep_stream.hip, conv2d_stream.hip, sobel_stream.hip, conv_sep_tile_f32.hip); past that the call goes to the tiled kernels. A 16-row
    view (their minimum height) at a pitch of 2^31 + 64 bytes is 30 GiB, so one side of each call has that pitch and the other is compact."""
    rows, cols = 16, COLS
    host = synth(oracle, kind, 13, rows, cols)
    if side == "source":
        big = Pitched(kind, rows, cols, PITCH_PAST_2_31 // psize(kind))
        assert big.pitch * psize(kind) > 0x7fffffff
        big.put(host)
        src = big.image()
    else:
        src = zg.Image(torch.from_numpy(host).cuda())
    k3 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float32) / 16
    k = np.array([1, 2, 1], np.float32) / 4
    ops = [("gaussianBlur(0.6)", kind, lambda s, d: s.gaussian_blur(0.6, out=d), oracle.gaussian_blur(host, 0.6))]
    if kind == "rgba_u8":
        ops += [("convolve 3x3", kind, lambda s, d: s.convolve(k3, zg.BorderMode.mirror, out=d), oracle.convolve(host, k3, zg.BorderMode.mirror)),
                ("sobel", "u8", lambda s, d: s.sobel(out=d), oracle.sobel(host))]
    else:
        ops += [("convolveSeparable 3 taps", kind, lambda s, d: s.convolve_separable(k, k, zg.BorderMode.mirror, out=d),
                 oracle.conv_separable(host, k, k, zg.BorderMode.mirror))]
    for what, out_kind, call, want in ops:
        what = f"{kind} {what}, {side} pitch 2^31 + 64 bytes"
        if side == "source":
            dtype, ch = LAYOUT[out_kind]
            out = zg.Image(torch.empty((rows, cols) if ch == 1 else (rows, cols, ch), dtype=dtype, device="cuda"))
            call(src, out)
            torch.cuda.synchronize()
            assert_bits_equal(out.to_numpy(), want, what)
        else:
            dst = Pitched(out_kind, rows, cols, PITCH_PAST_2_31 // psize(out_kind))
            assert dst.pitch * psize(out_kind) > 0x7fffffff
            call(src, dst.image())
            check(dst, want, what)
            del dst
            release()


RESAMPLE_KINDS = ("rgba_u8", "f32", "rgba_f32")


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("kind", RESAMPLE_KINDS)
def test_resize_on_huge_pitch_views(oracle, kind, band):
    """resize bilinear and bicubic, shrinking and growing. Rgba(u8) bicubic runs k_resize_planes, whose row taps are 16-byte buffer loads
    while rows x stride x 4 < 2^32; the 4- and 16-byte pixels gather with buffer loads below the same limit (zg_sample.h)."""
    host = synth(oracle, kind, 7, ROWS, COLS)
    src = Pitched(kind, ROWS, COLS, pitch_for(ROWS, kind, band))
    src.put(host)
    assert_band(band, frame_bytes(ROWS, src.pitch, kind))
    for shape in ((61, 450), (150, 1000)):
        dst = Pitched(kind, shape[0], shape[1], pitch_for(shape[0], kind, band))
        assert_band(band, frame_bytes(shape[0], dst.pitch, kind))
        for m, om in ((I.bilinear, oracle.BILINEAR), (I.bicubic, oracle.BICUBIC)):
            src.image().resize(dst.image(), m)
            check(dst, oracle.resize(host, shape, oracle.method(om)), f"{kind} {band} resize {shape} {m}")
        del dst
        release()
    del src


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("kind", RESAMPLE_KINDS)
def test_warp_rotate_extract_on_huge_pitch_views(oracle, kind, band):
    """warp (affine), rotate and extract, bilinear and bicubic: the W x W window gathers of zg_sample.h, buffer loads with int voffset /
    soffset products while rows x stride x pixel bytes < 2^32 (the Rgba(f32) bicubic one staged through LDS), the general path past it."""
    host = synth(oracle, kind, 8, ROWS, COLS)
    src = Pitched(kind, ROWS, COLS, pitch_for(ROWS, kind, band))
    src.put(host)
    assert_band(band, frame_bytes(ROWS, src.pitch, kind))
    aff = zg.AffineTransform([[0.97, 0.04], [-0.03, 0.98]], [3.5, 1.25])
    angle = 0.05
    cs = oracle.cos_sin(angle)
    cs_extract = oracle.cos_sin(0.1)
    rot = oracle.rotate_bounds(ROWS, COLS, angle)
    rect = (20.5, 10.25, 620.5, 90.25)
    for m, om in ((I.bilinear, oracle.BILINEAR), (I.bicubic, oracle.BICUBIC)):
        dst = Pitched(kind, ROWS, COLS, pitch_for(ROWS, kind, band))
        src.image().warp(aff, dst.image(), m)
        check(dst, oracle.warp(host, (ROWS, COLS), oracle.AFFINE, aff.coefficients(), oracle.method(om)), f"{kind} {band} warp {m}")
        del dst
        release()
        dst = Pitched(kind, rot[0], rot[1], pitch_for(rot[0], kind, band))
        src.image().rotate_into(dst.image(), angle, m, zg.BorderMode.zero, cos_sin=cs)
        want = np.empty(dst.view.shape, host.dtype)
        check(dst, oracle.rotate_into(host, want, angle, oracle.method(om), zg.BorderMode.zero), f"{kind} {band} rotate {m}")
        del dst
        release()
        dst = Pitched(kind, 70, 520, pitch_for(70, kind, band))
        src.image().extract(rect, 0.1, dst.image(), m, zg.BorderMode.replicate, cos_sin=cs_extract)
        want = np.empty(dst.view.shape, host.dtype)
        check(dst, oracle.extract(host, want, rect, 0.1, oracle.method(om), zg.BorderMode.replicate), f"{kind} {band} extract {m}")
        del dst
        release()
    del src


@pytest.mark.parametrize("band", BANDS)
def test_convert_to_oklab_on_huge_pitch_views(oracle, band):
    host, src, dst = pair(oracle, "rgba_u8", band, 9, dst_kind="rgb_f32")
    assert_band(band, frame_bytes(ROWS, src.pitch, "rgba_u8"))
    assert_band(band, frame_bytes(ROWS, dst.pitch, "rgb_f32"))
    src.image().convert(zg.CS_OKLAB, np.float32, out=dst.image())
    check(dst, oracle.convert(host, oracle.CS_RGBA, oracle.CS_OKLAB, np.float32, 3), f"{band} convert Oklab")
    del src, dst


@pytest.mark.parametrize("band", ("tile", "multi"))
def test_pyramid_level_on_a_huge_pitch_view(oracle, band):
    """zg_pyramid_build with its one level an 8-row Image(u8) view, reduced by 1.5 (k_pyr_tile takes ratios from 1.3): k_pyr_tile while the
    level's stride is below 2^32 pixels (here 400 MiB, offsets past 2^31); past it the level goes level by level (a blurred plane, then
    k_resize_bilinear_u8_rows), since round 5's multi-job kernels batch two levels or more. 28 GiB: the one case this large."""
    rows, cols = 12, 300
    host = synth(oracle, "u8", 12, rows, cols)
    want = oracle.pyramid(host, 2, 1.5, 1.6)[1]
    lr, lc = want.shape
    assert lr == 8
    pitch = 400 << 20 if band == "tile" else (1 << 32) + 64
    assert (pitch > 0xffffffff) == (band == "multi") and (lr - 1) * pitch >= (1 << 31)
    src = zg.Image(torch.from_numpy(host).cuda())
    level = Pitched("u8", lr, lc, pitch)
    lib = zg.lib()
    r, c, sigma = C.c_uint32(), C.c_uint32(), C.c_float()
    L.check(lib.zg_pyramid_level(rows, cols, C.c_float(lib.zg_pyramid_scale(C.c_float(1.5), 1)), C.c_float(1.6), C.byref(r), C.byref(c), C.byref(sigma)))
    assert (r.value, c.value) == (lr, lc) and sigma.value > 0.5
    sd, descs = src._desc(), (L.ZgImage * 1)(level.image()._desc())
    L.check(lib.zg_pyramid_build(C.byref(sd), descs, (C.c_float * 1)(sigma.value), 1, src._stream()))
    check(level, want, f"pyramid level, {band} pitch")
    del level, src


# ---- 2. large contiguous frames, checked by row bands ----------------------------------------------------------------------------------

def device_frame(kind, rows, cols, seed):
    dtype, ch = LAYOUT[kind]
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
    return torch.rand(shape, dtype=torch.float32, device="cuda", generator=gen)


def bands(rows, row_bytes, height=6):
    """Row ranges [a, b): the first rows, the rows around the 2^31 and 2^32 byte offsets, the last rows."""
    out = [(0, height)]
    for off in (1 << 31, 1 << 32):
        r = off // row_bytes
        if r < rows:
            out.append((max(0, r - height // 2), min(rows, r + height // 2 + 1)))
    return out + [(rows - height, rows)]


def check_bands(src, got, ref, halo, what):
    """got (device) against ref(host band) on each band of rows; ref runs on the band padded by `halo` rows (not past the frame's edges)."""
    rows = src.shape[0]
    torch.cuda.synchronize()
    row_bytes = src[0].numel() * src.element_size()
    for a, b in bands(rows, row_bytes):
        pa, pb = max(0, a - halo), min(rows, b + halo)
        want = ref(src[pa:pb].cpu().numpy())[a - pa:b - pa]
        assert_bits_equal(got[a:b].cpu().numpy(), want, f"{what}, rows {a}..{b}")


def test_headline_blur_on_a_4_gib_rgba_f32_frame(oracle):
    """gaussianBlur(0.6) on a 16384 x 16400 Rgba(f32) frame (4.1 GiB in, 4.1 GiB out)."""
    src = device_frame("rgba_f32", 16384, 16400, 20)
    assert src.numel() * 4 > (1 << 32)
    out = zg.Image(src).gaussian_blur(0.6)
    check_bands(src, out.data, lambda b: oracle.gaussian_blur(b, 0.6), 2, "Rgba(f32) 16384 x 16400 gaussianBlur(0.6)")
    del src, out


def test_stream_kernels_on_a_4_gib_rgba_u8_frame(oracle):
    """convolve 3 x 3 (k_conv2d_stream) and sobel (k_sobel_stream) on a 16384 x 65600 Rgba(u8) frame: span past 2^32, fast_ok off."""
    rows, cols = 16384, 65600
    src = device_frame("rgba_u8", rows, cols, 21)
    assert span(rows, cols, cols, "rgba_u8") > 0xffffffff and cols * 4 % 16 == 0 and cols * 4 <= 0x3fffffff
    k = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float32) / 16
    out = zg.Image(src).convolve(k, zg.BorderMode.mirror)
    check_bands(src, out.data, lambda b: oracle.convolve(b, k, zg.BorderMode.mirror), 1, "Rgba(u8) 16384 x 65600 convolve 3x3")
    del out
    release()
    out = zg.Image(src).sobel()
    check_bands(src, out.data, oracle.sobel, 1, "Rgba(u8) 16384 x 65600 sobel")
    del src, out


def test_convert_into_a_4_gib_oklab_frame(oracle):
    """convert Rgba(u8) -> Oklab f32: a 1.3 GiB source into a 4.0 GiB destination."""
    src = device_frame("rgba_u8", 8192, 44000, 22)
    out = zg.Image(src).convert(zg.CS_OKLAB, np.float32)
    assert out.data.numel() * 4 > (1 << 32)
    torch.cuda.synchronize()
    for a, b in bands(8192, 44000 * 12):
        want = oracle.convert(src[a:b].cpu().numpy(), oracle.CS_RGBA, oracle.CS_OKLAB, np.float32, 3)
        assert_bits_equal(out.data[a:b].cpu().numpy(), want, f"convert Oklab rows {a}..{b}")
    del src, out


def test_box_blur_with_a_sat_past_4_gib(oracle):
    """boxBlur radius 5 on a 16384^2 Rgba(u8) frame: its SAT is 4 GiB, so k_box_mean<Rgba(u8), false, false> (no buffer loads) runs. The
    f32 SAT rounds globally, so the oracle runs on the whole frame (the one such case)."""
    rows = cols = 16384
    assert 4 * rows * cols * 4 >= (1 << 32)
    src = device_frame("rgba_u8", rows, cols, 23)
    out = zg.Image(src).box_blur(5)
    torch.cuda.synchronize()
    host = src.cpu().numpy()
    del src
    release()
    assert_bits_equal(out.to_numpy(), oracle.box_blur(host, 5), "Rgba(u8) 16384^2 boxBlur(5)")


# ---- 3. batches above 4 GiB ------------------------------------------------------------------------------------------------------------

N_FRAMES, FR, FC = 560, 1080, 1920  # 4.33 GiB of 1080p Rgba(u8)


def batch_frames_to_check(frame_bytes_in, frame_bytes_out):
    picks = {0, N_FRAMES - 1}
    for fb in (frame_bytes_in, frame_bytes_out):
        for off in (1 << 31, 1 << 32):
            if off // fb < N_FRAMES:
                picks.add(off // fb)
    return sorted(picks)


@pytest.fixture(scope="module")
def batch():
    t = device_frame("rgba_u8", N_FRAMES * FR, FC, 30).view(N_FRAMES, FR, FC, 4)
    assert t.numel() > (1 << 32) + (1 << 28)
    yield t
    del t
    release()


BATCH_RECIPES = {
    "blur": ([zg.Step.gaussian_blur(0.6)], lambda o, f: o.gaussian_blur(f, 0.6)),
    "resize": ([zg.Step.resize(540, 960)], lambda o, f: o.resize(f, (540, 960), o.method(o.BILINEAR))),
    "convert_edges": ([zg.Step.convert(zg.CS_GRAY, np.uint8), zg.Step.edges_sobel()],
                      lambda o, f: o.sobel(o.convert(f, o.CS_RGBA, o.CS_GRAY, np.uint8, 1))),
}


@pytest.mark.parametrize("recipe", BATCH_RECIPES)
def test_batch_pipeline_past_4_gib(oracle, batch, recipe):
    steps, ref = BATCH_RECIPES[recipe]
    out = zg.Pipeline(steps).run(batch)
    torch.cuda.synchronize()
    fb_out = out[0].numel() * out.element_size()
    for f in batch_frames_to_check(FR * FC * 4, fb_out):
        assert_bits_equal(out[f].cpu().numpy(), ref(oracle, batch[f].cpu().numpy()), f"pipeline {recipe}, frame {f}")
    del out


def test_batch_blur_resize_past_4_gib(oracle, batch):
    out = torch.empty((N_FRAMES, 540, 960, 4), dtype=torch.uint8, device="cuda")
    m = I.bilinear._c()
    rc = zg.lib().zg_batch_blur_resize(C.c_void_p(batch.data_ptr()), N_FRAMES, FR, FC, L.PIXEL_RGBA_U8, C.c_float(0.6), C.c_void_p(out.data_ptr()),
                                       540, 960, C.byref(m), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, zg.lib().zg_last_error()
    torch.cuda.synchronize()
    for f in batch_frames_to_check(FR * FC * 4, 540 * 960 * 4):
        want = oracle.resize(oracle.gaussian_blur(batch[f].cpu().numpy(), 0.6), (540, 960), oracle.method(oracle.BILINEAR))
        assert_bits_equal(out[f].cpu().numpy(), want, f"batch blur + resize, frame {f}")
    del out


# ---- edge detectors past their documented limit ----------------------------------------------------------------------------------------

def test_canny_and_shen_castan_refuse_2_31_pixels(oracle):
    """The hysteresis labels are 32-bit (edges.hip): at rows x cols >= 2^31 canny and shenCastan return ZG_ERR_UNSUPPORTED before any work,
    and the stream stays usable: a small call after them is bit-exact."""
    n = 46341
    assert n * n > 0x7fffffff
    big = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(big)
    with pytest.raises(zg.ZignalError) as e:
        zg.Image(big).canny(1.0, 50.0, 100.0, out=zg.Image(out))
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(zg.ZignalError) as e:
        zg.Image(big).shen_castan(out=zg.Image(out))
    assert e.value.status == L.ERR_UNSUPPORTED
    del big, out
    release()
    img = synth(oracle, "u8", 40, 120, 200)
    got = zg.Image(torch.from_numpy(img).cuda()).canny(1.0, 20.0, 60.0)
    torch.cuda.synchronize()
    assert_bits_equal(got.to_numpy(), oracle.canny(img, 1.0, 20.0, 60.0), "canny after the refusals")

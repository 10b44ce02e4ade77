"""Every device op into destination views, bit for bit against the oracle, with every byte outside the view checked (tests/views.py).

The fast kernels are chosen by host predicates over BOTH images of a call (origin & 15, stride % 4, row bytes % 16, rows % 2, row bytes
% 1024 == 16); behind each sit 64- and 128-bit stores. Into a fresh contiguous destination a store that runs past `cols` lands in the next
row and is overwritten by that row's own store; into a view of a larger frame it lands in the frame, where the sentinel shows it. Each case
puts source and destination in a named layout that flips ONE term relative to the all-aligned layout, and asserts the flip from the
canvases' own facts() (views.place does it for origin and stride, `shaped` below for row bytes and rows), so that a later change of
shape cannot quietly move a case to the other side of a predicate.

Pairs of layouts: the diagonal, the aligned source with every destination layout, every source layout with the aligned destination. Where an
op's source and destination share their shape, the layouts that change the shape (cols-1, cols-3, odd_rows, rb1040) change both sides.

Base shape 272 x 272: rows x cols >= 65793 leaves k_box_direct (box_blur.hip), cols >= 256 and cols % 16 == 0 admits the packed byte kernels
(conv_sep_bytes.hip, conv_sep_bytes2.hip) and the f32 long-tap one (conv_sep_f32long.hip), cols >= 64 and rows >= 16 the stream kernels."""
import ctypes as C

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import views as V
from tests.util import assert_bits_equal, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I = zg.Interpolation
BASE = (272, 272)
SHAPE_DELTAS = {"base": (0, 0), "cols-1": (0, -1), "cols-3": (0, -3), "odd_rows": (-1, 0)}
U8S = ("u8", "rgb_u8", "rgba_u8")
ALL = ("u8", "rgb_u8", "rgba_u8", "f32", "rgb_f32", "rgba_f32")

_hosts, _wants = {}, {}


def host_of(oracle, kind, shape, seed=1, prep=None):
    key = (kind, shape, seed, prep)
    if key not in _hosts:
        h = synth(oracle, kind, seed, *shape)
        if prep == "binary":
            h = ((h > 128) * 255).astype(np.uint8)
        elif prep == "lab":  # L in 0..100, a and b in -50..50
            h = (h * np.float32(100) - np.array([0, 50, 50], np.float32)).astype(np.float32)
        h.flags.writeable = False
        _hosts[key] = h
    return _hosts[key]


def want_of(key, make):
    """One oracle run per (op, kind, shapes), shared by every layout of that shape and left unchanged."""
    if key not in _wants:
        w = make()
        if isinstance(w, np.ndarray):
            w.flags.writeable = False
        _wants[key] = w
    return _wants[key]


def shaped(kind, base, variant, placement, src_kind=None):
    """A canvas of `kind` in the named shape variant and placement, the variant's flip asserted from facts(). src_kind: the source's pixel
    type where the two share their shape (rb1040 is a property of the source's row bytes)."""
    src_kind = src_kind or kind
    if variant == "rb1040":  # row bytes k * 1024 + 16: the strip kernels' "the last strip would be one lane wide" exclusion
        rows, cols = base[0], 1040 // V.psize(src_kind)
    else:
        dr, dc = SHAPE_DELTAS[variant]
        rows, cols = base[0] + dr, base[1] + dc
    c = V.place(kind, rows, cols, placement)
    f = c.facts()
    p = V.psize(kind)
    if variant == "base":
        assert f["rows%2"] == 0 and f["cols%4"] == 0 and (f["row_bytes%16"] == 0 or p == 3), (kind, variant, f)
    elif variant in ("cols-1", "cols-3"):
        assert f["rows%2"] == 0 and (f["row_bytes%16"] != 0 if p != 16 else f["cols%4"] != 0), (kind, variant, f)
    elif variant == "odd_rows":
        assert f["rows%2"] == 1 and f["cols%4"] == 0, (kind, variant, f)
    else:
        assert cols * V.psize(src_kind) % 1024 == 16 and (f["row_bytes%16"] == 0 or src_kind != kind), (kind, variant, f)
    return c


def layout_pairs(src_kind, dst_kind, shared_shape, extra_variants=()):
    """(variant, source placement, destination placement): the diagonal, aligned source x every destination layout, every source layout x
    aligned destination. With a shared shape a shape variant is one case (both sides take it)."""
    ps, pd = V.placements(src_kind), V.placements(dst_kind)
    out = [("base", "aligned", "aligned")]
    for pl in V.PLACEMENTS[1:]:
        if pl in ps and pl in pd:
            out.append(("base", pl, pl))
        if pl in pd:
            out.append(("base", "aligned", pl))
        if pl in ps:
            out.append(("base", pl, "aligned"))
    for v in tuple(SHAPE_DELTAS)[1:] + tuple(extra_variants):
        if v == "rb1040" and 1040 % V.psize(src_kind if shared_shape else dst_kind):
            continue
        out.append((v, "aligned", "aligned"))
    return out


class Op:
    """call(src_image, dst_image); ref(oracle, host) -> the expected destination pixels. dst_kind: the destination's pixel type (the source's
    by default). src_shape: None when source and destination share their shape, else the source's fixed shape (the destination's varies)."""

    def __init__(self, name, kinds, call, ref, dst_kind=None, src_shape=None, base=BASE, prep=None, variants=()):
        self.name, self.kinds, self.call, self.ref, self.dst_kind, self.src_shape, self.base, self.prep, self.variants = (
            name, kinds, call, ref, dst_kind, src_shape, base, prep, variants)

    def cases(self):
        out = []
        for kind in self.kinds:
            dk = self.dst_kind(kind) if callable(self.dst_kind) else (self.dst_kind or kind)
            for v, sp, dp in layout_pairs(kind, dk, self.src_shape is None, self.variants):
                out.append(pytest.param(self, kind, dk, v, sp, dp, id=f"{self.name}-{kind}-{v}-{sp}>{dp}"))
        return out


def run_case(oracle, op, kind, dk, variant, sp, dp):
    dst = shaped(dk, op.base, variant, dp, kind if op.src_shape is None else None)
    if op.src_shape is None:
        src = shaped(kind, op.base, variant, sp)
    else:
        src = V.place(kind, op.src_shape[0], op.src_shape[1], sp)
    host = host_of(oracle, kind, (src.rows, src.cols), prep=op.prep)
    src.put(host)
    what = f"{op.name} {kind} {variant} {sp}>{dp} src {src.facts()} dst {dst.facts()}"
    op.call(src.image(), dst.image())
    want = want_of((op.name, kind, (src.rows, src.cols), (dst.rows, dst.cols)), lambda: op.ref(oracle, host, (dst.rows, dst.cols)))
    got = dst.take(what)  # raises on a byte written outside the destination view
    assert_bits_equal(got, want, what)
    assert_bits_equal(src.take(what + " (source)"), host, what + ": the source changed")


def cases(*ops):
    return [c for op in ops for c in op.cases()]


CASE = "op,kind,dk,variant,sp,dp"

# ---- separable convolutions ------------------------------------------------------------------------------------------------------------
K5 = np.array([-0.1, 0.3, 0.6, 0.3, -0.1], np.float32)
K13 = (np.array([1, -2, 3, -4, 5, 6, 9, 6, 5, -4, 3, -2, 1], np.float32) / np.float32(27)).astype(np.float32)


def blur(sigma):
    return Op(f"gaussian_blur_{sigma}", ALL, lambda s, d: s.gaussian_blur(sigma, out=d), lambda o, h, _: o.gaussian_blur(h, sigma), variants=("rb1040",))


# gaussian_blur 0.6 is 5 taps, 1.0 is 7, 2.5 is 17 (image.zig:973-990).
#   conv_sep_stream.hip:462-468  Rgb(u8) / Rgba(u8), 5 and 7 taps: rb % 16 (cols-1, cols-3), src / dst pitch % 16 (stride+4B, stride+1px), src / dst
#                                origin & 15 (origin+4B, +8B, +1px), rb % 1024 == 16 (rb1040); :466 is the down2 form (rows % 2), which only the
#                                pipeline's blur + half resize reaches: test_pipeline_into_out below, odd_rows here stays on the full-size form
#   conv_sep_rgba8.hip:241-245   what Rgba(u8) takes when the stream predicate refuses: cols % 4 (cols-1), stride % 4 (stride+4B), origin & 15
#   conv_sep_bytes.hip:231       Image(u8), 5 / 7 taps (one grey plane leaves the stream kernel): row bytes, both strides, both origins % 16
#   conv_sep_bytes2.hip:832      the packed two-pass kernels, 17 taps on the u8 types: the same five terms
#   conv_sep_tile_f32.hip:240    Image(f32), 5 / 7 taps: cols % 4, strides % 4, origins & 15, (cols * 4) % 1024 == 16 (rb1040)
#   conv_sep_f32x4.hip:165       Image(f32) where the tile kernel refuses (9 taps: convolve_separable_9 below): cols % 4, strides % 4, origins & 15
#   conv_sep_f32long.hip:215     f32 types, 17 taps: row floats % 4, src pitch % 16 bytes, dst pitch % 4 floats, origins & 15
# Rgb(f32) / Rgba(f32) take k_sep_fused (conv_separable.hip), which has no alignment term: every layout must equal the oracle there too.
SEPARABLE = cases(
    blur(0.6), blur(1.0), blur(2.5),
    Op("convolve_separable_5", ("f32", "rgba_f32"), lambda s, d: s.convolve_separable(K5, K5, zg.BorderMode.mirror, out=d),
       lambda o, h, _: o.conv_separable(h, K5, K5, zg.BorderMode.mirror), variants=("rb1040",)),
    Op("convolve_separable_9", ("f32",), lambda s, d: s.convolve_separable(K13[2:11], K13[2:11], zg.BorderMode.replicate, out=d),
       lambda o, h, _: o.conv_separable(h, K13[2:11], K13[2:11], zg.BorderMode.replicate)),
    Op("convolve_separable_13", ("f32", "rgba_f32"), lambda s, d: s.convolve_separable(K13, K13, zg.BorderMode.mirror, out=d),
       lambda o, h, _: o.conv_separable(h, K13, K13, zg.BorderMode.mirror)),
)


@pytest.mark.parametrize(CASE, SEPARABLE)
def test_separable_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- 2-D convolution -------------------------------------------------------------------------------------------------------------------
def conv2d(n):
    rng = np.random.default_rng(n)
    k = rng.normal(0, 1, (n, n)).astype(np.float32)
    k /= np.abs(k).sum()
    return Op(f"convolve_{n}x{n}", ("u8", "rgba_u8", "f32"), lambda s, d: s.convolve(k, zg.BorderMode.mirror, out=d),
              lambda o, h, _: o.convolve(h, k, zg.BorderMode.mirror), variants=("rb1040",))


# conv2d_stream.hip:294  3 x 3 and 5 x 5 on the u8 types: rb % 16 (cols-1, cols-3), sp_pitch / dp_pitch % 16 (stride+4B, stride+1px), src / dst
#                        origin & 15 (origin+...), rb % 1024 == 16 (rb1040). 7 x 7 and Image(f32) stay on k_conv2d, which has no such term.
CONV2D = cases(conv2d(3), conv2d(5), conv2d(7))


@pytest.mark.parametrize(CASE, CONV2D)
def test_convolve_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- box blur and sharpen --------------------------------------------------------------------------------------------------------------
# box_fused.hip:860  u8 planes and Rgba(u8), radius 1..3: dst origin & 3 and dst stride x channels % 4 (origin+1px, stride+1px on Image(u8) /
#                    Rgb(u8) leave it for the integral-image route), :867 the same two terms on the source copy it aside first.
BOX = cases(Op("box_blur_2", ALL, lambda s, d: s.box_blur(2, out=d), lambda o, h, _: o.box_blur(h, 2)),
            Op("sharpen_2", U8S + ("f32",), lambda s, d: s.sharpen(2, out=d), lambda o, h, _: o.sharpen(h, 2)))


@pytest.mark.parametrize(CASE, BOX)
def test_box_blur_and_sharpen_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- edge detectors --------------------------------------------------------------------------------------------------------------------
# sobel_stream.hip:229-232  Image(u8) / Rgba(u8): src rb % 16, src pitch % 16, src origin & 15; the destination is an Image(u8) whose unit is 16
#                           bytes for a u8 source and 4 for an Rgba(u8) one: dst stride % dalign, dst origin & (dalign - 1); rb % 1024 == 16
#                           (rb1040: 1040 columns of u8, 260 of Rgba(u8)). Image(f32) runs k_sobel.
EDGES = cases(
    Op("sobel", ("u8", "rgba_u8", "f32"), lambda s, d: s.sobel(out=d), lambda o, h, _: o.sobel(h), dst_kind="u8", variants=("rb1040",)),
    Op("canny", ("u8", "rgba_u8"), lambda s, d: s.canny(1.0, 30, 90, out=d), lambda o, h, _: o.canny(h, 1.0, 30, 90), dst_kind="u8"),
    Op("shen_castan", ("u8", "rgba_u8"), lambda s, d: s.shen_castan(out=d), lambda o, h, _: o.shen_castan(h), dst_kind="u8"),
)


@pytest.mark.parametrize(CASE, EDGES)
def test_edge_detectors_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- motion blurs and order statistics -------------------------------------------------------------------------------------------------
FILTERS = cases(
    Op("motion_blur_linear", U8S + ("f32",), lambda s, d: s.motion_blur_linear(0.6, 7, out=d), lambda o, h, _: o.motion_blur_linear(h, 0.6, 7)),
    Op("motion_blur_radial", U8S + ("f32",), lambda s, d: s.motion_blur_radial(0.4, 0.55, 0.5, False, out=d),
       lambda o, h, _: o.motion_blur_radial(h, 0.4, 0.55, 0.5, False)),
    Op("median_blur_1", U8S, lambda s, d: s.median_blur(1, out=d), lambda o, h, _: o.order_statistic_blur(h, 1, 0, 0.5, zg.BorderMode.mirror)),
    Op("max_blur_1", U8S, lambda s, d: s.max_blur(1, out=d), lambda o, h, _: o.order_statistic_blur(h, 1, 0, 1.0, zg.BorderMode.mirror)),
    Op("alpha_trimmed_mean_blur_2", U8S, lambda s, d: s.alpha_trimmed_mean_blur(2, 0.2, out=d),
       lambda o, h, _: o.order_statistic_blur(h, 2, 2, 0.2, zg.BorderMode.mirror)),
)


@pytest.mark.parametrize(CASE, FILTERS)
def test_motion_and_order_statistic_blurs_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- thresholds and morphology ---------------------------------------------------------------------------------------------------------
K3 = np.ones((3, 3), np.uint8)


def _otsu(s, d):
    s.threshold_otsu(out=d)


BINARY = cases(
    Op("threshold_otsu", ("u8",), _otsu, lambda o, h, _: o.threshold_otsu(h)[0]),
    Op("threshold_adaptive_mean", ("u8",), lambda s, d: s.threshold_adaptive_mean(3, 2.0, out=d), lambda o, h, _: o.threshold_adaptive_mean(h, 3, 2.0)),
    Op("dilate_binary", ("u8",), lambda s, d: s.dilate_binary(K3, 2, out=d), lambda o, h, _: o.morph(h, K3, 2, o.MORPH_DILATE), prep="binary"),
    Op("open_binary", ("u8",), lambda s, d: s.open_binary(K3, 2, out=d), lambda o, h, _: o.morph(h, K3, 2, o.MORPH_OPEN), prep="binary"),
)


@pytest.mark.parametrize(CASE, BINARY)
def test_thresholds_and_morphology_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- resize ----------------------------------------------------------------------------------------------------------------------------
DST = (96, 288)  # the destination's base shape of the resampling ops: two tiles of 256 columns (geom.hip), five of 64 (resize_planes.hip)


def resize(name, kinds, m, om, src_shape):
    return Op(name, kinds, lambda s, d: s.resize(d, m), lambda o, h, shape: o.resize(h, shape, o.method(getattr(o, om))), src_shape=src_shape, base=DST)


# geom.hip:412-414       bilinear on Image(u8): dword_rows = dst origin % 4 == 0 && dst stride % 4 == 0 (origin+1px, stride+1px flip it;
#                        origin+4B / +8B stay dword rows); ratio 1.5 (rx < 2) takes the several-rows kernel, 2.5 the one-row kernel
# resize_planes.hip:414  bilinear on Rgba(u8): x4 = ratio_x <= 1.5 && dst cols % 4 == 0 (cols-1, cols-3) && dst stride % 4 == 0 (stride+4B) && dst
#                        origin & 15 == 0 (origin+4B, +8B): ratio 1.25 has x4 to lose, ratio 3 never has it (forms 1 / 2)
RESIZE = cases(
    resize("resize_bilinear_1.5", ("u8",), I.bilinear, "BILINEAR", (144, 432)),
    resize("resize_bilinear_2.5", ("u8",), I.bilinear, "BILINEAR", (240, 720)),
    resize("resize_bilinear_1.25", ("rgba_u8",), I.bilinear, "BILINEAR", (120, 360)),
    resize("resize_bilinear_3", ("rgba_u8",), I.bilinear, "BILINEAR", (288, 864)),
    resize("resize_bicubic", ("rgba_u8", "rgba_f32"), I.bicubic, "BICUBIC", (144, 432)),
    resize("resize_catmull_rom", ("rgba_u8", "rgba_f32"), I.catmull_rom, "CATMULL_ROM", (144, 432)),
    resize("resize_lanczos", ("rgba_u8", "rgba_f32"), I.lanczos, "LANCZOS", (144, 432)),
    resize("resize_nearest", ("rgba_u8", "rgba_f32"), I.nearest, "NEAREST", (144, 432)),
    resize("resize_bilinear_up", ("rgb_u8", "f32", "rgb_f32"), I.bilinear, "BILINEAR", (61, 150)),
)


@pytest.mark.parametrize(CASE, RESIZE)
def test_resize_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- letterbox, warp, rotate, extract --------------------------------------------------------------------------------------------------
GEOM_KINDS = ("u8", "rgb_u8", "rgba_u8", "rgba_f32")
HOMOGRAPHY = zg.ProjectiveTransform([[0.96, 0.05, 3.5], [-0.04, 0.97, 2.25], [0.00011, -0.00007, 1.0]])
ANGLE, EX_ANGLE, EX_RECT = 0.3, 0.4, (30.5, 20.25, 330.5, 118.25)


def _letterbox_ref(o, h, shape):
    want = np.zeros(shape + h.shape[2:], h.dtype)
    o.letterbox(h, want, o.method(o.BILINEAR))
    return want


def warp(name, m, om):
    return Op(name, GEOM_KINDS, lambda s, d: s.warp(HOMOGRAPHY, d, m),
              lambda o, h, shape: o.warp(h, shape, o.PROJECTIVE, HOMOGRAPHY.coefficients(), o.method(getattr(o, om))), src_shape=DST, base=DST)


GEOMETRY = cases(
    Op("letterbox", GEOM_KINDS, lambda s, d: s.letterbox(d, I.bilinear), _letterbox_ref, src_shape=(120, 200), base=DST),
    warp("warp_bilinear", I.bilinear, "BILINEAR"), warp("warp_bicubic", I.bicubic, "BICUBIC"),
    Op("rotate_into", GEOM_KINDS, lambda s, d: s.rotate_into(d, ANGLE, I.bilinear, zg.BorderMode.zero, cos_sin=_cs(ANGLE)),
       lambda o, h, shape: o.rotate_into(h, np.empty(shape + h.shape[2:], h.dtype), ANGLE, o.method(o.BILINEAR), zg.BorderMode.zero),
       src_shape=(80, 240), base=DST),
    Op("extract", GEOM_KINDS, lambda s, d: s.extract(EX_RECT, EX_ANGLE, d, I.bilinear, zg.BorderMode.replicate, cos_sin=_cs(EX_ANGLE)),
       lambda o, h, shape: o.extract(h, np.empty(shape + h.shape[2:], h.dtype), EX_RECT, EX_ANGLE, o.method(o.BILINEAR), zg.BorderMode.replicate),
       src_shape=(144, 432), base=DST),
)


def _cs(angle):  # both sides get the same cos / sin values (a Zig caller passes Zig's)
    from oracle import pyoracle
    return pyoracle.cos_sin(angle)


@pytest.mark.parametrize(CASE, GEOMETRY)
def test_geometry_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- colour conversion and copy --------------------------------------------------------------------------------------------------------
def convert(name, kind, dk, src_space, dst_space, np_dtype, ch, prep=None):
    return Op(name, (kind,), lambda s, d: s.convert(dst_space, np_dtype, src_space=src_space, out=d),
              lambda o, h, _: o.convert(h, src_space, dst_space, np_dtype, ch), dst_kind=dk, prep=prep)


# convert.hip:237  Rgba(u8) / Rgb(u8) -> Xyz / Oklab / Lab f32, four pixels per lane: src origin and stride bytes % 16 (Rgba) or % 4 (Rgb), the
#                  12-byte destination pixel's origin % 16 and stride x 12 % 16 (origin+4B, +8B, stride+4B on rgb_f32)
# convert.hip:321  the way back, Lab f32 -> Rgba(u8): the same terms with the sides swapped
# convert.hip:411  Image(u8) -> Rgba(u8), four pixels per lane: src cols % 4 (cols-1, cols-3), src stride % 4 and origin & 3 (stride+1px,
#                  origin+1px), dst stride % 4 (stride+4B) and origin & 15 (origin+4B, +8B)
# resize_convert: the fused Rgba(u8) bilinear -> Oklab kernel writes the same 12-byte pixels.
COLOUR = cases(
    convert("convert_gray_to_rgba", "u8", "rgba_u8", zg.CS_GRAY, zg.CS_RGBA, np.uint8, 4),
    convert("convert_rgba_to_oklab", "rgba_u8", "rgb_f32", zg.CS_RGBA, zg.CS_OKLAB, np.float32, 3),
    convert("convert_rgb_to_xyz", "rgb_u8", "rgb_f32", zg.CS_RGB, zg.CS_XYZ, np.float32, 3),
    convert("convert_lab_to_rgba", "rgb_f32", "rgba_u8", zg.CS_LAB, zg.CS_RGBA, np.uint8, 4, prep="lab"),
    Op("resize_convert_oklab", ("rgba_u8",), lambda s, d: s.resize_convert(d, zg.CS_OKLAB),
       lambda o, h, shape: o.convert(o.resize(h, shape, o.method(o.BILINEAR)), o.CS_RGBA, o.CS_OKLAB, np.float32, 3),
       dst_kind="rgb_f32", src_shape=(144, 432), base=DST),
    Op("copy", ALL, lambda s, d: s.copy(d), lambda o, h, _: h.copy()),
)


@pytest.mark.parametrize(CASE, COLOUR)
def test_convert_and_copy_into_views(oracle, op, kind, dk, variant, sp, dp):
    run_case(oracle, op, kind, dk, variant, sp, dp)


# ---- in place on a view ----------------------------------------------------------------------------------------------------------------
def _pixel(kind, v):
    ch = V.LAYOUT[kind][1]
    v = np.float32(v) / np.float32(255) if kind.endswith("f32") else v
    return v if ch == 1 else [v] * ch


INSERT_1TO1, INSERT_ROT, INSERT_ANGLE = (30, 20, 90, 60), (100.5, 50.25, 220.5, 130.75), 0.35


def _insert(rect, angle, blend):
    def call(img, oracle):
        img.insert(zg.Image(torch.from_numpy(host_of(oracle, "rgba_u8", (40, 60), seed=9).copy()).cuda()), rect, angle, I.bilinear, blend, cos_sin=_cs(angle))

    def ref(o, a):
        return o.insert(a, host_of(o, "rgba_u8", (40, 60), seed=9), rect, angle, o.method(o.BILINEAR), blend)
    return call, ref


# name -> (kinds, call(image, oracle), ref(oracle, a copy of the host pixels) -> the pixels after the call)
IN_PLACE = {
    "fill": (ALL, lambda k: (lambda img, o: img.fill(_pixel(k, 77))), lambda k: (lambda o, a: o.fill(a, _pixel(k, 77)))),
    "set_border": (ALL, lambda k: (lambda img, o: img.set_border((5, 7, img.cols - 9, img.rows - 4), _pixel(k, 200))),
                   lambda k: (lambda o, a: o.set_border(a, (5, 7, a.shape[1] - 9, a.shape[0] - 4), _pixel(k, 200)))),
    "invert": (U8S + ("rgba_f32",), lambda k: (lambda img, o: img.invert()), lambda k: (lambda o, a: o.invert(a))),
    "flip_left_right": (ALL, lambda k: (lambda img, o: img.flip_left_right()), lambda k: (lambda o, a: o.flip_left_right(a))),
    "flip_top_bottom": (ALL, lambda k: (lambda img, o: img.flip_top_bottom()), lambda k: (lambda o, a: o.flip_top_bottom(a))),
    "autocontrast": (U8S, lambda k: (lambda img, o: img.autocontrast(0.02)), lambda k: (lambda o, a: o.autocontrast(a, 0.02))),
    "equalize": (U8S, lambda k: (lambda img, o: img.equalize()), lambda k: (lambda o, a: o.equalize(a))),
    "insert_1to1_none": (("rgba_u8",), lambda k: _insert(INSERT_1TO1, 0.0, zg.Blending.none)[0], lambda k: _insert(INSERT_1TO1, 0.0, zg.Blending.none)[1]),
    "insert_1to1_normal": (("rgba_u8",), lambda k: _insert(INSERT_1TO1, 0.0, zg.Blending.normal)[0], lambda k: _insert(INSERT_1TO1, 0.0, zg.Blending.normal)[1]),
    "insert_rotated_none": (("rgba_u8",), lambda k: _insert(INSERT_ROT, INSERT_ANGLE, zg.Blending.none)[0],
                            lambda k: _insert(INSERT_ROT, INSERT_ANGLE, zg.Blending.none)[1]),
    "insert_rotated_multiply": (("rgba_u8",), lambda k: _insert(INSERT_ROT, INSERT_ANGLE, zg.Blending.multiply)[0],
                                lambda k: _insert(INSERT_ROT, INSERT_ANGLE, zg.Blending.multiply)[1]),
}


def _in_place_cases():
    out = []
    for name, (kinds, _, _) in IN_PLACE.items():
        for kind in kinds:
            for pl in V.placements(kind):
                out.append(pytest.param(name, kind, "base", pl, id=f"{name}-{kind}-base-{pl}"))
            for v in tuple(SHAPE_DELTAS)[1:]:
                out.append(pytest.param(name, kind, v, "aligned", id=f"{name}-{kind}-{v}-aligned"))
    return out


@pytest.mark.parametrize("name,kind,variant,placement", _in_place_cases())
def test_in_place_ops_on_a_view(oracle, name, kind, variant, placement):
    _, call, ref = IN_PLACE[name]
    c = shaped(kind, BASE, variant, placement)
    host = host_of(oracle, kind, (c.rows, c.cols))
    c.put(host)
    what = f"{name} {kind} {variant} {placement} {c.facts()}"
    call(kind)(c.image(), oracle)
    want = want_of((name, kind, host.shape), lambda: ref(kind)(oracle, host.copy()))
    assert_bits_equal(c.take(what), want, what)


@pytest.mark.parametrize("side", ("source", "destination"))
@pytest.mark.parametrize("shift", (4, 8))
def test_rgba_f32_off_its_16_byte_alignment_is_refused(oracle, side, shift):
    """An Rgba(f32) pixel moves with one 16-byte instruction, so check_image (zg_runtime.cpp) refuses a first pixel that is not 16-byte
    aligned: the origin+4B / origin+8B layouts do not exist for this type. The refusal comes before any launch: nothing is written."""
    host = host_of(oracle, "rgba_f32", (64, 64))
    canvases = [V.Canvas("rgba_f32", 64, 64, 16, 2, 16, 2, shift_bytes=shift if side == s else 0) for s in ("source", "destination")]
    assert [c.facts()["origin%16"] for c in canvases] == [shift if side == s else 0 for s in ("source", "destination")]
    canvases[0].put(host)
    with pytest.raises(zg.InvalidArgument, match="16-byte aligned"):
        canvases[0].image().gaussian_blur(0.6, out=canvases[1].image())
    assert canvases[1].stray() is None and bool((canvases[1].view.view(torch.uint8) == V.SENTINEL).all())
    assert_bits_equal(canvases[0].take("refused"), host, "refused call")


# ---- the pyramid's levels as views -----------------------------------------------------------------------------------------------------
# pyramid_tile.hip:320  k_pyr_tile takes an Image(u8) source whose stride % 4 == 0 and origin & 3 == 0 (stride+1px, origin+1px leave it for the
#                       round-5 route); its levels are written at any origin and stride.
def _pyramid_cases():
    out = [("aligned", "aligned")]
    for pl in V.placements("u8")[1:]:
        out += [(pl, pl), ("aligned", pl), (pl, "aligned")]
    return out


@pytest.mark.parametrize("sp,dp", _pyramid_cases())
def test_pyramid_levels_into_views(oracle, sp, dp):
    rows, cols = 150, 271
    host = host_of(oracle, "u8", (rows, cols), seed=12)
    want = want_of(("pyramid", rows, cols), lambda: oracle.pyramid(host, 3, 1.5, 1.6))
    assert len(want) == 3
    src = V.place("u8", rows, cols, sp).put(host)
    levels = [V.place("u8", w.shape[0], w.shape[1], dp) for w in want[1:]]
    lib = zg.lib()
    sigmas = []
    for i, w in enumerate(want[1:], 1):
        r, c, sigma = C.c_uint32(), C.c_uint32(), C.c_float()
        L.check(lib.zg_pyramid_level(rows, cols, C.c_float(lib.zg_pyramid_scale(C.c_float(1.5), i)), C.c_float(1.6), C.byref(r), C.byref(c), C.byref(sigma)))
        assert (r.value, c.value) == w.shape
        sigmas.append(sigma.value)
    img = src.image()
    sd, descs = img._desc(), (L.ZgImage * 2)(*[l.image()._desc() for l in levels])
    L.check(lib.zg_pyramid_build(C.byref(sd), descs, (C.c_float * 2)(*sigmas), 2, img._stream()))
    for i, (level, w) in enumerate(zip(levels, want[1:]), 1):
        what = f"pyramid level {i}, {sp}>{dp}"
        assert_bits_equal(level.take(what), w, what)
    assert_bits_equal(src.take("pyramid source"), host, "pyramid: the source changed")


# ---- contiguous buffers inside a sentinel frame: the batched pipeline into out=, isef_smooth ----------------------------------------------------------------------------------------------------
Batch = V.Framed  # n contiguous frames inside a sentinel frame (Pipeline.run takes contiguous batches: the frame pitch follows from the shape)


@pytest.mark.parametrize("kind,rows,cols,pitch_is_16", [("rgba_u8", 34, 268, True), ("rgb_u8", 33, 267, False)])
def test_pipeline_into_out(oracle, kind, rows, cols, pitch_is_16):
    """[blur 1.0, resize half, edges sobel] over 3 frames into out=, the batches contiguous inside sentinel frames (Pipeline.run takes
    contiguous batches, so the frame pitch follows from the shape). Rgba(u8) 34 x 268: frame pitches of 36448, 9112 and 2278 bytes, the first a
    multiple of 16; Rgb(u8) 33 x 267: odd rows, pitches of 26433, 6384 and 2128 bytes, every frame-pitch term (src_frame % 16, dst_frame % 16
    in try_sep_stream, try_sep_bytes2_frames and try_sobel_stream) on its slow side. The down2 store forms are reached by
    test_blur_and_half_resize_into_out below (268 x 4 row bytes are no multiple of 32)."""
    ch = V.LAYOUT[kind][1]
    n, orows, ocols = 3, rows // 2, cols // 2
    assert (rows * cols * ch % 16 == 0) == pitch_is_16 and (rows % 2 == 0) == pitch_is_16
    host = np.stack([host_of(oracle, kind, (rows, cols), seed=20 + f) for f in range(n)])
    src, out = Batch((n, rows, cols, ch)), Batch((n, orows, ocols, ch))
    src.frames.copy_(torch.from_numpy(np.array(host)).cuda())
    steps = [zg.Step.gaussian_blur(1.0), zg.Step.resize(orows, ocols), zg.Step.edges_sobel()]
    got = zg.Pipeline(steps).run(src.frames, out=out.frames)
    assert got.data_ptr() == out.frames.data_ptr()
    space = oracle.CS_RGBA if ch == 4 else oracle.CS_RGB
    want = []
    for f in host:
        small = oracle.resize(oracle.gaussian_blur(f, 1.0), (orows, ocols), oracle.method(oracle.BILINEAR))
        grey = oracle.sobel(oracle.convert(small, space, oracle.CS_GRAY, np.uint8, 1))
        want.append(oracle.convert(grey, oracle.CS_GRAY, space, np.uint8, ch))
    assert_bits_equal(out.take(f"pipeline {kind} out"), np.stack(want), f"pipeline {kind}")
    assert_bits_equal(src.take(f"pipeline {kind} frames"), host, f"pipeline {kind}: the frames changed")


# rows, cols, source shift, destination shift (bytes) -> the route of gaussianBlur + bilinear resize to half of Rgba(u8) frames. Both entries
# ask one list (batch.hip's gaussian_u8_routes) for the blur + 2:1 form, rb being the row bytes:
#   try_sep_stream's down2 form:       rows % 2, rb % 32, dst pitch % 8, dst_frame % 8, dst & 7 (after rb % 16, src_frame % 16, src & 15)
#   try_sep_rgba8_batch's down2 form:  rows % 2, cols % 4, dst stride % 2 pixels, dst_frame % 8, dst & 7 (after src_frame % 16, src & 15): what
#                                      is tried when the stream kernel refuses
# A half-size resize is one only when rows == 2 x out rows, so rows % 2 cannot be flipped inside either predicate: an odd-rows batch
# is no half-size resize and takes the blur-then-resize route, which the 33-row case pins.
HALF_CASES = {
    "stream_down2": (32, 272, 0, 0),     # rb = 1088: % 32 == 0, every term on its fast side
    "rgba8_down2": (34, 268, 0, 0),      # rb = 1072: % 32 == 16, the stream form refuses; cols % 4 == 0, so k_sep_rgba8's down2 form takes it
    "cols%4": (34, 270, 0, 0),           # rb % 16 == 8 and cols % 4 == 2: both refuse
    "odd_rows": (33, 272, 0, 0),         # 33 -> 16 rows: not a half-size resize
    "src+4B": (32, 272, 4, 0),           # src & 15
    "src+8B": (32, 272, 8, 0),
    "dst+4B": (32, 272, 0, 4),           # dst & 7: both down2 forms refuse
    "dst+8B": (32, 272, 0, 8),           # dst & 7 == 0, dst & 15 != 0: the down2 forms store 8 bytes, still admitted
    "dst+4B_rgba8": (34, 268, 0, 4),
}


@pytest.mark.parametrize("entry", ("pipeline", "batch_blur_resize"))
@pytest.mark.parametrize("case", HALF_CASES)
def test_blur_and_half_resize_into_out(oracle, case, entry):
    rows, cols, src_shift, dst_shift = HALF_CASES[case]
    n, orows, ocols = 3, rows // 2, cols // 2
    host = np.stack([host_of(oracle, "rgba_u8", (rows, cols), seed=30 + f) for f in range(n)])
    src, out = Batch((n, rows, cols, 4), 512 + src_shift), Batch((n, orows, ocols, 4), 512 + dst_shift)
    assert src.frames.data_ptr() % 16 == src_shift and out.frames.data_ptr() % 16 == dst_shift
    assert (case in ("stream_down2", "src+4B", "src+8B", "dst+4B", "dst+8B")) == (rows % 2 == 0 and cols * 4 % 32 == 0)
    src.frames.copy_(torch.from_numpy(np.array(host)).cuda())
    if entry == "pipeline":
        zg.Pipeline([zg.Step.gaussian_blur(1.0), zg.Step.resize(orows, ocols)]).run(src.frames, out=out.frames)
    else:
        m = I.bilinear._c()
        rc = zg.lib().zg_batch_blur_resize(C.c_void_p(src.frames.data_ptr()), n, rows, cols, L.PIXEL_RGBA_U8, C.c_float(1.0), C.c_void_p(out.frames.data_ptr()),
                                           orows, ocols, C.byref(m), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, zg.lib().zg_last_error()
    want = want_of(("half", rows, cols), lambda: np.stack([oracle.resize(oracle.gaussian_blur(f, 1.0), (orows, ocols), oracle.method(oracle.BILINEAR)) for f in host]))
    what = f"{entry} blur 1.0 + half resize, {case}"
    assert_bits_equal(out.take(what), want, what)
    assert_bits_equal(src.take(what), host, what + ": the frames changed")


@pytest.mark.parametrize("dst_shift", (0, 4, 8))
@pytest.mark.parametrize("src_shift", (0, 4, 8))
@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_isef_smooth_planes_at_every_origin(oracle, kind, src_shift, dst_shift):
    """isef_smooth takes contiguous planes only (isef.hip, zg_isef_smooth: a strided view is refused as unsupported, checked last), so its
    planes sit contiguous inside sentinel frames with the origin moved by one and two dwords: the u8 route's predicate is
    source origin & 15 and destination origin & 15 (isef.hip, "isef_2d also wants a 16-byte aligned destination")."""
    rows, cols = 272, 272
    host = host_of(oracle, kind, (rows, cols), seed=3)
    src = Batch((rows, cols), 512 + src_shift, torch.uint8 if kind == "u8" else torch.float32)
    dst = Batch((rows, cols), 512 + dst_shift, torch.float32)
    assert src.frames.data_ptr() % 16 == src_shift and dst.frames.data_ptr() % 16 == dst_shift
    src.frames.copy_(torch.from_numpy(np.array(host)).cuda())
    zg.Image(src.frames).isef_smooth(0.8, out=zg.Image(dst.frames))
    what = f"isef_smooth {kind} origin+{src_shift}B > origin+{dst_shift}B"
    want = want_of(("isef", kind), lambda: oracle.isef_plane(host.astype(np.float32), 0.8))
    assert_bits_equal(dst.take(what), want, what)
    assert_bits_equal(src.take(what), host, what + ": the source changed")
    view = V.place("f32", rows, cols, "aligned")
    with pytest.raises(zg.ZignalError) as e:
        zg.Image(src.frames).isef_smooth(0.8, out=view.image())
    assert e.value.status == L.ERR_UNSUPPORTED
    view.take(what + ", refused view")


def test_host_band_layer_aliased(oracle):
    """zg_runtime.cpp:438 "an in-place call (or any overlap) would have later bands read rows that earlier bands already overwrote": host
    images of 24 MiB and more go band by band unless source and destination share bytes; then the whole-frame path runs, which uploads the
    source before anything comes back. In place and into a view of the same host frame 3 rows down and 5 pixels right, on an unaligned view."""
    rows, cols = 1800, 1901
    assert 2 * rows * cols * 4 >= 24 << 20
    host = host_of(oracle, "rgba_u8", (rows, cols), seed=6)
    want = oracle.gaussian_blur(host, 0.6)
    for how in ("same_view", "shifted_3_rows_5_px"):
        frame = np.full((rows + 7, cols + 40, 4), V.SENTINEL, np.uint8)
        src = frame[2:2 + rows, 17:17 + cols]
        src[...] = host
        top, left = (2, 17) if how == "same_view" else (5, 22)
        dst = frame[top:top + rows, left:left + cols]
        zg.Image(src).gaussian_blur(0.6, out=zg.Image(dst))
        assert_bits_equal(dst, want, f"host gaussian_blur {how}")
        outside = np.ones(frame.shape[:2], bool)
        outside[2:2 + rows, 17:17 + cols] = False
        outside[top:top + rows, left:left + cols] = False
        assert np.all(frame[outside] == V.SENTINEL), f"host gaussian_blur {how}: a byte outside both views was written"


# ---- aliased destinations --------------------------------------------------------------------------------------------------------------
# The sources say src may alias dst for these:
#   box_blur.hip:7         "All SAT planes are complete before any output is written, so src may alias dst as in the reference."
#   box_fused.hip:864      "the in-place call (examples/src/face_alignment.zig:95): a strip's outputs would be read by its neighbours' chains,
#                           so the source is copied first"
#   binary.hip:154-160     "`iterations` applications of one operation from src to dst through two scratch planes (src may alias dst)" ... "if dst
#                           shares bytes with the buffer being read (in place or a shifted view of it, single step) go through scratch first"
#   order_stat.hip:114     "in place, or a destination view that shares bytes with the source: other workgroups would read pixels this one has
#                           already replaced"
#   zg_runtime.cpp:438     "an in-place call (or any overlap) would have later bands read rows that earlier bands already overwrote" (the host
#                           band layer: it steps aside and the whole-frame path runs; host images, so no device view is involved)
#   edges.hip (sobel_frames) "in place on an Image(u8), or a destination view that shares bytes with the source: a lane reads its neighbours'
#                           pixels, so the source is copied first"; canny and shen_castan read the source into scratch planes before any stage
#                           writes the destination.
# (a) out = the same view; (b) out = a view of the same canvas 3 rows down and 5 pixels right. Both equal the oracle run on a copy of the input:
# no op of this list answers a partial overlap with InvalidArgument, each does what its exact-alias path does (the source is read, or copied
# aside, before the first output is written).
K1 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
ALIAS_OPS = {  # name -> (kind, call(src, dst), ref(oracle, host), prep, behaviour on a partial overlap)
    "box_blur_2": ("u8", lambda s, d: s.box_blur(2, out=d), lambda o, h: o.box_blur(h, 2), None, "oracle"),
    "box_blur_2_rgba": ("rgba_u8", lambda s, d: s.box_blur(2, out=d), lambda o, h: o.box_blur(h, 2), None, "oracle"),
    "box_blur_5": ("rgb_u8", lambda s, d: s.box_blur(5, out=d), lambda o, h: o.box_blur(h, 5), None, "oracle"),
    "sharpen_2": ("u8", lambda s, d: s.sharpen(2, out=d), lambda o, h: o.sharpen(h, 2), None, "oracle"),
    "dilate_binary_x1": ("u8", lambda s, d: s.dilate_binary(K1, 1, out=d), lambda o, h: o.morph(h, K1, 1, o.MORPH_DILATE), "binary", "oracle"),
    "dilate_binary_x2": ("u8", lambda s, d: s.dilate_binary(K3, 2, out=d), lambda o, h: o.morph(h, K3, 2, o.MORPH_DILATE), "binary", "oracle"),
    "open_binary_x1": ("u8", lambda s, d: s.open_binary(K3, 1, out=d), lambda o, h: o.morph(h, K3, 1, o.MORPH_OPEN), "binary", "oracle"),
    "open_binary_x2": ("u8", lambda s, d: s.open_binary(K3, 2, out=d), lambda o, h: o.morph(h, K3, 2, o.MORPH_OPEN), "binary", "oracle"),
    "median_blur_1": ("u8", lambda s, d: s.median_blur(1, out=d), lambda o, h: o.order_statistic_blur(h, 1, 0, 0.5, zg.BorderMode.mirror), None, "oracle"),
    "max_blur_1": ("rgba_u8", lambda s, d: s.max_blur(1, out=d), lambda o, h: o.order_statistic_blur(h, 1, 0, 1.0, zg.BorderMode.mirror), None, "oracle"),
    "alpha_trimmed_mean_blur_2": ("rgb_u8", lambda s, d: s.alpha_trimmed_mean_blur(2, 0.2, out=d),
                                  lambda o, h: o.order_statistic_blur(h, 2, 2, 0.2, zg.BorderMode.mirror), None, "oracle"),
    "sobel": ("u8", lambda s, d: s.sobel(out=d), lambda o, h: o.sobel(h), None, "oracle"),
    "canny": ("u8", lambda s, d: s.canny(1.0, 30, 90, out=d), lambda o, h: o.canny(h, 1.0, 30, 90), None, "oracle"),
    "shen_castan": ("u8", lambda s, d: s.shen_castan(out=d), lambda o, h: o.shen_castan(h), None, "oracle"),
}
ALIAS_ROWS, ALIAS_COLS = 272, 267  # an unaligned view: origin, stride bytes and row bytes all off their 16-byte multiples (asserted)


@pytest.mark.parametrize("how", ("same_view", "shifted_3_rows_5_px"))
@pytest.mark.parametrize("name", ALIAS_OPS)
def test_aliased_destination(oracle, name, how):
    kind, call, ref, prep, partial = ALIAS_OPS[name]
    canvas = V.Canvas(kind, ALIAS_ROWS + 3, ALIAS_COLS + 5, 17, 2, 18, 2)
    assert canvas.facts()["origin%16"] != 0 and canvas.facts()["stride_bytes%16"] != 0 and ALIAS_COLS * V.psize(kind) % 16 != 0
    host = host_of(oracle, kind, (ALIAS_ROWS, ALIAS_COLS), seed=5, prep=prep)
    want = want_of(("alias", name), lambda: ref(oracle, host.copy()))
    src_rect, dst_rect = (0, 0, ALIAS_COLS, ALIAS_ROWS), (5, 3, ALIAS_COLS + 5, ALIAS_ROWS + 3)
    src = canvas.image(src_rect)
    src.data.copy_(torch.from_numpy(np.array(host)).cuda())
    dst = src if how == "same_view" else canvas.image(dst_rect)
    what = f"{name} {kind} {how}"
    try:
        call(src, dst)
    except zg.InvalidArgument:
        assert how != "same_view" and partial == "raises", f"{what}: the call was rejected"
        canvas.take(what)
        return
    assert how == "same_view" or partial == "oracle", f"{what}: the table says this call is rejected"
    canvas.take(what)  # nothing outside the canvas's own view (which holds both rectangles)
    torch.cuda.synchronize()
    assert_bits_equal(dst.data.cpu().numpy(), want, what)

"""The f32 routes on negative, tiny, huge and non-finite pixels (tests/domain_frames.py), against the oracle with NaN compared as a class
(tests/util.py: assert_bits_equal_nan_class). tests/util.py: synth gives every other f32 test frame non-negative multiples of 2^-24 below 1.

One test per (op, pixel type). Inside it every frame name runs at two shapes:
  48 x 272  rows >= 16, cols >= 256, cols % 16 == 0, contiguous and aligned: the tile, x4 and long-tap f32 kernels take it
  47 x 67   ragged: the general kernels take it
The ops, with their device call and their oracle call, are the Op objects of tests/test_gpu_dst_views.py (or made by its factories); only
the frames differ. Integral-image ops (box_blur, sharpen) take huge_sat and nonfinite_corner in place of huge and nonfinite: an f32 summed
area table overflows on `huge` and carries one infinity into every sum below and to the right of it.

CASES below is a plain table: tests/test_domain_frames.py runs the oracle alone over it and holds every expected output to the caps and
classes that keep a GPU case from passing by being empty (at most 10 % NaN, a non-finite value wherever the frame has one, subnormals on
`tiny`, the signs of zero on `negzero`)."""
import numpy as np
import pytest

import zignal_amd as zg
from tests import domain_frames as DF
from tests import metrics_ref as R
from tests import test_gpu_dst_views as D
from tests import views as V
from tests.util import assert_bits_equal_nan_class

torch = pytest.importorskip("torch")

I = zg.Interpolation
F32S = ("f32", "rgb_f32", "rgba_f32")
SHAPES = ((48, 272), (47, 67))
FRAMES = ("signed", "tiny", "huge", "negzero", "nonfinite")
INTEGRAL_FRAMES = ("signed", "tiny", "huge_sat", "negzero", "nonfinite_corner")
Op = D.Op

# the Op objects of the destination-view tables, by name
_TABLE = {p.values[0].name: p.values[0] for p in D.SEPARABLE + D.CONV2D + D.BOX + D.EDGES + D.FILTERS + D.RESIZE + D.GEOMETRY}


def same(rows, cols):
    return rows, cols


class Case:
    """op: a tests/test_gpu_dst_views.py Op (call(src_image, dst_image), ref(oracle, host, dst_shape)); kinds: the f32 source types it runs on;
    dst_shape(rows, cols) of the source -> the destination's; frames: the frame names; linear: a linear filter whose output on `tiny` stays
    tiny (the subnormal condition of tests/test_domain_frames.py applies)."""

    def __init__(self, op, kinds, dst_shape=same, frames=FRAMES, linear=False):
        assert all(k in F32S for k in kinds), (op.name, kinds)
        self.op, self.kinds, self.dst_shape, self.frames, self.linear = op, tuple(kinds), dst_shape, tuple(frames), linear
        self.name = op.name

    def dst_kind(self, kind):
        dk = self.op.dst_kind
        return dk(kind) if callable(dk) else (dk or kind)


def table(name, kinds=None, **kw):
    """The named Op of tests/test_gpu_dst_views.py on its own f32 kinds, or on `kinds`. An Op restricted to u8 kinds has no case."""
    op = _TABLE[name]
    kinds = tuple(k for k in op.kinds if k in F32S) if kinds is None else kinds
    return [Case(op, kinds, **kw)] if kinds else []


# ---- separable convolutions ------------------------------------------------------------------------------------------------------------
# 48 x 272 (contiguous; run_device asserts the 16-byte origins):
#   conv_sep_tile_f32.hip:233-245  Image(f32), 5 and 7 taps without a negligible tap (gaussian_blur 0.6 / 1.0, K5): cols % 4 == 0, strides % 4 == 0,
#                                  origins & 15 == 0, cols >= 64, rows >= 16, row bytes % 1024 != 16 -> k_sep_tile_f32
#   conv_sep_f32x4.hip:165-167     Image(f32), 9 taps (ZERO_ENDS: its skip masks keep it out of the tile kernel and of the long-tap one): cols % 4,
#                                  strides % 4, origins & 15, cols >= 64 -> k_sep_f32x4
#   conv_sep_f32long.hip:215-218   every f32 type, 13 and 17 taps (K13, gaussian_blur 2.5; conv_separable.hip:523 sends equal odd counts up to 9
#                                  elsewhere): row floats % 4 == 0 and >= 256, pitches and origins % 16, no tap below 1e-10 -> k_rows_f32 + k_cols_f32
#   conv_separable.hip:432-440     Rgb(f32) / Rgba(f32), 5 to 9 taps: k_sep_fused, which has no alignment term
# 47 x 67: cols % 4 != 0 refuses the tile and x4 kernels: Image(f32) takes k_sep_fused up to 13 taps and k_sep_h + k_sep_v at 17; Rgb(f32) has
# 201 row floats (< 256, % 4 != 0): k_sep_fused up to 9 taps, k_sep_h + k_sep_v above; Rgba(f32) has 268 row floats: k_sep_fused up to 9 taps and
# the long-tap kernels again at 13 and 17.
# conv_separable.hip:13 / oracle/conv.c:191,215: an interior pixel skips a tap with |k| < 1e-10, a border pixel does not. ZERO_ENDS has two
# outer taps of exactly 0.0 and runs under BorderMode.replicate, where the 0.0 tap of the first four columns and rows lands on pixel 0: nonfinite's
# corner +inf makes inf * 0 = NaN there, and its centre -inf, which only interior pixels reach, makes none.
K5, K13 = D.K5, D.K13
K5X3 = (K5 * np.float32(3)).astype(np.float32)  # taps that sum to 3: on `huge` the sums overflow to infinity, in the reference too
ZERO_ENDS = np.array([0.0, 0.1, 0.2, 0.15, 0.1, 0.15, 0.2, 0.1, 0.0], np.float32)
B = zg.BorderMode


def sep(name, k, border, frames=FRAMES):
    return Case(Op(name, F32S, lambda s, d: s.convolve_separable(k, k, border, out=d), lambda o, h, _: o.conv_separable(h, k, k, border)),
                F32S, frames=frames, linear=True)


SEPARABLE = (
    table("gaussian_blur_0.6", linear=True) + table("gaussian_blur_1.0", linear=True) + table("gaussian_blur_2.5", linear=True)
    + table("convolve_separable_5", F32S, linear=True) + table("convolve_separable_13", F32S, linear=True)
    + [sep("convolve_separable_5_zero_border", K5, B.zero), sep("convolve_separable_9_zero_end_taps", ZERO_ENDS, B.replicate),
       sep("convolve_separable_5_times_3", K5X3, B.mirror, frames=("huge",))]
)

# ---- 2-D convolution -------------------------------------------------------------------------------------------------------------------
# Every f32 type and shape: k_conv2d (conv2d.hip), which has no alignment term (conv2d_stream.hip:294 takes the u8 types only).
CONV2D = table("convolve_3x3", F32S, linear=True) + table("convolve_5x5", F32S, linear=True) + table("convolve_7x7", F32S, linear=True)

# ---- box blur and sharpen: the integral-image ops ------------------------------------------------------------------------------------------
# box_blur.hip:741 (k_box_direct), box_fused.hip:860 and the exact-row scans (box_blur.hip:621) take u8 pixels only. Every f32 type, at both
# shapes: k_sat_rows + k_sat_cols build the f32 summed-area planes (box_blur.hip:640-641) and k_box_mean takes the four-corner difference and
# divides by the area through v_rcp (box_blur.hip:126-128).
BOX = table("box_blur_2", frames=INTEGRAL_FRAMES, linear=True) + table("sharpen_2", F32S, frames=INTEGRAL_FRAMES)

# ---- resize ----------------------------------------------------------------------------------------------------------------------------
# geom.hip:412-414 and resize_planes.hip:414 take u8 types; every f32 type goes through k_geom (geom.hip:94) and zg_sample.h's interpolators at
# both shapes. down: 48 x 272 -> 31 x 181 (47 x 67 -> 30 x 43); up: x 2; up3: x 3, where destination pixel 3 k + 1 samples source pixel k exactly
# ((d + 0.5) / 3 - 0.5 is an integer): every other tap of that sample has weight zero, next to an infinity that is inf * 0.
METHODS = (("nearest", I.nearest, "NEAREST"), ("bilinear", I.bilinear, "BILINEAR"), ("bicubic", I.bicubic, "BICUBIC"),
           ("catmull_rom", I.catmull_rom, "CATMULL_ROM"), ("mitchell", I.mitchell_default, "MITCHELL"), ("lanczos", I.lanczos, "LANCZOS"))
SCALES = {"down": lambda r, c: (r * 31 // 48, c * 181 // 272), "up": lambda r, c: (2 * r, 2 * c), "up3": lambda r, c: (3 * r, 3 * c)}
assert SCALES["down"](48, 272) == (31, 181) and SCALES["up"](48, 272) == (96, 544)
RESIZE = [Case(D.resize(f"resize_{mn}_{sn}", F32S, m, om, None), F32S, dst_shape=scale, linear=True) for mn, m, om in METHODS for sn, scale in SCALES.items()]

# ---- letterbox, warp, rotate, extract, insert --------------------------------------------------------------------------------------------
# k_geom (geom.hip:94) for letterbox, warp, rotate and extract, k_insert / k_insert_assign (geom.hip:665,703) for insert, all through zg_sample.h; the destination of letterbox is a quarter taller and a tenth wider
# than the source, so the content is a true resize with bars above and below.
INSERT_SRC = (13, 21)
INSERT_1TO1, INSERT_ROT, INSERT_ANGLE = (10, 8, 31, 21), (20.5, 10.25, 52.5, 38.75), 0.35


def insert(name, rect, angle, kinds):
    """Image.insert is in place: the destination is a copy of the frame, the inserted image the frame's own top-left 13 x 21 pixels (with
    nonfinite's corner special)."""
    def call(s, d):
        s.copy(d)
        d.insert(s.view((0, 0, INSERT_SRC[1], INSERT_SRC[0])), rect, angle, I.bilinear, zg.Blending.none, cos_sin=D._cs(angle))

    def ref(o, h, _):
        return o.insert(h.copy(), np.ascontiguousarray(h[:INSERT_SRC[0], :INSERT_SRC[1]]), rect, angle, o.method(o.BILINEAR), 0)

    return Case(Op(name, kinds, call, ref), kinds)


def insert_into(dk, how, rect_of, angle):
    """An f32 frame inserted whole into a u8 destination of its own shape (1:1, or shrunk and rotated): assignPixel converts every sample
    with convertColor (convert_px, zg_blend.h, in k_insert_assign), the clamp into a byte with NaN -> 255 included. The destination starts
    as the sentinel byte on both sides."""
    def call(s, d):
        d.insert(s, rect_of(s.rows, s.cols), angle, I.bilinear, zg.Blending.none, cos_sin=D._cs(angle))

    def ref(o, h, shape):
        dst = np.full(tuple(shape) + {"u8": (), "rgb_u8": (3,), "rgba_u8": (4,)}[dk], V.SENTINEL, np.uint8)
        return o.insert(dst, h, rect_of(h.shape[0], h.shape[1]), angle, o.method(o.BILINEAR), 0)

    return Case(Op(f"insert_into_{dk}_{how}", F32S, call, ref, dst_kind=dk), F32S)


INSERT_MIXED = [insert_into(dk, how, rect_of, angle) for dk in ("u8", "rgb_u8", "rgba_u8")
                for how, rect_of, angle in (("1to1", lambda r, c: (0, 0, c, r), 0.0), ("rotated", lambda r, c: (5.5, 4.25, c - 6.5, r - 3.75), 0.1))]
GEOM_F32 = tuple(k for k in D.GEOM_KINDS if k in F32S)
GEOMETRY = (
    table("letterbox", dst_shape=lambda r, c: (r + r // 4, c + c // 10)) + table("warp_bilinear") + table("warp_bicubic")
    + table("rotate_into") + table("extract")
    + [insert("insert_1to1", INSERT_1TO1, 0.0, ("f32",) + GEOM_F32), insert("insert_rotated", INSERT_ROT, INSERT_ANGLE, ("f32",) + GEOM_F32)]
    + INSERT_MIXED
)

# ---- motion blurs, sobel, the f32 -> u8 conversions ---------------------------------------------------------------------------------------
# motion.hip: k_motion_linear / k_motion_radial on every type, no alignment term; :59 is the u8 store, the f32 types store the quotient.
# edges.hip: k_sobel on every f32 type (sobel_stream.hip:229-232 takes the u8 types). An Image(f32) is its own grey plane: the reference multiplies
# every tap, the zero ones too (convolution.zig:158-169), so an infinity under a zero weight is a NaN and the byte 255 (sobel_3x3<true>). Rgb(f32)
# and Rgba(f32) go through a clamped grey byte first (sobel_gray), where a NaN clamps to 255. The magnitude is clamped into a byte (k_sobel).
# convert.hip: k_convert's f32 -> u8 branch (unit_to_u8, convert.hip:30-31) at every shape; :237 / :321 / :411 are u8-source or Lab routes.
# canny / shen_castan on Image(f32): k_canny_gray<Image(f32)> (canny_gray, edges.hip) clamps every pixel into a grey byte in f64 first, NaN -> 255
# (color.zig:114-118); everything after it works on bytes, which is why k_canny_nms keeps sobel's short form.
FILTERS = (table("motion_blur_linear", F32S, linear=True) + table("motion_blur_radial", F32S, linear=True) + table("sobel", F32S)
           + table("canny", ("f32",)) + table("shen_castan", ("f32",)))
SPACE = {"f32": zg.CS_GRAY, "rgb_f32": zg.CS_RGB, "rgba_f32": zg.CS_RGBA}
U8_DST = (("u8", zg.CS_GRAY, 1), ("rgb_u8", zg.CS_RGB, 3), ("rgba_u8", zg.CS_RGBA, 4))
CONVERT = [Case(D.convert(f"convert_{k}_to_{dk}", k, dk, SPACE[k], space, np.uint8, ch), (k,)) for dk, space, ch in U8_DST for k in F32S]

CASES = SEPARABLE + CONV2D + BOX + RESIZE + GEOMETRY + FILTERS + CONVERT
assert len({(c.name, k) for c in CASES for k in c.kinds}) == sum(len(c.kinds) for c in CASES)


def nan_on_black(shape):
    host = np.zeros(shape, np.float32)
    host[shape[0] // 2, shape[1] // 2] = np.nan
    host.flags.writeable = False
    return host


def runs(case, kind):
    """Every (frame name, source shape, destination shape) of one (op, pixel type)."""
    return [(name, shape, case.dst_shape(*shape)) for name in case.frames for shape in SHAPES]


def want_of(oracle, case, kind, name, shape):
    """The oracle's output for one run (milliseconds each; nothing is kept)."""
    return case.op.ref(oracle, DF.frame(name, kind, *shape), case.dst_shape(*shape))


def run_device(case, kind, host, dst_shape):
    """The op on contiguous device images; the destination starts as a pattern no op produces (0xA5 bytes), so an unwritten pixel shows."""
    dtype, ch = V.LAYOUT[case.dst_kind(kind)]
    shape = tuple(dst_shape) + ((ch,) if ch > 1 else ())
    src = torch.from_numpy(np.array(host)).cuda()
    dst = torch.full((int(np.prod(shape)) * (1 if dtype == torch.uint8 else 4),), V.SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and src.is_contiguous() and dst.is_contiguous()
    case.op.call(zg.Image(src), zg.Image(dst))
    torch.cuda.synchronize()
    return dst.cpu().numpy(), src.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", [pytest.param(c, k, id=f"{c.name}-{k}") for c in CASES for k in c.kinds])
def test_f32_route_on_the_whole_value_domain(oracle, case, kind):
    for name, shape, dst_shape in runs(case, kind):
        host = DF.frame(name, kind, *shape)
        what = f"{case.name} {kind} {name} {shape[0]}x{shape[1]} -> {dst_shape[0]}x{dst_shape[1]}"
        got, src_after = run_device(case, kind, host, dst_shape)
        assert_bits_equal_nan_class(got, want_of(oracle, case, kind, name, shape), what)
        assert_bits_equal_nan_class(src_after, host, what + ": the source changed")


# ---- metrics on f32 pairs ------------------------------------------------------------------------------------------------------------
# metrics.hip: the f32 types make their f64 terms on the fly (a generator per metric; k_ssim writes the map first), k_chunk_sums and k_chunk_guess
# guess each chunk's binade, k_chunk_records (metrics.hip:203-215) marks a chunk `bad` when a term leaves that binade's exponent range (an infinity,
# a NaN, a term too large for the integers used) and k_walk then adds that chunk serially. Terms are f64: the squares of (huge, -huge) reach
# 2^256 and stay finite (an f32 difference cannot overflow an f64 square), so that pair's sum is huge and finite; the sum is NaN only through
# the infinities and NaN of `nonfinite` (tests/test_domain_frames.py holds each pair to that).
def disturbed(a):
    rng = np.random.default_rng(5)
    b = (a * (np.float32(1) + (rng.random(a.shape, np.float32) - np.float32(0.5)) * np.float32(0.01) * (rng.random(a.shape) < 0.6))).astype(np.float32)
    b.flags.writeable = False
    return b


def metric_pairs(kind, shape):
    f = lambda name: DF.frame(name, kind, *shape)
    return (("signed,disturbed", f("signed"), disturbed(f("signed"))), ("huge,-huge", f("huge"), -f("huge")),
            ("nonfinite,signed", f("nonfinite"), f("signed")), ("tiny,negzero", f("tiny"), f("negzero")))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", F32S)
def test_metrics_on_f32_pairs_of_the_whole_value_domain(kind):
    from zignal_amd import metrics as M
    for shape in SHAPES:
        for pair_name, a, b in metric_pairs(kind, shape):
            ia, ib = (zg.Image(torch.from_numpy(np.array(x)).cuda()) for x in (a, b))
            with np.errstate(all="ignore"):
                sq, ab, smap = R.difference_terms(a, b, True), R.difference_terms(a, b, False), R.ssim_map(a, b, zg.ssim_window())
                wants = {"psnr": (R.left_to_right(sq), sq.size, R.mse(a, b)),
                         "mean_pixel_error": (R.left_to_right(ab), ab.size, R.mean_pixel_error(a, b)),
                         "ssim": (R.left_to_right(smap), smap.size, R.left_to_right(smap) / float(smap.size))}
            for metric, (want_sum, count, want_value) in wants.items():
                res = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
                getattr(ia, metric)(ib, result=res)
                torch.cuda.synchronize()
                r = M._record(res)
                what = (metric, kind, pair_name, shape, float(r["sum"]), want_sum, float(r["value"]), want_value)
                assert R.same_bits_nan_class(float(r["sum"]), want_sum), what
                assert R.same_bits_nan_class(float(r["value"]), want_value), what
                assert int(r["count"]) == count and 0 <= int(r["serial_terms"]) <= count, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("canny", "shen_castan"))
def test_edge_detectors_see_a_nan_pixel_of_an_f32_plane_as_255(oracle, name):
    """A black Image(f32) with one NaN: the grey byte of the NaN is 255 (canny_gray), so the detector draws a ring around it; as the byte 0
    it would draw nothing (tests/test_domain_frames.py holds the oracle to the ring)."""
    case = next(c for c in CASES if c.name == name)
    for shape in SHAPES:
        host = nan_on_black(shape)
        got, _ = run_device(case, "f32", host, shape)
        want = case.op.ref(oracle, host, shape)
        assert want.any()
        assert_bits_equal_nan_class(got, want, f"{name} f32 black with one NaN {shape}")

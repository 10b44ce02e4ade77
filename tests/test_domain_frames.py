"""tests/domain_frames.py and the expected outputs of tests/test_gpu_f32_domain.py, from the oracle alone: conditions on the inputs, so that no
GPU case can pass by being empty. Each frame holds what its name says; over every (op, pixel type, frame, shape) the GPU file runs, at most
10 % of an expected f32 output is NaN, an output of a `nonfinite*` frame holds a NaN or an infinity, a linear filter of `tiny` stays at least
10 % subnormal, and `negzero` comes out with the signs of zero the reference's accumulators give it.

No GPU is needed, but torch is: the table is made of the Op objects of tests/test_gpu_dst_views.py, imported and not copied, and that module and
tests/views.py import torch to describe their canvases."""
import numpy as np
import pytest

from tests import domain_frames as DF
from tests import test_gpu_f32_domain as G
from tests.util import assert_bits_equal_nan_class

KINDS = tuple(DF.CHANNELS)


def fraction(mask):
    return float(np.count_nonzero(mask)) / mask.size


# ---- the frames ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", G.SHAPES)
def test_each_frame_holds_what_its_name_says(kind, rows, cols):
    ch = DF.CHANNELS[kind]
    frames = {name: DF.frame(name, kind, rows, cols) for name in DF.NAMES}
    for name, f in frames.items():
        assert f.dtype == np.float32 and f.shape == ((rows, cols) if ch == 1 else (rows, cols, ch)) and not f.flags.writeable, name
        assert DF.frame(name, kind, rows, cols) is f  # built once
        again = DF.frame.__wrapped__(name, kind, rows, cols)
        assert np.array_equal(DF.u32(again), DF.u32(f)), name  # and deterministic
    for name, lo, hi in (("signed", -40, 40), ("huge", 107, 126), ("huge_sat", 90, 109)):
        f = frames[name]
        exponent = ((DF.u32(f) >> np.uint32(23)) & np.uint32(255)).astype(np.int64) - 127
        assert exponent.min() == lo and exponent.max() == hi and np.isfinite(f).all(), name
        assert 0.4 < fraction(f < 0) < 0.6 and len(np.unique(DF.u32(f) & np.uint32(0x7FFFFF))) > f.size // 2, name
    t, flat = frames["tiny"], DF.u32(frames["tiny"]).reshape(-1)
    assert ((flat & np.uint32(0x7FFFFFFF)) < np.uint32(1 << 25)).all()
    assert (flat[::17] == DF.NEG_ZERO).all() and (flat[::19][np.arange(0, flat.size, 19) % 17 != 0] == 0).all()
    assert fraction(DF.is_subnormal(t)) > 0.2 and fraction(~DF.is_subnormal(t) & (t != 0)) > 0.5 and 0.4 < fraction(np.signbit(t)) < 0.6
    z = frames["negzero"]
    patch = z == np.float32(1.5)
    assert np.count_nonzero(patch) == DF.PATCH * DF.PATCH * ch and (DF.is_neg_zero(z) | DF.is_pos_zero(z) | patch).all()
    grid = np.zeros(z.shape, bool)
    grid[::3, ::5] = True
    assert (DF.is_pos_zero(z) == (grid & ~patch)).all() and fraction(DF.is_neg_zero(z)) > 0.9
    for name, sites in (("nonfinite", DF.nonfinite_sites(rows, cols)), ("nonfinite_corner", DF.corner_sites(rows, cols))):
        f = frames[name].reshape(rows, cols, ch)
        special = ~np.isfinite(f)
        assert np.count_nonzero(special) == len(sites), name
        for i, ((r, c), bits) in enumerate(zip(sites, DF.SPECIALS)):
            assert DF.u32(f)[r, c, i % ch] == bits and np.count_nonzero(special[r, c]) == 1, (name, i)  # one field of its pixel, field i mod channels
        finite = f[~special]
        assert finite.min() >= -2 and finite.max() <= 2 and 0.4 < fraction(finite < 0) < 0.6, name
    n = DF.frame("nonfinite", kind, rows, cols).reshape(rows, cols, ch)
    assert [int(np.count_nonzero(x)) for x in (n == np.inf, n == -np.inf, DF.is_nan(n))] == [2, 2, 2]
    sites = DF.nonfinite_sites(rows, cols)
    assert sites[0] == (0, 0) and sites[1] == (rows // 2, cols // 2) and sites[2][0] == rows - 1 and sites[3][1] == cols - 1
    assert all(0 < r < rows - 1 and 0 < c < cols - 1 for r, c in sites[4:]) and len(set(sites)) == 6
    assert all(r >= rows - 3 and c >= cols - 3 for r, c in DF.corner_sites(rows, cols))


def test_nan_class_comparison():
    a = np.array([1.0, -0.0, np.inf, np.nan, 1e-45], np.float32)
    b = a.copy()
    b.view(np.uint32)[3] = 0xFFC00001  # another NaN: sign and payload do not count
    assert_bits_equal_nan_class(a, b)
    for i, v in ((1, 0.0), (2, -np.inf), (3, 0.0), (0, np.nan), (4, 0.0)):
        c = a.copy()
        c[i] = v
        with pytest.raises(AssertionError):
            assert_bits_equal_nan_class(c, a, "differs")
    with pytest.raises(AssertionError):
        assert_bits_equal_nan_class(np.array([1, 2], np.uint8), np.array([1, 3], np.uint8))
    assert_bits_equal_nan_class(np.array([1, 2], np.uint8), np.array([1, 2], np.uint8))


# ---- the expected outputs ----------------------------------------------------------------------------------------------------------------
NO_NEG_ZERO = ("gaussian_blur_0.6", "gaussian_blur_1.0", "gaussian_blur_2.5", "convolve_separable_5", "convolve_separable_13",
               "convolve_separable_5_zero_border", "convolve_separable_9_zero_end_taps")  # every accumulator starts at +0.0: (+0.0) + (-0.0) = +0.0
BOTH_ZEROS = ("resize_bilinear_up", "resize_bilinear_up3", "resize_nearest_down", "resize_nearest_up", "resize_nearest_up3", "sharpen_2")


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in G.CASES])
def test_expected_outputs_hold_their_classes(oracle, case):
    for kind in case.kinds:
        for name, shape, dst_shape in G.runs(case, kind):
            want = G.want_of(oracle, case, kind, name, shape)
            what = (case.name, kind, name, shape)
            ch = G.V.LAYOUT[case.dst_kind(kind)][1]
            assert want.shape == tuple(dst_shape) + ((ch,) if ch > 1 else ()), what
            if want.dtype != np.float32:
                assert want.dtype == np.uint8, what
                if name in ("signed", "nonfinite"):  # both ends of the byte range: the clamp is at work
                    assert want.min() == 0 and want.max() == 255, what
                continue
            nan, inf = fraction(DF.is_nan(want)), fraction(DF.is_inf(want))
            assert nan <= 0.10, (what, nan)
            if name.startswith("nonfinite"):
                assert nan + inf > 0, what
            elif name != "negzero":  # (an insert can cover negzero's patch of 1.5 and leave the two zeros)
                assert len(np.unique(DF.u32(want))) > 2, what
            if name == "tiny" and case.linear:
                assert fraction(DF.is_subnormal(want)) >= 0.10, (what, fraction(DF.is_subnormal(want)))
            if name == "negzero":
                if case.name in NO_NEG_ZERO:
                    assert not DF.is_neg_zero(want).any() and DF.is_pos_zero(want).any(), what
                if case.name in BOTH_ZEROS:
                    assert DF.is_neg_zero(want).any() and DF.is_pos_zero(want).any(), (what, fraction(DF.is_neg_zero(want)))
            if case.name == "convolve_separable_5_times_3":
                assert inf > 0, what  # the sums do overflow


def test_the_zero_end_taps_make_nan_at_the_border_only(oracle):
    """oracle/conv.c:191,215: the interior skips a tap with |k| < 1e-10, the border does not. The corner special of `nonfinite` is a +inf
    under a 0.0 tap for the border pixels that reach it; the centre special is an infinity too and makes no NaN."""
    case = next(c for c in G.CASES if c.name == "convolve_separable_9_zero_end_taps")
    for kind in case.kinds:
        for shape in G.SHAPES:
            rows, cols = shape
            want = G.want_of(oracle, case, kind, "nonfinite", shape).reshape(rows, cols, -1)
            frame = DF.frame("nonfinite", kind, rows, cols).reshape(rows, cols, -1)
            (r0, c0), (r1, c1) = DF.nonfinite_sites(rows, cols)[:2]
            assert frame[r0, c0, 0] == np.inf and DF.is_inf(frame[r1, c1, 1 % frame.shape[2]])
            assert DF.is_nan(want[:9, :9, 0]).any(), (kind, shape)
            centre = want[r1 - 4:r1 + 5, c1 - 4:c1 + 5, 1 % frame.shape[2]]
            assert DF.is_inf(centre).any() and not DF.is_nan(centre).any(), (kind, shape)


def test_the_metric_pairs_reach_their_sums():
    from tests import metrics_ref as R
    for kind in KINDS:
        for shape in G.SHAPES:
            sums = {}
            for pair_name, a, b in G.metric_pairs(kind, shape):
                with np.errstate(all="ignore"):
                    sums[pair_name] = R.left_to_right(R.difference_terms(a, b, True))
            assert 0 < sums["signed,disturbed"] < np.inf and 2.0 ** 200 < sums["huge,-huge"] < np.inf  # f64 squares of f32 differences stay finite
            assert np.isnan(sums["nonfinite,signed"]) and 0 < sums["tiny,negzero"] < np.inf


def test_a_nan_becomes_the_byte_255_in_the_mixed_inserts_and_the_edge_detectors(oracle):
    """The cases of tests/test_gpu_f32_domain.py that reach convertColor's clamp outside Image.convert: a 1:1 insert of `nonfinite` into a u8
    type has 255 at both NaN sites (in the NaN's own field where the destination keeps fields), and canny / shen_castan draw a ring around
    the one NaN of a black plane (its grey byte is 255; as 0 there would be nothing to draw)."""
    for case in G.INSERT_MIXED:
        if not case.name.endswith("1to1"):
            continue
        for kind in case.kinds:
            for shape in G.SHAPES:
                want = G.want_of(oracle, case, kind, "nonfinite", shape).reshape(shape + (-1,))
                frame = DF.frame("nonfinite", kind, *shape).reshape(shape + (-1,))
                sites = np.argwhere(DF.is_nan(frame))
                assert len(sites) == 2
                for r, c, f in sites:
                    px = want[r, c]
                    if frame.shape[2] == 1:  # a grey source is replicated
                        assert (px[:3] == 255).all(), (case.name, kind, shape, px)
                    elif px.size == 1:  # a grey destination takes the clamped luminance, which alpha is no part of
                        assert px[0] == 255 or f == 3, (case.name, kind, shape, px)
                    else:
                        assert f >= px.size or px[f] == 255, (case.name, kind, shape, px)
    for name in ("canny", "shen_castan"):
        case = next(c for c in G.CASES if c.name == name)
        for shape in G.SHAPES:
            assert case.op.ref(oracle, G.nan_on_black(shape), shape).any(), (name, shape)
            assert not case.op.ref(oracle, np.zeros(shape, np.float32), shape).any(), (name, shape)

"""Every one of the 2^24 Rgb(u8) colours through the colour kernels, bit for bit against the CPU oracle. tests/test_gpu_color.py samples a
64^3 lattice; here the argument set of a u8 source, which is finite, is simply exhausted: the fast forms of zg_colordev.h hand about one
lane in 32 768 back to the plain form through rare-branch groups shared by three values, and the IN_RANGE instantiations drop the range
tests on the strength of a host-side look at the table, so a fault there shows on a handful of colours and in the last bit.

Colour i is (i >> 16, (i >> 8) & 255, i & 255); slab k holds colours k * 2^22 .. (k + 1) * 2^22 as 1024 x 4096 pixels (rows of 12 288
bytes). Per (space, slab) the oracle's forward conversion is computed once and shared by the forward and the backward test (a module-scoped
parametrised fixture keeps the tests of one case together, so one slab's 48 MB is alive at a time).

Which kernel a call takes is worked out in the test from convert.hip's rule (lab4_applies / lab4_back_applies: u8 side origin and pitch a
multiple of 4 bytes for Rgb, 16 for Rgba; f32 side origin and pitch a multiple of 16) and stated in the assertion's message.

The oracle's own round trip Rgb(u8) -> space(f32) -> Rgb(u8), max |back - rgb| over all 2^24 colours (measured on the CPU; asserted below
as an upper bound on the ORACLE's bytes, the device's bytes being equal to those):
    HSL 0   HSV 0   LAB 0   LCH 0   LMS 0   OKLAB 0   OKLCH 0   XYB 0   XYZ 0   YCBCR 0

1 : 1 bilinear: oracle.resize(slab as Rgba(u8), its own shape, BILINEAR) returns its input bit for bit, so one slab also goes through the fused
resize_convert kernels (Rgba(u8) bilinear -> Oklab / Xyz) at the source's own size and must equal the plain conversion."""
import functools

import numpy as np
import pytest

import zignal_amd as zg
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SPACES = ("HSL", "HSV", "LAB", "LCH", "LMS", "OKLAB", "OKLCH", "XYB", "XYZ", "YCBCR")
ROUND_TRIP_MAX = {"HSL": 0, "HSV": 0, "LAB": 0, "LCH": 0, "LMS": 0, "OKLAB": 0, "OKLCH": 0, "XYB": 0, "XYZ": 0, "YCBCR": 0}
SLABS, ROWS, COLS = 4, 1024, 4096
LAB4 = ("XYZ", "OKLAB", "LAB")  # k_u8_to_lab4's destinations
SENTINEL = 0xA5


def cs(name):
    return getattr(zg, "CS_" + name)


@functools.lru_cache(maxsize=2)
def slab_rgb(k):
    i = np.arange(k << 22, (k + 1) << 22, dtype=np.uint32)
    out = np.stack([i >> 16, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(ROWS, COLS, 3)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def slab_rgba(k):
    rgb = slab_rgb(k)
    out = np.ascontiguousarray(np.concatenate([rgb, rgb[..., 2:3]], -1))  # alpha = i & 255: the alpha lane is not constant
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def want(oracle, space, k):
    """The oracle's forward conversion of a slab: computed once, shared by forward and back, never written."""
    out = oracle.convert(slab_rgb(k), zg.CS_RGB, cs(space), np.float32, 3)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def not_plain_table(oracle):
    """The library's table with entry 0 as -0.0: device_srgb_lut (convert.hip) calls a table plain when every entry is +0 or within
    [2^-60, 2^60], so this one is not, and the range-tested instantiations run; no colour's value moves except black's zero signs, which
    the oracle, given the same table, reproduces."""
    lut = oracle.srgb_to_linear_lut().copy()
    assert lut.view(np.uint32)[0] == 0 and ((lut.view(np.uint32)[1:] >= 0x21800000) & (lut.view(np.uint32)[1:] < 0x5D800000)).all(), "the library's own table is plain"
    lut[0] = np.float32(-0.0)
    assert lut.view(np.uint32)[0] == 0x80000000
    lut.setflags(write=False)
    return lut


@pytest.fixture(scope="module", params=[(s, k) for k in range(SLABS) for s in SPACES], ids=lambda p: f"{p[0]}-slab{p[1]}")
def case(request):
    return request.param


@pytest.fixture(scope="module", params=range(SLABS), ids=lambda k: f"slab{k}")
def slab(request):
    return request.param


def up(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared host arrays are read-only


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def aligned(t, need):
    """origin and pitch of a device tensor's rows both multiples of `need` bytes"""
    return t.data_ptr() % need == 0 and t.stride(0) * t.element_size() % need == 0


def test_forward(oracle, case):
    space, k = case
    rgb, expect = slab_rgb(k), want(oracle, space, k)
    assert rgb.shape == (ROWS, COLS, 3) and int(rgb[0, 0, 0]) == k * 64 and tuple(rgb[-1, -1]) == (k * 64 + 63, 255, 255)
    four = space in LAB4
    # aligned Rgb(u8)
    src, dst = up(rgb), torch.empty((ROWS, COLS, 3), dtype=torch.float32, device="cuda")
    assert aligned(src, 4) and aligned(dst, 16), "an aligned frame: rows of 12 288 and 49 152 bytes"
    route = "k_u8_to_lab4<3> with the library's table (IN_RANGE)" if four else "k_convert_spaces"
    zg.Image(src).convert(cs(space), np.float32, out=zg.Image(dst))
    assert_bits_equal(down(dst), expect, f"Rgb(u8) -> {space}, slab {k}, aligned: {route}")
    # a caller's table that is not plain: the range-tested instantiations
    if four:
        lut = not_plain_table(oracle)
        with np.errstate(all="ignore"):
            expect_lut = oracle.convert(rgb, zg.CS_RGB, cs(space), np.float32, 3, srgb_lut=lut)
        zg.Image(src).convert(cs(space), np.float32, out=zg.Image(dst), srgb_lut=lut)
        assert_bits_equal(down(dst), expect_lut, f"Rgb(u8) -> {space}, slab {k}, aligned, table with -0.0: k_u8_to_lab4<3> without IN_RANGE")
        same = expect_lut.view(np.uint32) == expect.view(np.uint32)
        assert same.reshape(-1, 3)[1:].all() if k == 0 else same.all(), "the -0.0 entry moves no colour but black"
        del expect_lut
    # the same pixels one pixel into a parent one pixel wider: the origin sits at byte 3
    parent = torch.full((ROWS, COLS + 1, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    view = parent[:, 1:]
    view.copy_(src)
    del src
    assert view.data_ptr() % 4 == 3 and not aligned(view, 4), "origin at byte 3 of the allocation: lab4_applies is false"
    zg.Image(view).convert(cs(space), np.float32, out=zg.Image(dst))
    assert_bits_equal(down(dst), expect, f"Rgb(u8) view at byte 3 -> {space}, slab {k}: {'k_convert' if space in ('XYZ', 'OKLAB') else 'k_convert_spaces'}")
    assert bool((parent[:, 0] == SENTINEL).all()), "the source's parent was written"
    del parent, view
    # Rgba(u8), aligned, alpha moving
    rgba = slab_rgba(k)
    src4 = up(rgba)
    assert aligned(src4, 16) and aligned(dst, 16)
    expect4 = oracle.convert(rgba, zg.CS_RGBA, cs(space), np.float32, 3)
    zg.Image(src4).convert(cs(space), np.float32, out=zg.Image(dst))
    assert_bits_equal(down(dst), expect4, f"Rgba(u8) -> {space}, slab {k}, aligned: {'k_u8_to_lab4<4> (IN_RANGE)' if four else 'k_convert_spaces'}")
    assert_bits_equal(expect4, expect, f"the oracle's Rgba(u8) -> {space} against its Rgb(u8) -> {space}")
    del src4, dst
    torch.cuda.empty_cache()


def test_back_and_round_trip(oracle, case):
    space, k = case
    rgb, there = slab_rgb(k), want(oracle, space, k)
    src = up(there)
    assert aligned(src, 16)
    for dst_space, ch in ((zg.CS_RGB, 3), (zg.CS_RGBA, 4)):
        expect = oracle.convert(there, cs(space), dst_space, np.uint8, ch)
        if ch == 3:  # the reference: how far the oracle's own round trip strays
            worst = int(np.abs(expect.astype(np.int16) - rgb.astype(np.int16)).max())
            assert worst <= ROUND_TRIP_MAX[space], f"the oracle's {space} round trip on slab {k}: max |back - rgb| = {worst}"
        else:
            assert (expect[..., 3] == 255).all()
        dst = torch.empty((ROWS, COLS, ch), dtype=torch.uint8, device="cuda")
        assert aligned(dst, 16 if ch == 4 else 4)
        zg.Image(src).convert(dst_space, np.uint8, src_space=cs(space), out=zg.Image(dst))
        route = f"k_lab4_to_u8<{ch}>" if space == "LAB" else "k_convert_spaces"
        assert_bits_equal(down(dst), expect, f"{space} -> {'Rgba' if ch == 4 else 'Rgb'}(u8), slab {k}, aligned: {route}")
        del dst
        if space == "LAB":  # a destination one pixel into a parent one pixel wider and two rows taller: lab4_back_applies is false
            parent = torch.full((ROWS + 2, COLS + 1, ch), SENTINEL, dtype=torch.uint8, device="cuda")
            view = parent[1:-1, 1:]
            assert not aligned(view, 16 if ch == 4 else 4), f"origin {view.data_ptr() % 16} mod 16, pitch {(COLS + 1) * ch}"
            zg.Image(src).convert(dst_space, np.uint8, src_space=zg.CS_LAB, out=zg.Image(view))
            assert_bits_equal(down(view), expect, f"LAB -> {ch}-channel u8 view, slab {k}, misaligned: k_convert_spaces")
            outside = parent != SENTINEL
            outside[1:-1, 1:] = False
            assert not bool(outside.any()), f"LAB -> {ch}-channel u8 view, slab {k}: a byte outside the view was written"
            del parent, view, outside
    del src
    torch.cuda.empty_cache()


def test_ycbcr_u8_and_gray(oracle, slab):
    """The integer forms: Rgb(u8) -> Ycbcr(u8) (k_convert) and back (k_convert_spaces' u8 route), Rgb(u8) -> Gray(u8) / Gray(f32)."""
    k = slab
    rgb = slab_rgb(k)
    src = up(rgb)
    ycc = oracle.convert(rgb, zg.CS_RGB, zg.CS_YCBCR, np.uint8, 3)
    got = zg.Image(src).convert(zg.CS_YCBCR, np.uint8)
    assert_bits_equal(down(got.data), ycc, f"Rgb(u8) -> Ycbcr(u8), slab {k}")
    back = got.convert(zg.CS_RGB, np.uint8, src_space=zg.CS_YCBCR)
    assert_bits_equal(down(back.data), oracle.convert(ycc, zg.CS_YCBCR, zg.CS_RGB, np.uint8, 3), f"Ycbcr(u8) -> Rgb(u8), slab {k}")
    del got, back
    for dtype in (np.uint8, np.float32):
        got = zg.Image(src).convert(zg.CS_GRAY, dtype)
        assert_bits_equal(down(got.data), oracle.convert(rgb, zg.CS_RGB, zg.CS_GRAY, dtype, 1), f"Rgb(u8) -> Gray({np.dtype(dtype).name}), slab {k}")
        del got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("space", ("OKLAB", "XYZ"))
def test_fused_resize_convert_at_the_sources_own_size(oracle, space):
    """resize_convert's fused Rgba(u8) bilinear -> Oklab / Xyz kernels at 1 : 1, where bilinear resampling is the identity (asserted on the
    oracle's resize first): the result is the plain conversion of the slab. The last slab: bright colours, the cube's white corner."""
    k = SLABS - 1
    rgba = slab_rgba(k)
    assert_bits_equal(oracle.resize(rgba, (ROWS, COLS), oracle.method(oracle.BILINEAR)), rgba, "the oracle's 1 : 1 bilinear resize")
    got = zg.Image(up(rgba)).resize_convert((ROWS, COLS), cs(space), np.float32)
    assert_bits_equal(down(got.data), want(oracle, space, k), f"Rgba(u8) 1 : 1 bilinear + {space}, slab {k}: the fused kernel")

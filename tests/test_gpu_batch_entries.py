"""zg_batch_blur_resize and zg.Pipeline([blur, resize]) are two doors to one recipe: for every route of the u8 Gaussian and of the
resize behind it, both give the oracle's resize(gaussian_blur(frame)) bit for bit on every frame and leave the source frames alone.
The shapes are the smallest that still reach each route (the conditions are the try_* predicates' own: conv_sep_stream.hip,
conv_sep_rgba8.hip, conv_sep_bytes2.hip, geom.hip's resize_frames). zg_batch_blur_resize's return codes are pinned beside them."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import zignal_amd as zg  # noqa: E402
from zignal_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
I = zg.Interpolation

# kind, frames, rows, cols, out rows, out cols, method, sigma
CASES = {
    "stream_down2": ("rgba_u8", 3, 32, 272, 16, 136, "bilinear", 1.0),      # 7 taps, row bytes 1088 % 32 == 0: k_sep_stream's down2 form
    "tiled_down2": ("rgba_u8", 3, 34, 268, 17, 134, "bilinear", 1.0),       # row bytes 1072 % 32 == 16: the stream form refuses, k_sep_rgba8's down2 form takes it
    "no_down2": ("rgba_u8", 3, 34, 270, 17, 135, "bilinear", 1.0),          # cols % 4 == 2: both refuse; blur, then resize
    "blur_then_bicubic": ("rgba_u8", 3, 32, 272, 16, 100, "bicubic", 1.0),  # a batched blur, then a batched resize
    "nine_taps_half": ("rgba_u8", 3, 32, 272, 16, 136, "bilinear", 1.2),    # 9 taps on 4-byte pixels: (9 / 2 + 1) * 4 > 16, the stream kernel refuses
    "nine_taps_bicubic": ("rgba_u8", 3, 32, 272, 16, 100, "bicubic", 1.2),
    "long_taps": ("rgba_u8", 3, 32, 272, 16, 136, "bilinear", 6.0),         # 37 taps: past every 9-tap route
    "long_taps_one_frame": ("rgba_u8", 1, 32, 272, 16, 136, "bilinear", 6.0),
    "rgb_u8": ("rgb_u8", 3, 32, 272, 16, 136, "bilinear", 0.6),             # 272 columns: row bytes a multiple of 16 for 1, 3 and 4 bytes per pixel
    "u8": ("u8", 3, 32, 272, 16, 136, "bilinear", 0.6),
    "unaligned": ("rgba_u8", 3, 31, 131, 16, 65, "bilinear", 0.6),          # nothing is aligned: every frame on its own
    "rgba_f32": ("rgba_f32", 3, 40, 72, 20, 36, "bilinear", 0.6),
    "sigma_zero": ("rgba_u8", 3, 32, 272, 16, 136, "bilinear", 0.0),        # the blur is a copy
}
LAYOUT = {"u8": (np.uint8, 1, L.PIXEL_U8), "rgb_u8": (np.uint8, 3, L.PIXEL_RGB_U8), "rgba_u8": (np.uint8, 4, L.PIXEL_RGBA_U8), "rgba_f32": (np.float32, 4, L.PIXEL_RGBA_F32)}


def batch_blur_resize(src, n, rows, cols, pixel, sigma, dst, orows, ocols, method):
    m = method._c() if method is not None else None
    return zg.lib().zg_batch_blur_resize(C.c_void_p(src), n, rows, cols, pixel, C.c_float(sigma), C.c_void_p(dst), orows, ocols,
                                         C.byref(m) if m is not None else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("case", CASES)
def test_both_entries_one_answer(oracle, case):
    kind, n, rows, cols, orows, ocols, mname, sigma = CASES[case]
    dtype, ch, pixel = LAYOUT[kind]
    method, omethod = getattr(I, mname), oracle.method(getattr(oracle, mname.upper()))
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    synth = oracle.synth_f32 if dtype == np.float32 else oracle.synth_u8
    host = np.stack([synth(400 + f, shape) for f in range(n)])
    want = np.stack([oracle.resize(oracle.gaussian_blur(f, sigma), (orows, ocols), omethod) for f in host])
    src = torch.from_numpy(host).cuda()
    oshape = (n, orows, ocols) if ch == 1 else (n, orows, ocols, ch)

    direct = torch.zeros(oshape, dtype=src.dtype, device="cuda")
    rc = batch_blur_resize(src.data_ptr(), n, rows, cols, pixel, sigma, direct.data_ptr(), orows, ocols, method)
    assert rc == 0, zg.lib().zg_last_error()
    piped = zg.Pipeline([zg.Step.gaussian_blur(sigma), zg.Step.resize(orows, ocols, method)]).run(src)
    torch.cuda.synchronize()
    for entry, got in (("zg_batch_blur_resize", direct.cpu().numpy()), ("Pipeline", piped.cpu().numpy())):
        assert got.shape == want.shape and got.dtype == want.dtype, (entry, got.shape, want.shape)
        for f in range(n):
            assert np.array_equal(got[f].view(np.uint8), want[f].view(np.uint8)), f"{case}: {entry}, frame {f} differs from the oracle"
    assert np.array_equal(src.cpu().numpy().view(np.uint8), host.view(np.uint8)), f"{case}: the source frames changed"


def test_batch_blur_resize_return_codes():
    n, rows, cols, orows, ocols = 2, 16, 64, 8, 32
    src = torch.full((n, rows, cols, 4), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((n, orows, ocols, 4), 0xA5, dtype=torch.uint8, device="cuda")
    call = lambda **kw: batch_blur_resize(**{**dict(src=src.data_ptr(), n=n, rows=rows, cols=cols, pixel=L.PIXEL_RGBA_U8, sigma=1.0, dst=dst.data_ptr(),  # noqa: E731
                                                    orows=orows, ocols=ocols, method=I.bilinear), **kw})
    assert call(method=None) == L.ERR_INVALID_ARGUMENT
    assert call(sigma=-1.0) == L.ERR_INVALID_ARGUMENT
    assert call(sigma=float("nan")) == L.ERR_INVALID_ARGUMENT
    assert call(pixel=99) == L.ERR_INVALID_ARGUMENT and call(pixel=-1) == L.ERR_INVALID_ARGUMENT
    assert call(src=None) == L.ERR_INVALID_ARGUMENT and call(dst=None) == L.ERR_INVALID_ARGUMENT
    bad = I.bilinear._c()
    bad.kind = 99
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert zg.lib().zg_batch_blur_resize(C.c_void_p(src.data_ptr()), n, rows, cols, L.PIXEL_RGBA_U8, C.c_float(1.0), C.c_void_p(dst.data_ptr()), orows, ocols,
                                         C.byref(bad), stream) == L.ERR_INVALID_ARGUMENT
    # nothing to do is no error, whatever the pointers are, and nothing is touched
    for zero in ("n", "rows", "cols", "orows", "ocols"):
        assert call(**{zero: 0}) == 0, zero
        assert call(**{zero: 0}, src=None, dst=None) == 0, zero
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()), "an empty batch wrote to the destination"
    assert bool((src == 7).all())

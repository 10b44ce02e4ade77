"""Palette quantisation and dithering (reference src/image/quantize.zig, src/image/dither.zig, mapImageToPalette of src/codecs/gif.zig)
through the zg_color_histogram / zg_median_cut / zg_palette_lut / zg_dither / zg_palette_map entry points (include/zignal_hip_quantize.h).
Image.color_histogram, .median_cut, .dither and .map_to_palette (zignal_amd/image.py) call into this module.
A palette is an (n, 3) uint8 array, 1 <= n <= 256; a lookup table is 32768 bytes indexed by r5 << 10 | g5 << 5 | b5."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_U8P = C.POINTER(C.c_uint8)
_U32P = C.POINTER(C.c_uint32)


class DitherMode:
    """dither.Mode (dither.zig:18-30), the reference's ordinals. `none` and `auto` leave the image as it is."""
    none, floyd_steinberg, atkinson, ordered, auto = range(5)


class PaletteMode:
    """PaletteMode (quantize.zig:476-498), the reference's ordinals; `adaptive` takes max_colors."""
    fixed_6x7x6, fixed_vga16, fixed_web216, adaptive = range(4)


def dither_geometry():
    """(band rows, phase columns, rows per launch) of the error-diffusion kernel (zg_dither_geometry)."""
    b, p, r = C.c_uint32(), C.c_uint32(), C.c_uint32()
    L.lib().zg_dither_geometry(C.byref(b), C.byref(p), C.byref(r))
    return int(b.value), int(p.value), int(r.value)


def _host_palette(palette) -> np.ndarray:
    p = np.ascontiguousarray(palette, np.uint8)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("a palette is an (n, 3) uint8 array")
    return p


def _is_device(t) -> bool:
    return hasattr(t, "is_cuda") and t.is_cuda


def _device_bytes(t, name: str, nbytes: int, device):
    """The pointer of a contiguous uint8 device tensor of at least nbytes bytes on `device`."""
    import torch
    if not (_is_device(t) and t.dtype == torch.uint8 and t.is_contiguous() and t.device == device and t.numel() >= nbytes):
        raise ValueError(f"{name} is a contiguous uint8 tensor of at least {nbytes} bytes on the image's device")
    return C.c_void_p(t.data_ptr())


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def median_cut_from_histogram(counts, first, max_colors: int = 256, capacity: int = 256) -> np.ndarray:
    """zg_median_cut_from_histogram_host: medianCut (quantize.zig:239-412) from the 32768 counts and first raster indices of a colour
    histogram, as an (n, 3) uint8 palette. Host arithmetic, no GPU needed. InvalidArgument (NoPaletteColors) when nothing can be written."""
    counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
    first = np.ascontiguousarray(first, np.uint32).reshape(-1)
    if counts.size != L.HISTOGRAM_CELLS or first.size != L.HISTOGRAM_CELLS:
        raise ValueError(f"counts and first hold {L.HISTOGRAM_CELLS} words each")
    out, n = np.zeros((max(int(capacity), 1), 3), np.uint8), C.c_uint32(0)
    L.check(L.lib().zg_median_cut_from_histogram_host(counts.ctypes.data_as(_U32P), first.ctypes.data_as(_U32P), int(max_colors), int(capacity),
                                                      out.ctypes.data_as(_U8P), C.byref(n)))
    return out[:n.value].copy()


def build_palette(mode: int, image=None, max_colors: int = 256) -> np.ndarray:
    """buildPalette (quantize.zig:502-527) as an (n, 3) uint8 host array. The fixed modes need neither an image nor a GPU;
    PaletteMode.adaptive runs median cut on `image` (a device image) and falls back to the 6x7x6 palette when it fails."""
    out, n = np.zeros((256, 3), np.uint8), C.c_uint32(0)
    if int(mode) == PaletteMode.adaptive:
        if image is None or not image.on_device:
            raise ValueError("the adaptive palette is built from a device image")
        import torch
        d = image._desc()
        with torch.cuda.device(image.data.device):
            L.check(L.lib().zg_build_palette(C.byref(d), int(mode), int(max_colors), out.ctypes.data_as(_U8P), C.byref(n)))
    else:
        L.check(L.lib().zg_build_palette(None, int(mode), int(max_colors), out.ctypes.data_as(_U8P), C.byref(n)))
    return out[:n.value].copy()


def palette_lut(palette, out=None):
    """ColorLookupTable.init (quantize.zig:66-159). A host palette ((n, 3) uint8 array): computed on the host, returns a (32768,) uint8
    array. A device palette (a contiguous uint8 tensor of 3 n bytes): asynchronous on the current stream, returns a device tensor of
    32768 bytes (`out` when given)."""
    if not _is_device(palette):
        p = _host_palette(palette)
        lut = np.empty(L.HISTOGRAM_CELLS, np.uint8)
        L.check(L.lib().zg_palette_lut_host(p.ctypes.data_as(_U8P), p.shape[0], lut.ctypes.data_as(_U8P)))
        return lut
    import torch
    n = palette.numel() // 3
    pal = _device_bytes(palette, "palette", 3 * n, palette.device)
    if out is None:
        out = torch.empty(L.HISTOGRAM_CELLS, dtype=torch.uint8, device=palette.device)
    lut = _device_bytes(out, "out", L.HISTOGRAM_CELLS, palette.device)
    with torch.cuda.device(palette.device):
        L.check(L.lib().zg_palette_lut(pal, n, lut, _stream(palette.device)))
    return out


def _palette_on(palette, device):
    """(tensor, n) of a palette given as a host array or a device tensor."""
    import torch
    if _is_device(palette):
        return palette, palette.numel() // 3
    p = _host_palette(palette)
    return torch.from_numpy(p).to(device), p.shape[0]


def color_histogram(image, counts=None, first=None):
    """zg_color_histogram: (counts, first), two device tensors of 32768 32-bit words, asynchronous on the current stream."""
    import torch
    if not image.on_device:
        raise ValueError("color_histogram takes a device image")
    dev = image.data.device
    outs = []
    for name, t in (("counts", counts), ("first", first)):
        if t is None:
            t = torch.empty(L.HISTOGRAM_CELLS, dtype=torch.int32, device=dev)
        elif not (_is_device(t) and t.device == dev and t.is_contiguous() and t.numel() * t.element_size() >= 4 * L.HISTOGRAM_CELLS and t.data_ptr() % 4 == 0):
            raise ValueError(f"{name} is a contiguous tensor of at least {4 * L.HISTOGRAM_CELLS} bytes on the image's device")
        outs.append(t)
    d = image._desc()
    with torch.cuda.device(dev):
        L.check(L.lib().zg_color_histogram(C.byref(d), C.c_void_p(outs[0].data_ptr()), C.c_void_p(outs[1].data_ptr()), _stream(dev)))
    return outs[0], outs[1]


def median_cut(image, max_colors: int = 256, capacity: int = 256) -> np.ndarray:
    """zg_median_cut: medianCut of a device image as an (n, 3) uint8 host array; synchronises once."""
    import torch
    if not image.on_device:
        raise ValueError("median_cut takes a device image")
    out, n = np.zeros((max(int(capacity), 1), 3), np.uint8), C.c_uint32(0)
    d = image._desc()
    with torch.cuda.device(image.data.device):
        L.check(L.lib().zg_median_cut(C.byref(d), int(max_colors), int(capacity), out.ctypes.data_as(_U8P), C.byref(n)))
    return out[:n.value].copy()


def dither(image, palette, lut=None, mode: int = DitherMode.floyd_steinberg, n_frames: int = 1, frame_bytes: int = 0):
    """zg_dither / zg_dither_frames, in place on an Rgb(u8) device image; `palette` is a host array or a device tensor, `lut` the device
    table of that palette (built here when None). With n_frames > 1 the image describes the first of n_frames frames frame_bytes apart."""
    import torch
    if not image.on_device:
        raise ValueError("dither takes a device image")
    dev = image.data.device
    pal, n = _palette_on(palette, dev)
    if lut is None:
        lut = palette_lut(pal)
    d = image._desc()
    p, t = _device_bytes(pal, "palette", 3 * n, dev), _device_bytes(lut, "lut", L.HISTOGRAM_CELLS, dev)
    with torch.cuda.device(dev):
        if int(n_frames) == 1 and not frame_bytes:
            L.check(L.lib().zg_dither(C.byref(d), p, n, t, int(mode), _stream(dev)))
        else:
            L.check(L.lib().zg_dither_frames(C.byref(d), int(n_frames), int(frame_bytes), p, n, t, int(mode), _stream(dev)))
    return image


def map_to_palette(image, palette, use_dither: bool = False, transparent_index=None, out=None):
    """zg_palette_map (mapImageToPalette, gif.zig:875-920): the u8 index plane of a u8, Rgb(u8) or Rgba(u8) device image; `out`, when
    given, is a u8 device image of the same rows and cols (a view too)."""
    import torch
    if not image.on_device:
        raise ValueError("map_to_palette takes a device image")
    dev = image.data.device
    pal, n = _palette_on(palette, dev)
    if out is None:
        out = type(image)(torch.empty((image.rows, image.cols), dtype=torch.uint8, device=dev))
    s, o = image._desc(), out._desc()
    with torch.cuda.device(dev):
        L.check(L.lib().zg_palette_map(C.byref(s), C.byref(o), _device_bytes(pal, "palette", 3 * n, dev), n, 1 if use_dither else 0,
                                       -1 if transparent_index is None else int(transparent_index), _stream(dev)))
    return out

"""Seam carving (reference examples/src/seam_carving.zig) over the zg_seam_* entry points (include/zignal_hip_seam.h): the energy map
of an edge map, the seam of an energy map, its removal, and the whole iteration. Image.seam_carve and Image.seam_remove
(zignal_amd/image.py) end here.

Word buffers (energy maps, seams) are numpy uint32 arrays beside host images and contiguous torch int32 tensors beside device images:
torch has no arithmetic on unsigned words, and every sum and column is below 2^31, so the two read the same."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .image import Image, _is_torch, torch

_AXES = {"vertical": L.SEAM_VERTICAL, "horizontal": L.SEAM_HORIZONTAL}


def seam_band_rows() -> int:
    """Rows one launch of the energy kernel covers (zg_seam_band_rows)."""
    return int(L.lib().zg_seam_band_rows())


def seam_strip_cols() -> int:
    """Columns one wave of the energy kernel stores (zg_seam_strip_cols)."""
    return int(L.lib().zg_seam_strip_cols())


def _words(buf, count: int, like, name: str):
    """`buf`, or a new buffer, as `count` 32-bit words on the side (host / device) of `like`; returns (buffer, pointer)."""
    if _is_torch(like):
        if buf is None:
            buf = torch.empty(count, dtype=torch.int32, device=like.device)
        if not (_is_torch(buf) and buf.is_cuda and buf.device == like.device and buf.is_contiguous() and buf.element_size() == 4
                and buf.numel() >= count):
            raise ValueError(f"{name} is a contiguous tensor of at least {count} 32-bit words on the image's device")
        return buf, C.c_void_p(buf.data_ptr())
    if buf is None:
        buf = np.empty(count, np.uint32)
    if not (isinstance(buf, np.ndarray) and buf.dtype.itemsize == 4 and buf.dtype.kind in "iu" and buf.flags.c_contiguous and buf.size >= count):
        raise ValueError(f"{name} is a C-contiguous array of at least {count} 32-bit words")
    return buf, C.c_void_p(buf.ctypes.data)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def seam_energy(edges, out=None):
    """computeEnergy (:22-45): the rows x cols map of cumulative sums of an Image(u8) edge map, as rows * cols packed words, reshaped
    (rows, cols) when allocated here."""
    edges = Image._wrap(edges)
    own = out is None
    buf, ptr = _words(out, edges.rows * edges.cols, edges.data, "out")
    d = edges._desc()
    if edges.on_device:
        with torch.cuda.device(edges.data.device):
            L.check(L.lib().zg_seam_energy(C.byref(d), ptr, edges._stream()))
    else:
        L.check(L.lib().zg_seam_energy_host(C.byref(d), ptr))
    return buf.reshape(edges.rows, edges.cols) if own else buf


def seam_find(energy, rows: int, cols: int, out=None):
    """computeSeam (:47-74): the `rows` columns of the seam of a packed rows x cols energy map."""
    rows, cols = int(rows), int(cols)
    if not (0 <= rows < 1 << 32 and 0 <= cols < 1 << 32):
        raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"seam_find: {rows} x {cols}")
    if energy is None:
        raise TypeError("seam_find: energy is an array or a tensor of rows * cols words")
    energy, eptr = _words(energy, rows * cols, energy, "energy")
    buf, ptr = _words(out, rows, energy, "out")
    if _is_torch(energy):
        with torch.cuda.device(energy.device):
            L.check(L.lib().zg_seam_find(eptr, rows, cols, ptr, _stream(energy)))
    else:
        L.check(L.lib().zg_seam_find_host(eptr, rows, cols, ptr))
    return buf


def seam_remove(image: Image, seam, out=None) -> Image:
    """removeSeam (:76-102), out of place: row r of the rows x (cols - 1) result is row r of `image` without column seam[r]."""
    if image.cols < 1:
        raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, "seam_remove: the image has no column to lose")
    out = image._like(cols=image.cols - 1) if out is None else Image._wrap(out)
    image._same_side(out)
    _, sptr = _words(seam, image.rows, image.data, "seam")
    a, b = image._desc(), out._desc()
    if image.on_device:
        with torch.cuda.device(image.data.device):
            L.check(L.lib().zg_seam_remove(C.byref(a), sptr, C.byref(b), image._stream()))
    else:
        L.check(L.lib().zg_seam_remove_host(C.byref(a), sptr, C.byref(b)))
    return out


def seam_carve(image: Image, n: int, axis="vertical", out=None, seams=None) -> Image:
    """n iterations of seam_carve (:104-144): sobel, computeEnergy, computeSeam, removeSeam, the edge map recomputed from the carved
    frame each time. axis "vertical" removes n columns (the reference), "horizontal" n rows (the library's definition: the transposed
    frame is carved). `seams`, when given, receives n * rows words (n * cols for the horizontal axis): the column removed from each
    row at each iteration, in that iteration's coordinates."""
    n = int(n)
    ax = _AXES.get(axis, axis) if isinstance(axis, str) else axis
    if isinstance(ax, str) or not 0 <= n < 1 << 32:
        raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"seam_carve: n = {n}, axis {axis!r} (\"vertical\" or \"horizontal\")")
    ax = int(ax)
    across = image.rows if ax == L.SEAM_HORIZONTAL else image.cols
    if out is None:
        left = max(across - n, 0)
        out = image._like(rows=left) if ax == L.SEAM_HORIZONTAL else image._like(cols=left)
    else:
        out = Image._wrap(out)
    image._same_side(out)
    sptr = None
    if seams is not None:
        _, sptr = _words(seams, n * (image.cols if ax == L.SEAM_HORIZONTAL else image.rows), image.data, "seams")
    a, b = image._desc(), out._desc()
    if image.on_device:
        with torch.cuda.device(image.data.device):
            L.check(L.lib().zg_seam_carve(C.byref(a), C.byref(b), n, ax, None, sptr, image._stream()))
    else:
        L.check(L.lib().zg_seam_carve_host(C.byref(a), C.byref(b), n, ax, None, sptr))
    return out

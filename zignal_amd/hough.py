"""HoughTransform (reference src/image/hough.zig) over libzignal_hip.so's zg_hough_* entry points (include/zignal_hip_hough.h): the
accumulator of an edge map and the reference's list of lines, bit for bit.

Edge maps are Image(u8) (numpy on the host, a torch tensor on the device: what Image.canny / sobel / shen_castan return); a device
accumulator is a size x size int32 tensor holding the u32 counters (rows may be strided), a host one a numpy uint32 array."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib as L
from .image import Image, _is_torch

try:  # torch is plumbing (device memory + streams); the host flavour works without it
    import torch
except Exception:  # pragma: no cover
    torch = None

# HoughTransform.Line (hough.zig:13-25) as a numpy structured dtype: the bytes of zg_hough_line.
HOUGH_LINE_DTYPE = np.dtype([("angle", "<f4"), ("radius", "<f4"), ("score", "<u4"), ("p1", "<f4", (2,)), ("p2", "<f4", (2,))])
assert HOUGH_LINE_DTYPE.itemsize == C.sizeof(L.ZgHoughLine) == 28

_FIRST_CANDIDATES = 4096  # the synchronous forms start with room for this many candidates and ask again when there are more


class HoughLine(NamedTuple):
    """HoughTransform.Line: angle in degrees, radius from the centre, score, and the clipped segment's end points (x, y)."""
    angle: np.float32
    radius: np.float32
    score: int
    p1: Tuple[np.float32, np.float32]
    p2: Tuple[np.float32, np.float32]

    @classmethod
    def from_record(cls, rec) -> "HoughLine":
        return cls(np.float32(rec["angle"]), np.float32(rec["radius"]), int(rec["score"]), (np.float32(rec["p1"][0]), np.float32(rec["p1"][1])),
                   (np.float32(rec["p2"][0]), np.float32(rec["p2"][1])))


def lds_max_size() -> int:
    """The largest size whose voting kernel keeps its counters in LDS (zg_hough_lds_max_size)."""
    return int(L.lib().zg_hough_lds_max_size())


def pixel_chunk() -> int:
    """The edge list is shared out among the voting workgroups in multiples of this many pixels (zg_hough_pixel_chunk)."""
    return int(L.lib().zg_hough_pixel_chunk())


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def _device_accumulator(acc, size: int):
    if not _is_torch(acc) or not acc.is_cuda or acc.element_size() != 4 or acc.dim() != 2 or tuple(acc.shape) != (size, size):
        raise ValueError(f"the accumulator is a {size} x {size} device tensor of 32-bit integers")
    if acc.stride(1) != 1 or (size > 1 and acc.stride(0) < size):
        raise ValueError("the accumulator's rows must be contiguous")
    return acc.stride(0) if size > 1 else size


class HoughTransform:
    """HoughTransform (hough.zig:11-230). `size` is the resolution of Hough space and the side of the box of the edge image it reads."""

    def __init__(self, size: int, tables=None):
        size = int(size)
        if not 0 <= size < 1 << 32:
            raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"hough: size = {size}")
        self._h = C.c_void_p()
        if tables is None:
            L.check(L.lib().zg_hough_create(size, C.byref(self._h)))
        else:
            cos_t, sin_t = (np.ascontiguousarray(t, np.int32) for t in tables)
            if len(cos_t) != size or len(sin_t) != size:
                raise ValueError("tables: size entries each")
            L.check(L.lib().zg_hough_create_with_tables(size, cos_t.ctypes.data_as(L._I32P), sin_t.ctypes.data_as(L._I32P), C.byref(self._h)))
        self.size = size
        self.even_size = size if size % 2 == 0 else size - 1

    def close(self) -> None:
        if getattr(self, "_h", None):
            L.lib().zg_hough_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self):
        return f"HoughTransform(size={self.size})"

    @staticmethod
    def tables(size: int) -> Tuple[np.ndarray, np.ndarray]:
        """The cos and sin tables of HoughTransform.init (zg_hough_tables_host): host arithmetic, no GPU needed."""
        size = int(size)
        cos_t, sin_t = np.zeros(max(size, 0), np.int32), np.zeros(max(size, 0), np.int32)
        L.check(L.lib().zg_hough_tables_host(size, cos_t.ctypes.data_as(L._I32P), sin_t.ctypes.data_as(L._I32P)))
        return cos_t, sin_t

    def _box(self, box):
        l, t, r, b = (0, 0, self.size, self.size) if box is None else (int(v) for v in box)
        return l, t, r, b

    # ---- asynchronous device forms ------------------------------------------------------------------------------------
    def compute_into(self, edges, accumulator, box=None) -> None:
        """zg_hough_compute on the current stream: the votes of the non-zero pixels of `box` (l, t, r, b; default the top-left size x
        size) are added to `accumulator`. Nothing is cleared and nothing is synchronised."""
        img = Image._wrap(edges)
        if not img.on_device:
            raise ValueError("the _into forms take device tensors")
        stride = _device_accumulator(accumulator, self.size)
        l, t, r, b = self._box(box)
        d = img._desc()
        with torch.cuda.device(img.data.device):
            L.check(L.lib().zg_hough_compute(self._h, C.byref(d), l, t, r, b, C.c_void_p(accumulator.data_ptr()), stride, img._stream()))

    def find_lines_into(self, accumulator, threshold, angle_nms_thresh: float, radius_nms_thresh: float, lines, counts,
                        capacity: Optional[int] = None, max_candidates: int = 65536) -> None:
        """zg_hough_find_lines on the current stream. `threshold` is an int or a device tensor of at least 4 bytes, read by the
        kernels. `lines` (a device tensor of at least capacity x 28 bytes; capacity defaults to what it holds) receives the first
        min(counts[1], capacity) lines, `counts` (at least 8 bytes) [candidates, lines] as u32. Nothing is synchronised."""
        stride = _device_accumulator(accumulator, self.size)
        if not all(_is_torch(o) and o.is_cuda for o in (lines, counts)):
            raise ValueError("the _into forms take device tensors")
        cap = _nbytes(lines) // 28 if capacity is None else int(capacity)
        if cap * 28 > _nbytes(lines) or _nbytes(counts) < 8:
            raise ValueError("lines or counts tensor too small")
        thr_dev = None
        if _is_torch(threshold):
            if not threshold.is_cuda or _nbytes(threshold) < 4:
                raise ValueError("a device threshold is a device tensor of at least 4 bytes")
            thr_dev, thr = C.c_void_p(threshold.data_ptr()), 0
        else:
            thr = int(threshold)
            if not 0 <= thr < 1 << 32:
                raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"hough: threshold = {thr}")
        with torch.cuda.device(accumulator.device):
            stream = C.c_void_p(torch.cuda.current_stream(accumulator.device).cuda_stream)
            L.check(L.lib().zg_hough_find_lines(self._h, C.c_void_p(accumulator.data_ptr()), stride, thr, thr_dev, float(angle_nms_thresh),
                                                float(radius_nms_thresh), int(max_candidates), C.c_void_p(lines.data_ptr()) if cap else None, cap,
                                                C.c_void_p(counts.data_ptr()), stream))

    # ---- the reference's calls ----------------------------------------------------------------------------------------
    def compute(self, edges, box=None, accumulator=None):
        """HoughTransform.compute (:75-139). With accumulator None a zeroed one is made; otherwise the votes are added to it, as in
        the reference. Returns the accumulator: a numpy uint32 array for host edges, an int32 device tensor for device edges."""
        img = Image._wrap(edges)
        l, t, r, b = self._box(box)
        if img.on_device:
            if accumulator is None:
                accumulator = torch.zeros((self.size, self.size), dtype=torch.int32, device=img.data.device)
            self.compute_into(img, accumulator, (l, t, r, b))
            return accumulator
        if accumulator is None:
            accumulator = np.zeros((self.size, self.size), np.uint32)
        acc = accumulator
        if acc.dtype != np.uint32 or acc.shape != (self.size, self.size) or acc.strides[1] != 4 or acc.strides[0] % 4:
            raise ValueError(f"the accumulator is a {self.size} x {self.size} uint32 array with contiguous rows")
        d = img._desc()
        L.check(L.lib().zg_hough_compute_host(self._h, C.byref(d), l, t, r, b, C.c_void_p(acc.ctypes.data), max(acc.strides[0] // 4, self.size)))
        return acc

    def find_lines(self, accumulator, threshold: int, angle_nms_thresh: float, radius_nms_thresh: float) -> np.ndarray:
        """HoughTransform.findLines (:142-204): the reference's list as a HOUGH_LINE_DTYPE array. The call is repeated with more room
        when the candidates or the lines outnumber the first guess; more than 2^20 candidates raise ZignalError."""
        maxc, cap = _FIRST_CANDIDATES, 256
        while True:
            n_cand, n_lines, out = self._find_once(accumulator, threshold, angle_nms_thresh, radius_nms_thresh, maxc, cap)
            if n_cand > L.HOUGH_MAX_CANDIDATES:
                raise L.ZignalError(L.ERR_UNSUPPORTED, f"hough find_lines: {n_cand} candidates, more than {L.HOUGH_MAX_CANDIDATES}: raise the threshold")
            if n_cand > maxc:
                maxc = n_cand
            elif n_lines > cap:
                cap = n_lines
            else:
                return out[:n_lines].copy()

    def _find_once(self, accumulator, threshold, angle, radius, maxc: int, cap: int):
        if _is_torch(accumulator):
            dev = accumulator.device
            lines = torch.empty(cap * 28, dtype=torch.uint8, device=dev)
            counts = torch.zeros(2, dtype=torch.int32, device=dev)
            self.find_lines_into(accumulator, threshold, angle, radius, lines, counts, cap, maxc)
            c = counts.cpu().numpy().view(np.uint32)
            return int(c[0]), int(c[1]), lines[: min(int(c[1]), cap) * 28].cpu().numpy().view(HOUGH_LINE_DTYPE)
        acc = np.asarray(accumulator)
        if acc.dtype != np.uint32 or acc.shape != (self.size, self.size) or acc.strides[1] != 4 or acc.strides[0] % 4:
            raise ValueError(f"the accumulator is a {self.size} x {self.size} uint32 array with contiguous rows")
        thr = int(threshold)
        if not 0 <= thr < 1 << 32:
            raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"hough: threshold = {thr}")
        out = np.zeros(cap, HOUGH_LINE_DTYPE)
        counts = np.zeros(2, np.uint32)
        L.check(L.lib().zg_hough_find_lines_host(self._h, C.c_void_p(acc.ctypes.data), max(acc.strides[0] // 4, self.size), thr, float(angle), float(radius),
                                                 maxc, C.c_void_p(out.ctypes.data), cap, counts.ctypes.data_as(L._U32P)))
        return int(counts[0]), int(counts[1]), out[: min(int(counts[1]), cap)]

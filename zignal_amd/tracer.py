"""Tracer (reference src/features/Tracer.zig) over libzignal_hip.so's zg_trace_paths* entry points (include/zignal_hip_tracer.h): an
Image(u8) edge map (numpy on the host, a torch tensor on the device: what Image.canny / sobel / shen_castan return) to the reference's
list of polylines, bit for bit. The builder from a device list of paths to Canvas line commands is zignal_amd.canvas.cmds_from_paths."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _lib as L
from .image import Image, _is_torch

try:  # torch is plumbing (device memory + streams); the host flavour works without it
    import torch
except Exception:  # pragma: no cover
    torch = None


def scratch_bytes(rows: int, cols: int) -> int:
    """zg_trace_scratch_bytes: the scratch one trace of a rows x cols map takes."""
    return int(L.lib().zg_trace_scratch_bytes(int(rows), int(cols)))


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def split_paths(points: np.ndarray, path_offsets: np.ndarray) -> List[np.ndarray]:
    """The list of (k, 2) float32 arrays of (x, y) points that `points` and `path_offsets` hold."""
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    return [pts[int(a):int(b)].copy() for a, b in zip(path_offsets[:-1], path_offsets[1:])]


class Tracer:
    """Tracer (Tracer.zig:17-40): min_path_length is compared with a path's raw length; paths are simplified iff
    simplification_epsilon > 0."""

    def __init__(self, min_path_length: int = 5, simplification_epsilon: float = 1.0):
        self.min_path_length, self.simplification_epsilon = int(min_path_length), float(simplification_epsilon)

    def _c(self) -> L.ZgTracerOptions:
        if not 0 <= self.min_path_length < 1 << 32:
            raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"tracer: min_path_length = {self.min_path_length}")
        return L.ZgTracerOptions(self.min_path_length, self.simplification_epsilon)

    def __repr__(self):
        return f"Tracer(min_path_length={self.min_path_length}, simplification_epsilon={self.simplification_epsilon!r})"

    def trace_into(self, edges, points, path_offsets, counts, point_capacity: Optional[int] = None, path_capacity: Optional[int] = None) -> None:
        """zg_trace_paths on the current stream. `points` (a device tensor of at least point_capacity x 8 bytes, or None with capacity
        0), `path_offsets` (at least (path_capacity + 1) x 4 bytes) and `counts` (at least 16 bytes) are device tensors; the capacities
        default to what the tensors hold. Nothing is synchronised."""
        img = Image._wrap(edges)
        if not img.on_device or not all(_is_torch(t) and t.is_cuda for t in (path_offsets, counts) + (() if points is None else (points,))):
            raise ValueError("the _into forms take device tensors")
        pt_cap = (0 if points is None else _nbytes(points) // 8) if point_capacity is None else int(point_capacity)
        pa_cap = _nbytes(path_offsets) // 4 - 1 if path_capacity is None else int(path_capacity)
        if pa_cap < 0 or (pa_cap + 1) * 4 > _nbytes(path_offsets) or _nbytes(counts) < 16 or pt_cap * 8 > (0 if points is None else _nbytes(points)):
            raise ValueError("points, path_offsets or counts tensor too small")
        d, opt = img._desc(), self._c()
        with torch.cuda.device(img.data.device):
            L.check(L.lib().zg_trace_paths(C.byref(d), C.byref(opt), C.c_void_p(points.data_ptr()) if pt_cap else None, pt_cap,
                                           C.c_void_p(path_offsets.data_ptr()), pa_cap, C.c_void_p(counts.data_ptr()), img._stream()))

    def trace(self, edges) -> List[np.ndarray]:
        """Tracer.trace (:46-80): the reference's list of paths, each a (k, 2) float32 array of (x, y) points. Two calls: the first
        asks for the counts alone, the second has room for everything. Device edges are traced where they are; only the paths come back."""
        img = Image._wrap(edges)
        if img.on_device:
            dev = img.data.device
            counts = torch.zeros(4, dtype=torch.int32, device=dev)
            offsets = torch.zeros(1, dtype=torch.int32, device=dev)
            self.trace_into(img, None, offsets, counts, 0, 0)
            n_paths, n_points = (int(v) for v in counts.cpu().numpy().view(np.uint32)[:2])
            points = torch.zeros(max(n_points, 1) * 2, dtype=torch.float32, device=dev)
            offsets = torch.zeros(n_paths + 1, dtype=torch.int32, device=dev)
            self.trace_into(img, points, offsets, counts, n_points, n_paths)
            return split_paths(points[: 2 * n_points].cpu().numpy(), offsets.cpu().numpy().view(np.uint32))
        d, opt = img._desc(), self._c()
        counts = np.zeros(4, np.uint32)
        L.check(L.lib().zg_trace_paths_host(C.byref(d), C.byref(opt), None, 0, None, 0, counts.ctypes.data_as(L._U32P)))
        n_paths, n_points = int(counts[0]), int(counts[1])
        points, offsets = np.zeros((n_points, 2), np.float32), np.zeros(n_paths + 1, np.uint32)
        L.check(L.lib().zg_trace_paths_host(C.byref(d), C.byref(opt), C.c_void_p(points.ctypes.data) if n_points else None, n_points,
                                            C.c_void_p(offsets.ctypes.data), n_paths, counts.ctypes.data_as(L._U32P)))
        return split_paths(points, offsets)

"""BruteForceMatcher and MatchStats (reference src/features/matcher.zig) over libzignal_hip.so's zg_match_* entry points
(include/zignal_hip_match.h): Hamming matching of ORB's 32-byte descriptors, the reference's lists in the reference's order.

Descriptor sets are numpy BINARY_DESCRIPTOR_DTYPE arrays (the host path) or device uint8 tensors of 32 bytes per descriptor, each
with an optional device count tensor — the buffers and the count word Orb.detect_and_compute_into wrote, as they are."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import numpy as np

from . import _lib as L
from .image import BINARY_DESCRIPTOR_DTYPE, _is_torch

try:  # torch is plumbing (device memory + streams); the host flavour works without it
    import torch
except Exception:  # pragma: no cover
    torch = None

# Match (matcher.zig:10-19) as a numpy structured dtype: the bytes of zg_match.
MATCH_DTYPE = np.dtype([("query_idx", "<u4"), ("train_idx", "<u4"), ("distance", "<f4")])
assert MATCH_DTYPE.itemsize == C.sizeof(L.ZgMatch) == 12


def train_chunk() -> int:
    """The train descriptors the nearest-neighbour kernel stages at a time (zg_match_train_chunk)."""
    return int(L.lib().zg_match_train_chunk())


class MatchStats(NamedTuple):
    """MatchStats (matcher.zig:237-270)."""
    total_matches: int
    mean_distance: np.float32
    min_distance: np.float32
    max_distance: np.float32

    @classmethod
    def compute(cls, matches) -> "MatchStats":
        m = np.ascontiguousarray(matches, MATCH_DTYPE)
        out = L.ZgMatchStatistics()
        L.check(L.lib().zg_match_stats(m.ctypes.data if len(m) else None, len(m), C.byref(out)))
        return cls(int(out.total_matches), np.float32(out.mean_distance), np.float32(out.min_distance), np.float32(out.max_distance))


class _Set:
    """One side of a call: the zg_descriptor_set and what keeps its memory alive."""

    def __init__(self, descriptors, count, name: str):
        self.device = _is_torch(descriptors)
        if self.device:
            if descriptors.dtype != torch.uint8 or not descriptors.is_cuda or not descriptors.is_contiguous():
                raise ValueError(f"{name}: a contiguous device uint8 tensor of 32 bytes per descriptor")
            if count is not None and (not _is_torch(count) or not count.is_cuda or count.numel() * count.element_size() < 4):
                raise ValueError(f"{name}: the count is a device tensor of at least 4 bytes")
            self.keep = (descriptors, count)
            self.capacity = descriptors.numel() // 32
            self.desc = L.ZgDescriptorSet(descriptors.data_ptr() if self.capacity else None, self.capacity, count.data_ptr() if count is not None else None)
            self.torch_device = descriptors.device
        else:
            if count is not None:
                raise ValueError(f"{name}: a host array is taken whole; slice it instead of passing a count")
            arr = np.ascontiguousarray(descriptors, BINARY_DESCRIPTOR_DTYPE).reshape(-1)
            self.keep = (arr,)
            self.capacity = len(arr)
            self.desc = L.ZgDescriptorSet(arr.ctypes.data if len(arr) else None, len(arr), None)

    def size(self) -> int:
        """How many descriptors count (reads the device count word: synchronises)."""
        if self.device and self.keep[1] is not None:
            return min(int(self.keep[1].view(torch.uint8)[:4].cpu().numpy().view(np.uint32)[0]), self.capacity)
        return self.capacity


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


class BruteForceMatcher:
    """BruteForceMatcher (matcher.zig:33-41): same fields, same defaults. match returns a MATCH_DTYPE array, knn_match and
    radius_match a list of one MATCH_DTYPE array per query (an empty list when a side is empty, as the reference's)."""

    def __init__(self, cross_check: bool = False, max_distance: int = 64, ratio_threshold: float = 0.8):
        self.cross_check, self.max_distance, self.ratio_threshold = bool(cross_check), int(max_distance), float(ratio_threshold)

    def __repr__(self):
        return f"BruteForceMatcher(cross_check={self.cross_check}, max_distance={self.max_distance}, ratio_threshold={self.ratio_threshold})"

    def _params(self) -> "L.ZgMatcherParams":
        if not 0 <= self.max_distance < 1 << 32:
            raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"matcher: max_distance = {self.max_distance}")
        return L.ZgMatcherParams(int(self.cross_check), self.max_distance, self.ratio_threshold)

    @staticmethod
    def _sets(query, train, query_count, train_count):
        q, t = _Set(query, query_count, "query"), _Set(train, train_count, "train")
        if q.device != t.device:
            raise ValueError("query and train are both host arrays or both device tensors")
        return q, t

    @staticmethod
    def _stream(q: _Set):
        return C.c_void_p(torch.cuda.current_stream(q.torch_device).cuda_stream)

    @staticmethod
    def _device_sets(query, train, query_count, train_count, *outputs):
        q, t = BruteForceMatcher._sets(query, train, query_count, train_count)
        if not q.device or not all(_is_torch(o) and o.is_cuda for o in outputs):
            raise ValueError("the _into forms take device tensors")
        return q, t

    # ---- asynchronous device forms ------------------------------------------------------------------------------------
    def match_into(self, query, train, matches, count, capacity: Optional[int] = None, query_count=None, train_count=None) -> None:
        """zg_match_descriptors on the current stream: `matches` (a device tensor of at least capacity x 12 bytes; capacity defaults
        to what it holds) receives the first min(count, capacity) matches, `count` (at least 4 bytes) the full length as a u32.
        Nothing is synchronised."""
        q, t = self._device_sets(query, train, query_count, train_count, matches, count)
        cap = _nbytes(matches) // 12 if capacity is None else int(capacity)
        if cap * 12 > _nbytes(matches) or _nbytes(count) < 4:
            raise ValueError("matches or count tensor too small")
        p = self._params()
        with torch.cuda.device(q.torch_device):
            L.check(L.lib().zg_match_descriptors(C.byref(q.desc), C.byref(t.desc), C.byref(p), C.c_void_p(matches.data_ptr()) if cap else None, cap,
                                                 C.c_void_p(count.data_ptr()), self._stream(q)))

    def knn_match_into(self, query, train, k: int, matches, row_counts, query_count=None, train_count=None) -> None:
        """zg_match_knn on the current stream: row q at matches[q * k ..] (query capacity x k x 12 bytes), its length in
        row_counts[q] (query capacity u32 words)."""
        q, t = self._device_sets(query, train, query_count, train_count, matches, row_counts)
        k = int(k)
        if q.capacity * k * 12 > _nbytes(matches) or q.capacity * 4 > _nbytes(row_counts):
            raise ValueError("matches or row_counts tensor too small")
        p = self._params()
        with torch.cuda.device(q.torch_device):
            L.check(L.lib().zg_match_knn(C.byref(q.desc), C.byref(t.desc), C.byref(p), k, C.c_void_p(matches.data_ptr()), C.c_void_p(row_counts.data_ptr()),
                                         self._stream(q)))

    def radius_match_into(self, query, train, max_dist: float, matches, row_counts, count, capacity: Optional[int] = None, query_count=None,
                          train_count=None) -> None:
        """zg_match_radius on the current stream: the rows back to back in `matches` (the first min(count, capacity) entries), the
        full row lengths in row_counts (query capacity u32 words), their sum in `count`."""
        q, t = self._device_sets(query, train, query_count, train_count, matches, row_counts, count)
        cap = _nbytes(matches) // 12 if capacity is None else int(capacity)
        if cap * 12 > _nbytes(matches) or q.capacity * 4 > _nbytes(row_counts) or _nbytes(count) < 4:
            raise ValueError("matches, row_counts or count tensor too small")
        with torch.cuda.device(q.torch_device):
            L.check(L.lib().zg_match_radius(C.byref(q.desc), C.byref(t.desc), float(max_dist), C.c_void_p(matches.data_ptr()) if cap else None, cap,
                                            C.c_void_p(row_counts.data_ptr()), C.c_void_p(count.data_ptr()), self._stream(q)))

    # ---- the reference's calls ----------------------------------------------------------------------------------------
    def match(self, query, train, query_count=None, train_count=None) -> np.ndarray:
        """BruteForceMatcher.match (:44-106). Host arrays go through zg_match_descriptors_host, device tensors through
        zg_match_descriptors on the current stream (synchronised to read the count)."""
        q, t = self._sets(query, train, query_count, train_count)
        cap = q.capacity  # a match per query at the most
        if not q.device:
            out = np.empty(cap, MATCH_DTYPE)
            n, p = C.c_uint32(), self._params()
            L.check(L.lib().zg_match_descriptors_host(C.byref(q.desc), C.byref(t.desc), C.byref(p), out.ctypes.data if cap else None, cap, C.byref(n)))
            return out[: n.value].copy()
        matches = torch.empty(max(cap, 1) * 12, dtype=torch.uint8, device=q.torch_device)
        count = torch.zeros(1, dtype=torch.int32, device=q.torch_device)
        self.match_into(query, train, matches, count, cap, query_count, train_count)
        n = int(count.item())
        return matches[: n * 12].cpu().numpy().view(MATCH_DTYPE).copy()

    def knn_match(self, query, train, k: int, query_count=None, train_count=None) -> List[np.ndarray]:
        """BruteForceMatcher.knnMatch (:109-162)."""
        q, t = self._sets(query, train, query_count, train_count)
        k = int(k)
        nq, nt = q.size(), t.size()
        if nq == 0 or nt == 0 or k == 0:
            return []
        if not q.device:
            out = np.empty(nq * k, MATCH_DTYPE)
            rows = np.zeros(nq, np.uint32)
            p = self._params()
            L.check(L.lib().zg_match_knn_host(C.byref(q.desc), C.byref(t.desc), C.byref(p), k, out.ctypes.data, rows.ctypes.data))
        else:
            matches = torch.empty(q.capacity * k * 12, dtype=torch.uint8, device=q.torch_device)
            row_counts = torch.zeros(q.capacity, dtype=torch.int32, device=q.torch_device)
            self.knn_match_into(query, train, k, matches, row_counts, query_count, train_count)
            rows = row_counts.cpu().numpy().view(np.uint32)
            out = matches.cpu().numpy().view(MATCH_DTYPE)
        return [out[i * k: i * k + int(rows[i])].copy() for i in range(nq)]

    def radius_match(self, query, train, max_dist: float, query_count=None, train_count=None) -> List[np.ndarray]:
        """BruteForceMatcher.radiusMatch (:165-212). The call runs twice: once for the row lengths, once with room for their sum."""
        q, t = self._sets(query, train, query_count, train_count)
        nq, nt = q.size(), t.size()
        if nq == 0 or nt == 0:
            return []
        if not q.device:
            rows = np.zeros(q.capacity, np.uint32)
            n = C.c_uint32()
            L.check(L.lib().zg_match_radius_host(C.byref(q.desc), C.byref(t.desc), float(max_dist), None, 0, rows.ctypes.data, C.byref(n)))
            out = np.empty(n.value, MATCH_DTYPE)
            if n.value:
                L.check(L.lib().zg_match_radius_host(C.byref(q.desc), C.byref(t.desc), float(max_dist), out.ctypes.data, n.value, rows.ctypes.data, C.byref(n)))
        else:
            dev = q.torch_device
            row_counts = torch.zeros(q.capacity, dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            matches = torch.empty(12, dtype=torch.uint8, device=dev)
            self.radius_match_into(query, train, max_dist, matches, row_counts, count, 0, query_count, train_count)
            n = int(count.cpu().numpy().view(np.uint32)[0])
            matches = torch.empty(max(n, 1) * 12, dtype=torch.uint8, device=dev)
            if n:
                self.radius_match_into(query, train, max_dist, matches, row_counts, count, n, query_count, train_count)
            rows = row_counts.cpu().numpy().view(np.uint32)
            out = matches[: n * 12].cpu().numpy().view(MATCH_DTYPE)
        ends = np.cumsum(rows[:nq].astype(np.int64))
        return [out[int(e) - int(r): int(e)].copy() for e, r in zip(ends, rows[:nq])]

"""SimilarityTransform.find, AffineTransform.find and ProjectiveTransform.find (reference src/geometry/transforms.zig:47-112, :155-191,
:242-290) through the zg_transform_* entry points (include/zignal_hip_transform.h).

On device tensors every call is asynchronous on the current stream and nothing is copied or synchronised: a fit leaves a 128-byte
zg_transform_fit in device memory, and warp_fitted resamples with the matrix read from there, so ORB twice, match, fit and warp are one
enqueued chain. On host arrays the same arithmetic runs on the CPU (the _host forms), no GPU needed. Results are the reference's bit for
bit, except AffineTransform.find on 86 or more points, where the reference's own value depends on its build (the header says why)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from .image import Image, Interpolation, _is_torch

SIMILARITY, AFFINE, PROJECTIVE = L.TRANSFORM_SIMILARITY, L.TRANSFORM_AFFINE, L.TRANSFORM_PROJECTIVE
FIT_DTYPE = np.dtype([("kind", "<i4"), ("status", "<i4"), ("n_points", "<u4"), ("svd_converged", "<u4"), ("m64", "<f8", (9,)), ("m32", "<f4", (9,)),
                      ("reserved", "<u4")])
assert FIT_DTYPE.itemsize == C.sizeof(L.ZgTransformFit) == 128
_SCALARS = {np.dtype(np.float32): L.SCALAR_F32, np.dtype(np.float64): L.SCALAR_F64}
_STATUS_NAMES = {L.FIT_NOT_CONVERGED: "NotConverged", L.FIT_RANK_DEFICIENT: "RankDeficient", L.FIT_BAD_COUNT: "BadCount", L.FIT_BAD_INPUT: "BadInput"}


class FitError(RuntimeError):
    """A fit whose record is not ZG_FIT_OK: error.NotConverged, error.RankDeficient, or a count or an index out of bounds."""

    def __init__(self, status: int):
        super().__init__(_STATUS_NAMES.get(status, f"status {status}"))
        self.status = status


def chunk() -> int:
    """zg_transform_chunk: the points one stage of the device's ordered sums takes."""
    return int(L.lib().zg_transform_chunk())


def _scalar_of(scalar) -> int:
    """ZG_SCALAR_* of an ordinal or of anything numpy takes for a dtype."""
    if isinstance(scalar, int):
        if scalar not in (L.SCALAR_F32, L.SCALAR_F64):
            raise ValueError("scalar is ZG_SCALAR_F32 or ZG_SCALAR_F64")
        return scalar
    return _SCALARS[np.dtype(scalar)]


def _torch_scalar(t) -> int:
    import torch
    if t.dtype == torch.float32:
        return L.SCALAR_F32
    if t.dtype == torch.float64:
        return L.SCALAR_F64
    raise ValueError("points are float32 or float64")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def new_record(device="cuda"):
    """Room for one zg_transform_fit in device memory."""
    import torch
    return torch.empty(128, dtype=torch.uint8, device=device)


def record_to_host(record) -> np.ndarray:
    """A device record read back as a FIT_DTYPE scalar (synchronises)."""
    return np.frombuffer(record.cpu().numpy().tobytes(), FIT_DTYPE)[0]


def upload_record(record, device="cuda"):
    """A FIT_DTYPE record (or a ZgTransformFit) as a device tensor of its bytes."""
    import torch
    raw = bytes(record) if isinstance(record, L.ZgTransformFit) else np.asarray(record, FIT_DTYPE).tobytes()
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(device)


def _host_record(rec: L.ZgTransformFit) -> np.ndarray:
    return np.frombuffer(bytes(rec), FIT_DTYPE)[0]


def fit_points_into(kind: int, from_points, to_points, record, count=None, capacity: Optional[int] = None) -> None:
    """zg_transform_fit_points on the current stream: from_points and to_points are device tensors of shape (capacity, 2) in float32 or
    float64 (the type the fit runs in), `count` an optional device tensor holding a u32, `record` a device tensor of at least 128 bytes."""
    import torch
    if not (_is_torch(from_points) and from_points.is_cuda and _is_torch(to_points) and to_points.is_cuda and _is_torch(record) and record.is_cuda):
        raise ValueError("fit_points_into takes device tensors")
    if from_points.dtype != to_points.dtype or not from_points.is_contiguous() or not to_points.is_contiguous():
        raise ValueError("from and to are contiguous tensors of one scalar type")
    cap = from_points.numel() // 2 if capacity is None else int(capacity)
    if cap * 2 > from_points.numel() or cap * 2 > to_points.numel() or record.numel() * record.element_size() < 128:
        raise ValueError("points or record tensor too small")
    dev = record.device
    with torch.cuda.device(dev):
        L.check(L.lib().zg_transform_fit_points(int(kind), _torch_scalar(from_points), _ptr(from_points), _ptr(to_points), cap, _ptr(count), _ptr(record),
                                                _stream(dev)))


def fit_matches_into(kind: int, scalar, query_kps, train_kps, matches, record, count=None, capacity: Optional[int] = None, train_to_query: bool = False,
                     n_query: Optional[int] = None, n_train: Optional[int] = None) -> None:
    """zg_transform_fit_matches on the current stream: keypoint tensors of 28 bytes an entry, a match tensor of 12 bytes an entry, the
    count word zg_match_descriptors wrote. train_to_query: the map zg_warp needs to bring the query frame onto the train frame's grid."""
    import torch
    for t in (query_kps, train_kps, matches, record):
        if not (_is_torch(t) and t.is_cuda):
            raise ValueError("fit_matches_into takes device tensors")
    nbytes = lambda t: t.numel() * t.element_size()  # noqa: E731
    nq = nbytes(query_kps) // 28 if n_query is None else int(n_query)
    nt = nbytes(train_kps) // 28 if n_train is None else int(n_train)
    cap = nbytes(matches) // 12 if capacity is None else int(capacity)
    if nq * 28 > nbytes(query_kps) or nt * 28 > nbytes(train_kps) or cap * 12 > nbytes(matches) or nbytes(record) < 128:
        raise ValueError("keypoints, matches or record tensor too small")
    dev = record.device
    with torch.cuda.device(dev):
        L.check(L.lib().zg_transform_fit_matches(int(kind), _scalar_of(scalar), _ptr(query_kps), nq, _ptr(train_kps), nt, _ptr(matches), cap, _ptr(count),
                                                 1 if train_to_query else 0, _ptr(record), _stream(dev)))


def fit_points_host(kind: int, from_points, to_points, scalar=None, count: Optional[int] = None) -> np.ndarray:
    """zg_transform_fit_points_host: the record (a FIT_DTYPE scalar) of a fit on host arrays of shape (n, 2). Host arithmetic."""
    f = np.asarray(from_points)
    dt = np.dtype(np.float32 if _scalar_of(scalar) == L.SCALAR_F32 else np.float64) if scalar is not None else (f.dtype if f.dtype in _SCALARS else np.dtype(np.float64))
    f = np.ascontiguousarray(f, dt).reshape(-1, 2)
    t = np.ascontiguousarray(to_points, dt).reshape(-1, 2)
    if len(f) != len(t):
        raise ValueError("from and to have one length")
    out = L.ZgTransformFit()
    cnt = C.c_uint32(count) if count is not None else None
    L.check(L.lib().zg_transform_fit_points_host(int(kind), _SCALARS[dt], f.ctypes.data, t.ctypes.data, len(f), C.byref(cnt) if cnt is not None else None,
                                                 C.byref(out)))
    return _host_record(out)


def fit_matches_host(kind: int, scalar, query_kps, train_kps, matches, count: Optional[int] = None, train_to_query: bool = False) -> np.ndarray:
    """zg_transform_fit_matches_host on host arrays (KEYPOINT_DTYPE, MATCH_DTYPE or their bytes)."""
    q = np.ascontiguousarray(query_kps).view(np.uint8).reshape(-1)
    t = np.ascontiguousarray(train_kps).view(np.uint8).reshape(-1)
    m = np.ascontiguousarray(matches).view(np.uint8).reshape(-1)
    out = L.ZgTransformFit()
    cnt = C.c_uint32(count) if count is not None else None
    L.check(L.lib().zg_transform_fit_matches_host(int(kind), _scalar_of(scalar), q.ctypes.data if q.size else None, q.size // 28, t.ctypes.data if t.size else None,
                                                  t.size // 28, m.ctypes.data if m.size else None, m.size // 12, C.byref(cnt) if cnt is not None else None,
                                                  1 if train_to_query else 0, C.byref(out)))
    return _host_record(out)


def _as_struct(record) -> L.ZgTransformFit:
    return record if isinstance(record, L.ZgTransformFit) else L.ZgTransformFit.from_buffer_copy(np.asarray(record, FIT_DTYPE).tobytes())


def project_points(record, points, out=None):
    """project of (n, 2) points with a record's matrix, in the points' scalar type: device tensors with a device record (asynchronous),
    host arrays with a host record."""
    if _is_torch(points):
        import torch
        if out is None:
            out = torch.empty_like(points)
        n = points.numel() // 2
        dev = points.device
        with torch.cuda.device(dev):
            L.check(L.lib().zg_transform_project_points(_ptr(record), _torch_scalar(points), _ptr(points), _ptr(out), n, _stream(dev)))
        return out
    p = np.ascontiguousarray(points)
    if p.dtype not in _SCALARS:
        p = p.astype(np.float64)
    res = np.empty_like(p)
    rec = _as_struct(record)
    L.check(L.lib().zg_transform_project_points_host(C.byref(rec), _SCALARS[p.dtype], p.ctypes.data, res.ctypes.data, p.size // 2))
    return res


def invert(record, scalar, out=None):
    """ProjectiveTransform.inv of a record: a device record into a device record (asynchronous), or a host record into a host record."""
    if _is_torch(record):
        import torch
        if out is None:
            out = torch.empty_like(record)
        dev = record.device
        with torch.cuda.device(dev):
            L.check(L.lib().zg_transform_invert(_ptr(record), _scalar_of(scalar), _ptr(out), _stream(dev)))
        return out
    rec, res = _as_struct(record), L.ZgTransformFit()
    L.check(L.lib().zg_transform_invert_host(C.byref(rec), _scalar_of(scalar), C.byref(res)))
    return _host_record(res)


def warp_fitted(src: Image, record, shape_or_out=None, method: Interpolation = Interpolation.bilinear) -> Image:
    """zg_warp_fitted: Image.warp of a device image with the kind and m32 of a device record. A record that is not ZG_FIT_OK leaves the
    output untouched."""
    import torch
    src = Image._wrap(src)
    if not src.on_device:
        raise ValueError("warp_fitted takes a device image")
    if shape_or_out is None:
        out = src._like()
    elif isinstance(shape_or_out, Image):
        out = shape_or_out
    else:
        out = src._like(int(shape_or_out[0]), int(shape_or_out[1]))
    src._same_side(out)
    s, d, m = src._desc(), out._desc(), method._c()
    dev = src.data.device
    with torch.cuda.device(dev):
        L.check(L.lib().zg_warp_fitted(C.byref(s), C.byref(d), _ptr(record), C.byref(m), _stream(dev)))
    return out


class FittedTransform:
    """The outcome of find for one kind: .matrix (2 x 2 or 3 x 3) and .bias as the reference's fields, .coefficients() as zg_warp
    takes them, so Image.warp accepts it."""

    def __init__(self, record: np.ndarray, scalar: int):
        if int(record["status"]) != L.FIT_OK:
            raise FitError(int(record["status"]))
        self.record = record
        self.kind = int(record["kind"])
        m = np.array(record["m32"] if scalar == L.SCALAR_F32 else record["m64"])
        if self.kind == PROJECTIVE:
            self.matrix, self.bias = m.reshape(3, 3), None
        else:
            self.matrix, self.bias = m[:4].reshape(2, 2), m[4:6].copy()

    def coefficients(self):
        return [float(v) for v in (self.record["m32"] if self.kind == PROJECTIVE else self.record["m32"][:6])]

    def project(self, points):
        return project_points(self.record, points)


def find(kind: int, from_points, to_points, scalar=np.float64) -> FittedTransform:
    """SimilarityTransform(T).init / AffineTransform(T).init / ProjectiveTransform(T).init on host points: raises FitError where the
    reference returns an error."""
    s = _scalar_of(scalar)
    return FittedTransform(fit_points_host(kind, from_points, to_points, scalar=s), s)

"""FeatureDistributionMatching (reference src/fdm.zig) through the zg_fdm_* entry points (include/zignal_hip_fdm.h): the colour statistics
(mean and 3 x 3 covariance) of a target image moved onto a source image, in place, for u8, Rgb(u8) and Rgba(u8) images.

On device images every step is asynchronous on the current stream and nothing is copied or synchronised: set_target leaves a 136-byte
zg_fdm_target in device memory, update runs moments, transform and apply on the source. The statistics come from exact integer moments,
not from the reference's Welford recurrence (the header says what that can change: a byte whose value before rounding is a tie)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .image import Image

_PIXELS = (L.PIXEL_U8, L.PIXEL_RGB_U8, L.PIXEL_RGBA_U8)


class NoTargetSet(RuntimeError):
    """error.NoTargetSet (fdm.zig:142)."""


class NoSourceSet(RuntimeError):
    """error.NoSourceSet (fdm.zig:143)."""


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_pixel(image: Image, what: str) -> None:
    if image.pixel not in _PIXELS:
        raise L.ZignalError(L.ERR_UNSUPPORTED, f"{what}: feature distribution matching takes u8, Rgb(u8) and Rgba(u8) images (fdm.zig:20)")


def _descs(frames: Sequence[Image]):
    arr = (L.ZgImage * len(frames))()
    for i, f in enumerate(frames):
        arr[i] = f._desc()
    return arr


def _records(struct, n: int, device):
    import torch
    return torch.empty(n * C.sizeof(struct), dtype=torch.uint8, device=device)


def _to_host(tensor, struct, n: int):
    """n records of a device tensor as a ctypes array (synchronises)."""
    raw = tensor.cpu().numpy().tobytes()
    return (struct * n).from_buffer_copy(raw)


def compute_moments(frames, out=None):
    """zg_fdm_compute_moments(_frames): the integer moments of one device image or a list of them, as a device tensor of 104 bytes a
    frame (fdm.moments_to_host reads them back)."""
    import torch
    single = isinstance(frames, Image)
    frames = [frames] if single else list(frames)
    if not frames:
        raise ValueError("no frames")
    dev = frames[0].data.device
    for f in frames:
        if not f.on_device or f.data.device != dev:
            raise ValueError("compute_moments takes device images on one device")
    if out is None:
        out = _records(L.ZgFdmMoments, len(frames), dev)
    d = _descs(frames)
    with torch.cuda.device(dev):
        if single:
            L.check(L.lib().zg_fdm_compute_moments(C.byref(d[0]), C.c_void_p(out.data_ptr()), _stream(dev)))
        else:
            L.check(L.lib().zg_fdm_compute_moments_frames(d, len(frames), C.c_void_p(out.data_ptr()), _stream(dev)))
    return out


def moments_to_host(tensor, n: int = 1):
    return _to_host(tensor, L.ZgFdmMoments, n)


def target_host(pixel: int, mean, cov, is_gray: bool) -> L.ZgFdmTarget:
    """zg_fdm_target_host: setTarget from statistics given as f64 (mean[3], cov 3 x 3). Host arithmetic, no GPU needed."""
    m = np.ascontiguousarray(mean, np.float64).reshape(3)
    c = np.ascontiguousarray(cov, np.float64).reshape(9)
    out = L.ZgFdmTarget()
    L.check(L.lib().zg_fdm_target_host(int(pixel), m.ctypes.data_as(L._F64P), c.ctypes.data_as(L._F64P), 1 if is_gray else 0, C.byref(out)))
    return out


def transform_host(pixel: int, target: L.ZgFdmTarget, mean, cov) -> L.ZgFdmTransform:
    """zg_fdm_transform_host: update between the statistics and the pixels. Host arithmetic, no GPU needed."""
    m = np.ascontiguousarray(mean, np.float64).reshape(3)
    c = np.ascontiguousarray(cov, np.float64).reshape(9)
    out = L.ZgFdmTransform()
    L.check(L.lib().zg_fdm_transform_host(int(pixel), C.byref(target), m.ctypes.data_as(L._F64P), c.ctypes.data_as(L._F64P), C.byref(out)))
    return out


def stats_from_moments(moments: L.ZgFdmMoments, luminance: bool):
    """zg_fdm_stats_from_moments_host: (mean[3], cov[3][3]) as the device kernels derive them from the moments."""
    m, c = np.zeros(3), np.zeros(9)
    L.check(L.lib().zg_fdm_stats_from_moments_host(C.byref(moments), 1 if luminance else 0, m.ctypes.data_as(L._F64P), c.ctypes.data_as(L._F64P)))
    return m, c.reshape(3, 3)


def upload(record, device="cuda"):
    """A zg_fdm_target / zg_fdm_transform (or a ctypes array of them) as a device tensor of its bytes."""
    import torch
    return torch.from_numpy(np.frombuffer(bytes(record), np.uint8).copy()).to(device)


def apply(frames, transforms):
    """zg_fdm_apply(_frames): the per-pixel map, in place, on one device image or a list; `transforms` is a device tensor of 120 bytes a
    frame."""
    import torch
    single = isinstance(frames, Image)
    frames = [frames] if single else list(frames)
    dev = frames[0].data.device
    if transforms.numel() < len(frames) * C.sizeof(L.ZgFdmTransform):
        raise ValueError("one zg_fdm_transform a frame")
    d = _descs(frames)
    with torch.cuda.device(dev):
        if single:
            L.check(L.lib().zg_fdm_apply(C.byref(d[0]), C.c_void_p(transforms.data_ptr()), _stream(dev)))
        else:
            L.check(L.lib().zg_fdm_apply_frames(d, len(frames), C.c_void_p(transforms.data_ptr()), _stream(dev)))
    return frames[0] if single else frames


class FeatureDistributionMatching:
    """FeatureDistributionMatching(T) with the reference's state machine (fdm.zig:19-274): set_target once, then set_source and update for
    every frame; match does the three at once; match_frames serves a list against one target in one chain."""

    def __init__(self):
        self._target: Optional[Image] = None
        self._prepared = None  # device tensor holding the zg_fdm_target
        self._source: Optional[Image] = None

    @property
    def has_target(self) -> bool:
        return self._target is not None

    @property
    def has_source(self) -> bool:
        return self._source is not None

    def set_target(self, image: Image) -> "FeatureDistributionMatching":
        """setTarget: the target's statistics, computed once. A device image leaves them in device memory (asynchronous); a host image is
        kept and staged by update."""
        import torch
        image = Image._wrap(image)
        _check_pixel(image, "set_target")
        self._prepared = None
        if image.on_device:
            dev = image.data.device
            m = compute_moments(image)
            t = _records(L.ZgFdmTarget, 1, dev)
            with torch.cuda.device(dev):
                L.check(L.lib().zg_fdm_target_from_moments(C.c_void_p(m.data_ptr()), C.c_void_p(t.data_ptr()), _stream(dev)))
            self._prepared = t
        self._target = image
        return self

    def target_record(self) -> L.ZgFdmTarget:
        """The prepared zg_fdm_target of a device target, read back (synchronises)."""
        if self._prepared is None:
            raise NoTargetSet("no device target set")
        return _to_host(self._prepared, L.ZgFdmTarget, 1)[0]

    def set_source(self, image: Image) -> "FeatureDistributionMatching":
        image = Image._wrap(image)
        _check_pixel(image, "set_source")
        self._source = image
        return self

    def update(self) -> Image:
        """update: the source matched to the target, in place."""
        if self._target is None:
            raise NoTargetSet("update before set_target (error.NoTargetSet)")
        if self._source is None:
            raise NoSourceSet("update before set_source (error.NoSourceSet)")
        self.match_frames([self._source])
        return self._source

    def match(self, source: Image, target: Image) -> Image:
        self.set_target(target)
        self.set_source(source)
        return self.update()

    def match_frames(self, frames: Sequence[Image], target: Optional[Image] = None):
        """zg_fdm_match_frames: every frame matched in place against `target` (set first when given) or the target set before."""
        import torch
        if target is not None:
            self.set_target(target)
        if self._target is None:
            raise NoTargetSet("match_frames before set_target (error.NoTargetSet)")
        frames = [Image._wrap(f) for f in frames]
        if not frames:
            return frames
        for f in frames:
            _check_pixel(f, "match_frames")
            f._same_side(self._target)
            if f.pixel != self._target.pixel:
                raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"the frame's pixel type {f.pixel} is not the target's {self._target.pixel}")
        d = _descs(frames)
        if self._target.on_device:
            dev = self._target.data.device
            with torch.cuda.device(dev):
                L.check(L.lib().zg_fdm_match_frames(d, len(frames), None, C.c_void_p(self._prepared.data_ptr()), _stream(dev)))
        else:
            t = self._target._desc()
            L.check(L.lib().zg_fdm_match_frames_host(d, len(frames), C.byref(t)))
        return frames

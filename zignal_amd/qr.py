"""The QR detector (reference src/qrcode/detector.zig:57-641) over libzignal_hip.so's zg_qr_* entry points (include/zignal_hip_qr.h): a
frame (numpy on the host, a torch tensor on the device) to the sampled module grids and their corners, which are what the reference hands to
decoder.decodeModules, in the reference's order of trial, bit for bit. Decoding the grids is host work and not part of this package.
The builder from a device list of grids to Canvas line commands is zignal_amd.canvas.cmds_from_qr."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib as L
from .image import Image, _is_torch

try:  # torch is plumbing (device memory + streams); the host flavour works without it
    import torch
except Exception:  # pragma: no cover
    torch = None

FOURTH_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("is_alignment", "<u4")])
DETECTION_DTYPE = np.dtype([("finders", "<f4", (64, 4)), ("finder_count", "<u4"), ("merged_count", "<u4"), ("triple_found", "<u4"),
                            ("triple", "<f4", (3, 4)), ("version_estimate", "<u4"), ("version_count", "<u4"), ("versions", "u1", (8,)),
                            ("fourth_count", "<u4"), ("fourths", FOURTH_DTYPE, (5,)), ("grids_total", "<u4"), ("grids_written", "<u4"),
                            ("modules_written", "<u4")])
GRID_DTYPE = np.dtype([("version", "<u4"), ("dim", "<u4"), ("fourth_index", "<u4"), ("modules_offset", "<u4"), ("version_hint", "<i4"),
                       ("corners", "<f4", (8,)), ("reserved", "<u4"), ("transform", "<f8", (9,))])
assert DETECTION_DTYPE.itemsize == C.sizeof(L.ZgQrDetection) and GRID_DTYPE.itemsize == C.sizeof(L.ZgQrGrid)

ADAPTIVE, OTSU, BINARY = L.QR_ADAPTIVE, L.QR_OTSU, L.QR_BINARY


def scratch_bytes(rows: int, cols: int) -> int:
    """zg_qr_scratch_bytes: the scratch one detection on a rows x cols frame takes."""
    return int(L.lib().zg_qr_scratch_bytes(int(rows), int(cols)))


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


@dataclass
class QrGrid:
    """One trial of the reference's loops (detector.zig:126-153) that passed the timing check and sampleGrid."""
    binarize: int            # the pass that produced it: ADAPTIVE, OTSU or BINARY
    version: int
    fourth_index: int        # into the detection's fourth-correspondence candidates
    version_hint: int        # decoder.readVersion of this grid for version >= 7, else -1
    corners: np.ndarray      # (4, 2) float32 (x, y): top left, top right, bottom left, bottom right (symbolCorners)
    transform: np.ndarray    # (3, 3) float64, module space to image space
    modules: np.ndarray      # (dim, dim) uint8, 0 or 1


def split_grids(grids: np.ndarray, modules: np.ndarray, binarize: int) -> List[QrGrid]:
    """The QrGrid list that GRID_DTYPE records and their module bytes hold."""
    out = []
    for g in grids:
        dim, off = int(g["dim"]), int(g["modules_offset"])
        out.append(QrGrid(binarize, int(g["version"]), int(g["fourth_index"]), int(g["version_hint"]), g["corners"].reshape(4, 2).copy(),
                          g["transform"].reshape(3, 3).copy(), modules[off:off + dim * dim].reshape(dim, dim).copy()))
    return out


class QrDetector:
    """detectAndDecode (detector.zig:86-156) up to the decoder."""

    def detect_into(self, image, detection, grids, modules, binarize: int = ADAPTIVE, grid_capacity: Optional[int] = None,
                    module_capacity: Optional[int] = None) -> None:
        """zg_qr_detect on the current stream. `detection` (a device tensor of at least DETECTION_DTYPE.itemsize bytes), `grids` (at least
        grid_capacity x GRID_DTYPE.itemsize bytes, or None with capacity 0) and `modules` (at least module_capacity bytes, or None) are
        device tensors; the capacities default to what the tensors hold. Nothing is synchronised."""
        img = Image._wrap(image)
        given = tuple(t for t in (detection, grids, modules) if t is not None)
        if not img.on_device or detection is None or not all(_is_torch(t) and t.is_cuda for t in given):
            raise ValueError("the _into forms take device tensors")
        g_cap = (0 if grids is None else _nbytes(grids) // GRID_DTYPE.itemsize) if grid_capacity is None else int(grid_capacity)
        m_cap = (0 if modules is None else _nbytes(modules)) if module_capacity is None else int(module_capacity)
        if (_nbytes(detection) < DETECTION_DTYPE.itemsize or g_cap * GRID_DTYPE.itemsize > (0 if grids is None else _nbytes(grids))
                or m_cap > (0 if modules is None else _nbytes(modules))):
            raise ValueError("detection, grids or modules tensor too small")
        d = img._desc()
        with torch.cuda.device(img.data.device):
            L.check(L.lib().zg_qr_detect(C.byref(d), int(binarize), C.c_void_p(detection.data_ptr()), C.c_void_p(grids.data_ptr()) if g_cap else None, g_cap,
                                         C.c_void_p(modules.data_ptr()) if m_cap else None, m_cap, img._stream()))

    def detect_pass(self, image, binarize: int):
        """One binarisation: (detection record as a DETECTION_DTYPE scalar, [QrGrid]). Two calls: the first asks for the counts alone,
        the second has room for everything. A device frame is searched where it is; only the grids come back."""
        img = Image._wrap(image)
        if img.on_device:
            dev = img.data.device
            det = torch.zeros(DETECTION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            self.detect_into(img, det, None, None, binarize, 0, 0)
            n = int(det.cpu().numpy().view(DETECTION_DTYPE)[0]["grids_total"])
            grids = torch.zeros(max(n, 1) * GRID_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            modules = torch.zeros(max(n, 1) * L.QR_MAX_MODULES, dtype=torch.uint8, device=dev)
            self.detect_into(img, det, grids, modules, binarize, n, n * L.QR_MAX_MODULES)
            record = det.cpu().numpy().view(DETECTION_DTYPE)[0]
            return record, split_grids(grids.cpu().numpy().view(GRID_DTYPE)[:int(record["grids_written"])], modules.cpu().numpy(), binarize)
        d = img._desc()
        det = L.ZgQrDetection()
        L.check(L.lib().zg_qr_detect_host(C.byref(d), int(binarize), C.byref(det), None, 0, None, 0))
        n = int(det.grids_total)
        grids, modules = np.zeros(max(n, 1), GRID_DTYPE), np.zeros(max(n, 1) * L.QR_MAX_MODULES, np.uint8)
        L.check(L.lib().zg_qr_detect_host(C.byref(d), int(binarize), C.byref(det), C.c_void_p(grids.ctypes.data), n, C.c_void_p(modules.ctypes.data),
                                          n * L.QR_MAX_MODULES))
        record = np.frombuffer(bytes(det), DETECTION_DTYPE)[0]
        return record, split_grids(grids[:int(det.grids_written)], modules, binarize)

    def detect(self, image) -> List[QrGrid]:
        """The grids of the adaptive pass followed by those of the Otsu pass (detector.zig:71-82), each tagged with its pass. The
        reference runs the second pass only when nothing of the first decoded; a decoder walking this list in order reproduces it."""
        return self.detect_pass(image, ADAPTIVE)[1] + self.detect_pass(image, OTSU)[1]

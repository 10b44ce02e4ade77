"""Image(T).psnr / ssim / meanPixelError's host-side pieces (reference src/image/metrics.zig) and the exact sequential f64 sum they end in
(include/zignal_hip_metrics.h). The metrics themselves are Image.psnr, Image.ssim and Image.mean_pixel_error (zignal_amd/image.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

# zg_metric_result as a numpy record: a result tensor of four 64-bit words read back from the device is `.view(METRIC_RESULT_DTYPE)`
METRIC_RESULT_DTYPE = np.dtype([("sum", "<f8"), ("count", "<u8"), ("value", "<f8"), ("serial_terms", "<u8")])
METRIC_RESULT_BYTES = 32


def sum_f64_chunk() -> int:
    """The terms in one chunk of the sequential sum by default (zg_sum_f64_chunk)."""
    return int(L.lib().zg_sum_f64_chunk())


def ssim_window() -> np.ndarray:
    """generateSsimWindow (metrics.zig:230-249) as the library builds it: (11, 11) f64. Host arithmetic, no GPU needed."""
    w = np.empty(121, np.float64)
    L.check(L.lib().zg_ssim_window_host(w.ctypes.data_as(C.POINTER(C.c_double))))
    return w.reshape(11, 11)


def psnr_from_mse(mse: float, max_value: float) -> float:
    """20 log10(max_value) - 10 log10(mse), inf for mse == 0 (metrics.zig:49-53), with the library's own log10."""
    return float(L.lib().zg_psnr_from_mse(float(mse), float(max_value)))


def _is_result_tensor(t, device) -> bool:
    return (hasattr(t, "is_cuda") and t.is_cuda and t.device == device and t.is_contiguous() and t.numel() * t.element_size() >= METRIC_RESULT_BYTES
            and t.data_ptr() % 8 == 0)


def _record(t) -> np.void:
    """A result tensor's first 32 bytes as one METRIC_RESULT_DTYPE record (synchronises)."""
    import torch
    raw = t.view(torch.uint8).reshape(-1)[:METRIC_RESULT_BYTES].cpu().numpy()
    return raw.view(METRIC_RESULT_DTYPE)[0]


def sum_f64_sequential(values, chunk_log2: int = 0, result=None):
    """zg_sum_f64_sequential: the left-to-right f64 sum of a contiguous float64 device tensor, bit for bit. Without `result`: one
    synchronisation, returns the METRIC_RESULT_DTYPE record (sum, count, value, serial_terms). With `result` (a contiguous device tensor of
    at least 32 bytes): asynchronous on the current stream, fills and returns it."""
    import torch
    if not (hasattr(values, "is_cuda") and values.is_cuda and values.dtype == torch.float64 and values.is_contiguous()):
        raise ValueError("values is a contiguous float64 tensor on the device")
    own = result is None
    if own:
        result = torch.empty(4, dtype=torch.float64, device=values.device)
    elif not _is_result_tensor(result, values.device):
        raise ValueError("result is a contiguous, 8-byte aligned tensor of at least 32 bytes on the values' device")
    with torch.cuda.device(values.device):
        stream = C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream)
        L.check(L.lib().zg_sum_f64_sequential(C.c_void_p(values.data_ptr() if values.numel() else 0), values.numel(), int(chunk_log2),
                                              C.c_void_p(result.data_ptr()), stream))
    return _record(result) if own else result

"""Image(T).floodFill's options (reference src/image/flood_fill.zig:5-26) and the host-side constant of the zg_flood_fill* entry points
(include/zignal_hip_flood.h). The fill itself is Image.flood_fill (zignal_amd/image.py)."""
from __future__ import annotations

import ctypes as C

from . import _lib as L

_MODES = {"seed": L.FLOOD_MODE_SEED, "neighbor": L.FLOOD_MODE_NEIGHBOR}


class FloodFillOptions:
    """FloodFillOptions: threshold (f64, the largest pixel distance that joins), connectivity (4 or 8) and mode ("seed": candidates are
    compared with the seed pixel; "neighbor": with the pixel they were reached from). Values are checked by the library, not here."""

    def __init__(self, threshold: float = 0.0, connectivity: int = 4, mode="seed"):
        self.threshold, self.connectivity, self.mode = float(threshold), int(connectivity), mode

    def _c(self) -> L.ZgFloodFillOptions:
        mode = _MODES.get(self.mode, self.mode) if isinstance(self.mode, str) else self.mode
        if isinstance(mode, str):
            raise L.InvalidArgument(L.ERR_INVALID_ARGUMENT, f"flood_fill: mode {mode!r} (\"seed\" or \"neighbor\")")
        return L.ZgFloodFillOptions(self.threshold, self.connectivity, int(mode))

    def __repr__(self):
        return f"FloodFillOptions(threshold={self.threshold!r}, connectivity={self.connectivity}, mode={self.mode!r})"


FloodFillOptions.default = FloodFillOptions()


def flood_fill_tile() -> int:
    """The side of the tiles the fill labels in LDS (zg_flood_fill_tile)."""
    return int(L.lib().zg_flood_fill_tile())


def flood_fill_bound(pixel: int, threshold: float) -> float:
    """zg_flood_fill_bound_host: the constant the kernels compare with for a pixel type (zignal_amd._lib.PIXEL_*) and a threshold:
    the integer difference or sum of squares for byte pixels, the f64 difference or sum of squares for float pixels, -1 when nothing
    joins. Host arithmetic, no GPU needed."""
    out = C.c_double()
    L.check(L.lib().zg_flood_fill_bound_host(int(pixel), float(threshold), C.byref(out)))
    return out.value

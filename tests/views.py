"""Canvases for the destination-view tests: an image as a view into a larger allocation that holds a sentinel byte, so that anything an op
writes outside rows x cols of its destination shows. The reference's Image(T) is a view type (rows, cols, stride, data: image.zig:97-103)
and writing into a sub-rectangle of a larger frame is how its callers use it.

`Canvas` works on the device (the tests) and on CPU tensors (the helper's own test, tests/test_views.py). `place` builds the named layouts of
tests/test_gpu_dst_views.py: each flips one alignment term of the dispatch predicates relative to the all-aligned layout."""
import numpy as np
import torch

SENTINEL = 0xA5
LAYOUT = {"u8": (torch.uint8, 1), "rgb_u8": (torch.uint8, 3), "rgba_u8": (torch.uint8, 4),
          "f32": (torch.float32, 1), "rgb_f32": (torch.float32, 3), "rgba_f32": (torch.float32, 4)}
MIN_SIDE_PX, MIN_ROWS = 16, 2  # the guard around a view: what a kernel writes past the view's edge stays inside the allocation
_base_checked = set()


def psize(kind):
    dtype, ch = LAYOUT[kind]
    return ch * (1 if dtype == torch.uint8 else 4)


class Canvas:
    """rows x cols pixels of `kind` inside an allocation of (top + rows + bottom) rows of left_px + cols + right_px + extra_stride_px pixels,
    every byte of which starts as 0xA5. `shift_bytes` (a multiple of the element size, below 16) moves the whole frame inside the
    allocation: the only way to a 16-byte pixel whose origin is not 16-byte aligned."""

    def __init__(self, kind, rows, cols, left_px, top, right_px, bottom, extra_stride_px=0, shift_bytes=0, device="cuda"):
        assert left_px >= MIN_SIDE_PX and right_px >= MIN_SIDE_PX and top >= MIN_ROWS and bottom >= MIN_ROWS, (left_px, top, right_px, bottom)
        dtype, ch = LAYOUT[kind]
        esize = 1 if dtype == torch.uint8 else 4
        assert 0 <= shift_bytes < 16 and shift_bytes % esize == 0 and extra_stride_px >= 0
        self.kind, self.rows, self.cols, self.left, self.top = kind, rows, cols, left_px, top
        self.p = p = ch * esize
        self.stride = stride = left_px + cols + right_px + extra_stride_px
        self.shift = shift_bytes
        frame = (top + rows + bottom) * stride * p
        self.flat = torch.full(((shift_bytes + frame + 15) // 16 * 16,), SENTINEL, dtype=torch.uint8, device=device)
        if self.flat.is_cuda and "cuda" not in _base_checked:  # once: the origin arithmetic of the layouts rests on it
            assert self.flat.data_ptr() % 256 == 0, f"torch returned a device allocation at {self.flat.data_ptr():#x}: not 256-byte aligned"
            _base_checked.add("cuda")
        assert self.flat.data_ptr() % 16 == 0
        typed = self.flat[shift_bytes:shift_bytes + frame].view(dtype)
        shape, strides = ((rows, cols), (stride, 1)) if ch == 1 else ((rows, cols, ch), (stride * ch, ch, 1))
        self.origin = (top * stride + left_px) * p  # bytes from the frame's first byte
        self.view = torch.as_strided(typed, shape, strides, typed.storage_offset() + self.origin // esize)

    def _inside(self, t):
        """The view's bytes within `t`, a flat tensor of the allocation's length."""
        return torch.as_strided(t, (self.rows, self.cols * self.p), (self.stride * self.p, 1), self.shift + self.origin)

    def image(self, rect=None):
        """The zg.Image of the view, or of its sub-rectangle (l, t, r, b)."""
        import zignal_amd as zg
        img = zg.Image(self.view)
        return img if rect is None else img.view(rect)

    def put(self, host):
        self.view.copy_(torch.from_numpy(np.array(host, order="C")).to(self.view.device))  # a copy: the shared host arrays are read-only
        return self

    def facts(self):
        """The terms the dispatch predicates test, as the kernels see them."""
        return {"origin%16": self.view.data_ptr() % 16, "stride_bytes%16": self.stride * self.p % 16, "row_bytes%16": self.cols * self.p % 16,
                "rows%2": self.rows % 2, "cols%4": self.cols % 4}

    def stray(self):
        """None, or (byte offset in the allocation, row, col) of the first byte outside the view that no longer holds the sentinel; row and
        col are in pixels relative to the view's first pixel (negative above / left of it). Checked where the allocation lives."""
        if self.flat.is_cuda:
            torch.cuda.synchronize()
        bad = self.flat != SENTINEL
        self._inside(bad).fill_(False)
        if not bool(bad.any()):
            return None
        off = int(torch.nonzero(bad)[0])
        row, col_bytes = divmod(off - self.shift, self.stride * self.p)
        return off, row - self.top, col_bytes // self.p - self.left

    def take(self, what=""):
        """The view's pixels (a host array). Raises if any byte of the allocation outside the view was written."""
        hit = self.stray()
        if hit is not None:
            raise AssertionError(f"{what}: a byte outside the {self.rows} x {self.cols} {self.kind} view was written: byte {hit[0]} of the "
                                 f"allocation, (row, col) = ({hit[1]}, {hit[2]}) relative to the view (stride {self.stride} px, {self.facts()})")
        return self.view.cpu().numpy()


class Framed:
    """A contiguous tensor of `shape` inside a sentinel-filled allocation, `guard` bytes (at least 512, a multiple of 4) from its start and
    from its end: for the entry points that take contiguous buffers only (Pipeline.run's batches, zg_batch_blur_resize, isef_smooth). The
    guard's low bits move the buffer's origin off its 16-byte alignment."""

    def __init__(self, shape, guard=512, dtype=torch.uint8, device="cuda"):
        self.nbytes = int(np.prod(shape)) * (4 if dtype == torch.float32 else 1)
        self.guard = guard
        self.flat = torch.full((2 * guard + (self.nbytes + 15) // 16 * 16,), SENTINEL, dtype=torch.uint8, device=device)
        assert self.flat.data_ptr() % (256 if self.flat.is_cuda else 16) == 0 and guard % 4 == 0 and guard >= 512
        self.frames = self.flat[guard:guard + self.nbytes].view(dtype).view(shape)

    def stray(self):
        """None, or (byte offset in the allocation, byte offset relative to the buffer's first byte) of the first guard byte that was written."""
        if self.flat.is_cuda:
            torch.cuda.synchronize()
        bad = self.flat != SENTINEL
        bad[self.guard:self.guard + self.nbytes] = False
        if not bool(bad.any()):
            return None
        off = int(torch.nonzero(bad)[0])
        return off, off - self.guard

    def take(self, what=""):
        hit = self.stray()
        assert hit is None, f"{what}: byte {hit[1]} relative to the buffer (of {self.nbytes}) was written"
        return self.frames.cpu().numpy()


# ---- the named layouts ------------------------------------------------------------------------------------------------------------------
# A placement moves one term of the all-aligned layout and keeps the others: the origin (by bytes or by one pixel) or the stride.
PLACEMENTS = ("aligned", "origin+4B", "origin+8B", "origin+1px", "stride+4B", "stride+1px")


def placements(kind):
    """The placements that exist for this pixel size: one pixel is a dword already from 4 bytes up; a 16-byte pixel's stride is always a
    multiple of 16 bytes, and its origin too: the library refuses an Rgba(f32) image whose first pixel is not 16-byte aligned (check_image,
    zg_runtime.cpp: "kernels move whole pixels with one instruction"), which tests/test_gpu_dst_views.py pins."""
    p = psize(kind)
    out = ["aligned"] + (["origin+4B", "origin+8B"] if p != 16 else [])
    if p in (1, 3):
        out.append("origin+1px")
    if p != 16:
        out.append("stride+4B")
    if p in (1, 3):
        out.append("stride+1px")
    return out


def expected_facts(kind, placement):
    p = psize(kind)
    return {"aligned": (0, 0), "origin+4B": (4, 0), "origin+8B": (8, 0), "origin+1px": (p, 0), "stride+4B": (0, 4), "stride+1px": (0, p)}[placement]


def place(kind, rows, cols, placement="aligned", device="cuda"):
    """A rows x cols canvas in the named placement; asserts from facts() that origin and stride are on the side the name says."""
    p = psize(kind)
    left, right, top, extra, shift = 16, 32 + (-(16 + cols + 32)) % 16, 2, 0, 0  # aligned: the stride is a multiple of 16 pixels
    if placement in ("origin+4B", "origin+8B", "origin+1px"):
        want = p % 16 if placement == "origin+1px" else int(placement[7])
        moves = [d for d in range(16) if d * p % 16 == want]
        if moves:  # by whole pixels, the stride kept
            left, right = left + moves[0], right - moves[0]
        else:
            shift = want
    elif placement in ("stride+4B", "stride+1px"):
        want = p % 16 if placement == "stride+1px" else 4
        extra = [e for e in range(1, 16) if e * p % 16 == want][0]
        top = [t for t in range(2, 19) if t * extra * p % 16 == 0][0]  # the origin stays aligned
    else:
        assert placement == "aligned", placement
    c = Canvas(kind, rows, cols, left, top, right, 2, extra, shift, device)
    f = c.facts()
    assert (f["origin%16"], f["stride_bytes%16"]) == expected_facts(kind, placement), (kind, placement, f)
    return c

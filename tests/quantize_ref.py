"""Restatements of the reference's quantisation and dithering (src/image/quantize.zig, src/image/dither.zig, mapImageToPalette of
src/codecs/gif.zig:875-920) in numpy and plain Python, for tests/test_quantize_oracle.py and tests/test_gpu_quantize.py.

Error diffusion is restated twice, independently:
  dither_literal   the reference's loop: an in-place scatter in raster order, with its interior fast branch and its bounds-checked branch;
  dither_gather    the form the kernel uses: every pixel starts from its source byte and applies its neighbours' errors in the order
                   the scatter would have delivered them, clamping after each. Pixels with equal x + 2 r are independent of each other,
                   so the restatement walks those diagonals with numpy.
Images are (rows, cols, 3) uint8 arrays, palettes (n, 3) uint8 arrays, lookup tables (32768,) uint8 arrays."""
import numpy as np

CELLS = 32768
UNTOUCHED = 0xFFFFFFFF
NONE, FLOYD_STEINBERG, ATKINSON, ORDERED, AUTO = range(5)           # dither.Mode (dither.zig:18-30)
FIXED_6X7X6, FIXED_VGA16, FIXED_WEB216, ADAPTIVE = range(4)         # PaletteMode (quantize.zig:476-498)

# (dx, dy, weight, shift) in the reference's order (dither.zig:59-83)
FS_ENTRIES = ((1, 0, 7, 4), (-1, 1, 3, 4), (0, 1, 5, 4), (1, 1, 1, 4))
ATK_ENTRIES = ((1, 0, 1, 3), (2, 0, 1, 3), (-1, 1, 1, 3), (0, 1, 1, 3), (1, 1, 1, 3), (0, 2, 1, 3))
# what pixel (r, x) has received before it is quantised, in the order it arrives: (dr, dx, weight, shift) of the giving pixel
FS_GATHER = ((-1, -1, 1, 4), (-1, 0, 5, 4), (-1, 1, 3, 4), (0, -1, 7, 4))
ATK_GATHER = ((-2, 0, 1, 3), (-1, -1, 1, 3), (-1, 0, 1, 3), (-1, 1, 1, 3), (0, -2, 1, 3), (0, -1, 1, 3))

BAYER8 = np.array([[0, 32, 8, 40, 2, 34, 10, 42], [48, 16, 56, 24, 50, 18, 58, 26], [12, 44, 4, 36, 14, 46, 6, 38], [60, 28, 52, 20, 62, 30, 54, 22],
                   [3, 35, 11, 43, 1, 33, 9, 41], [51, 19, 59, 27, 49, 17, 57, 25], [15, 47, 7, 39, 13, 45, 5, 37], [63, 31, 55, 23, 61, 29, 53, 21]], np.int32)


# ---- convertColor(Rgb, pixel) and the cell key ------------------------------------------------------------------------------------
def to_rgb(img: np.ndarray) -> np.ndarray:
    """u8 replicates to (v, v, v); Rgba drops its alpha."""
    if img.ndim == 2:
        return np.repeat(img[:, :, None], 3, axis=2)
    return np.ascontiguousarray(img[:, :, :3])


def cell_keys(rgb: np.ndarray) -> np.ndarray:
    c = rgb.astype(np.uint32) >> 3
    return (c[..., 0] << 10) | (c[..., 1] << 5) | c[..., 2]


def expand5(v):
    return (v << 3) | (v >> 2)


# ---- histogram (quantize.zig:188-237) ---------------------------------------------------------------------------------------------
def histogram(img: np.ndarray):
    """(counts, first): the cell populations and the raster index of each cell's first pixel (UNTOUCHED for an empty cell)."""
    keys = cell_keys(to_rgb(img)).reshape(-1)
    counts = np.bincount(keys, minlength=CELLS).astype(np.uint32)
    first = np.full(CELLS, UNTOUCHED, np.uint32)
    uniq, index = np.unique(keys, return_index=True)
    first[uniq] = index.astype(np.uint32)
    return counts, first


# ---- median cut (quantize.zig:239-412) --------------------------------------------------------------------------------------------
def _sift_down(items, a, target, b, key):
    cur = target
    while True:
        child = 2 * (cur - a) + a + 1
        if not child < b:
            break
        nxt = child + 1
        if nxt < b and items[child][key] < items[nxt][key]:
            child = nxt
        if items[child][key] < items[cur][key]:
            break
        items[child], items[cur] = items[cur], items[child]
        cur = child


def heap_sort(items, a, b, key):
    """Zig's std.sort.heap over items[a:b] by items[i][key], restated: unstable."""
    if b - a < 2:
        return
    i = a + (b - a) // 2
    while i > a:
        i -= 1
        _sift_down(items, a, i, b, key)
    i = b
    while i > a:
        i -= 1
        items[a], items[i] = items[i], items[a]
        _sift_down(items, a, a, i, key)


class _Box:
    def __init__(self, items, begin, end):
        self.begin, self.end = begin, end
        self.mn, self.mx, self.population = [255, 255, 255], [0, 0, 0], 0
        for c in items[begin:end]:
            for k in range(3):
                self.mn[k], self.mx[k] = min(self.mn[k], c[k]), max(self.mx[k], c[k])
            self.population += c[3]

    def volume(self):
        if any(self.mx[k] < self.mn[k] for k in range(3)):
            return 0
        return (self.mx[0] - self.mn[0] + 1) * (self.mx[1] - self.mn[1] + 1) * (self.mx[2] - self.mn[2] + 1)

    def largest_dimension(self):
        r, g, b = (self.mx[k] - self.mn[k] if self.mx[k] >= self.mn[k] else 0 for k in range(3))
        if g >= r and g >= b:
            return 1
        return 0 if r >= b else 2


class NoPaletteColors(Exception):
    pass


def median_cut_from_histogram(counts, first, max_colors: int, capacity: int = 256) -> np.ndarray:
    keys = np.nonzero(counts)[0]
    keys = keys[np.argsort(first[keys], kind="stable")]  # the order the scan touched them
    items = [[expand5((k >> 10) & 31), expand5((k >> 5) & 31), expand5(k & 31), int(counts[k])] for k in (int(k) for k in keys)]
    palette_size = min(len(items), max_colors, capacity)
    if palette_size == 0:
        raise NoPaletteColors()
    if len(items) == 1:
        return np.array([items[0][:3]], np.uint8)
    boxes = [_Box(items, 0, len(items))]
    while len(boxes) < palette_size:
        largest, largest_score = None, 0
        for i, box in enumerate(boxes):
            if box.end - box.begin <= 1 or all(box.mx[k] <= box.mn[k] for k in range(3)):
                continue
            score = box.volume() * box.population
            if score > largest_score:
                largest, largest_score = i, score
        if largest is None:
            break
        box = boxes.pop(largest)
        heap_sort(items, box.begin, box.end, box.largest_dimension())
        n = box.end - box.begin
        half, acc, cut = sum(c[3] for c in items[box.begin:box.end]) // 2, 0, 0
        for i in range(n):
            acc += items[box.begin + i][3]
            if acc >= half:
                cut = max(1, min(i + 1, n - 1))
                break
        for part in (_Box(items, box.begin, box.begin + cut), _Box(items, box.begin + cut, box.end)):
            if part.end > part.begin and part.mx[0] >= part.mn[0]:
                boxes.append(part)
    out = []
    for box in boxes[:capacity]:
        part = items[box.begin:box.end]
        weight = sum(c[3] for c in part)
        if weight > 0:
            out.append([sum(c[k] * c[3] for c in part) // weight for k in range(3)])
        else:
            out.append([(box.mn[k] + box.mx[k]) // 2 for k in range(3)])
    return np.array(out, np.uint8)


def median_cut(img: np.ndarray, max_colors: int, capacity: int = 256) -> np.ndarray:
    return median_cut_from_histogram(*histogram(img), max_colors, capacity)


# ---- fixed palettes (quantize.zig:415-473) ----------------------------------------------------------------------------------------
VGA16 = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128], [192, 192, 192],
                  [128, 128, 128], [255, 0, 0], [0, 255, 0], [255, 255, 0], [0, 0, 255], [255, 0, 255], [0, 255, 255], [255, 255, 255]], np.uint8)


def fixed_palette(mode: int) -> np.ndarray:
    if mode == FIXED_6X7X6:
        return np.array([[(r * 255 + 2) // 5, (g * 255 + 3) // 6, (b * 255 + 2) // 5] for r in range(6) for g in range(7) for b in range(6)], np.uint8)
    if mode == FIXED_VGA16:
        return VGA16.copy()
    if mode == FIXED_WEB216:
        return np.array([[r * 51, g * 51, b * 51] for r in range(6) for g in range(6) for b in range(6)], np.uint8)
    raise ValueError(mode)


# ---- lookup table (quantize.zig:66-159) -------------------------------------------------------------------------------------------
def palette_lut(palette: np.ndarray) -> np.ndarray:
    cells = np.arange(CELLS, dtype=np.int64)
    target = np.stack([expand5((cells >> 10) & 31), expand5((cells >> 5) & 31), expand5(cells & 31)], axis=1)   # (CELLS, 3)
    diff = palette.astype(np.int64)[None, :, :] - target[:, None, :]
    score = ((diff * diff).sum(axis=2) << 8) | np.arange(len(palette), dtype=np.int64)[None, :]
    return (score.min(axis=1) & 0xFF).astype(np.uint8)


def lookup(lut: np.ndarray, rgb: np.ndarray) -> np.ndarray:
    return lut[cell_keys(rgb)]


# ---- ordered dither (dither.zig:113-196) ------------------------------------------------------------------------------------------
def dither_ordered(img: np.ndarray, palette: np.ndarray, lut: np.ndarray) -> np.ndarray:
    rows, cols = img.shape[:2]
    offsets = (BAYER8 - 32) >> 1
    off = offsets[np.arange(rows)[:, None] & 7, np.arange(cols)[None, :] & 7]
    v = np.clip(img.astype(np.int32) + off[:, :, None], 0, 255).astype(np.uint8)
    return palette[lookup(lut, v)]


# ---- error diffusion (dither.zig:208-331) -----------------------------------------------------------------------------------------
class DiffusionStats:
    """What the literal restatement met: updates clamped at 0, at 255, and negative products whose truncating division is not a floor."""

    def __init__(self):
        self.clamped_low = self.clamped_high = self.truncated = 0


def dither_literal(img: np.ndarray, palette: np.ndarray, lut: np.ndarray, mode: int, stats: DiffusionStats = None) -> np.ndarray:
    rows, cols = img.shape[:2]
    data = img.astype(np.int64).reshape(-1).tolist()
    pal, table = palette.tolist(), lut.tolist()
    stats = stats or DiffusionStats()
    entries = FS_ENTRIES if mode == FLOYD_STEINBERG else ATK_ENTRIES
    reach = 1 if mode == FLOYD_STEINBERG else 2

    def update(at, err, weight, shift):
        for ch in range(3):
            p = err[ch] * weight
            if p >= 0:
                d = p >> shift
            else:
                d = (p + (1 << shift) - 1) >> shift
                if p & ((1 << shift) - 1):
                    stats.truncated += 1
            v = data[at + ch] + d
            if v < 0:
                stats.clamped_low += 1
                v = 0
            elif v > 255:
                stats.clamped_high += 1
                v = 255
            data[at + ch] = v

    for r in range(rows):
        safe_row = r < rows - reach
        for c in range(cols):
            at = (r * cols + c) * 3
            cur = data[at:at + 3]
            q = pal[table[(cur[0] >> 3) << 10 | (cur[1] >> 3) << 5 | (cur[2] >> 3)]]
            data[at:at + 3] = q
            err = [cur[0] - q[0], cur[1] - q[1], cur[2] - q[2]]
            if safe_row and c > 0 and c < cols - reach:  # the interior branch, written out as the reference writes it
                if mode == FLOYD_STEINBERG:
                    update(at + 3, err, 7, 4)
                    update(at + (cols - 1) * 3, err, 3, 4)
                    update(at + cols * 3, err, 5, 4)
                    update(at + (cols + 1) * 3, err, 1, 4)
                else:
                    update(at + 3, err, 1, 3)
                    update(at + 6, err, 1, 3)
                    update(at + (cols - 1) * 3, err, 1, 3)
                    update(at + cols * 3, err, 1, 3)
                    update(at + (cols + 1) * 3, err, 1, 3)
                    update(at + 2 * cols * 3, err, 1, 3)
            else:
                for dx, dy, weight, shift in entries:
                    nc, nr = c + dx, r + dy
                    if 0 <= nr < rows and 0 <= nc < cols:
                        update((nr * cols + nc) * 3, err, weight, shift)
    return np.array(data, np.uint8).reshape(rows, cols, 3)


def dither_gather(img: np.ndarray, palette: np.ndarray, lut: np.ndarray, mode: int) -> np.ndarray:
    rows, cols = img.shape[:2]
    gather = FS_GATHER if mode == FLOYD_STEINBERG else ATK_GATHER
    err = np.zeros((rows + 2, cols + 4, 3), np.int32)  # the error of pixel (r, x) at [r + 2, x + 2]; pixels outside the image give 0
    out = np.empty((rows, cols, 3), np.uint8)
    src = img.astype(np.int32)
    pal = palette.astype(np.int32)
    for t in range(cols + 2 * (rows - 1)):
        r = np.arange(max(0, (t - cols + 2) // 2), min(rows - 1, t // 2) + 1)
        x = t - 2 * r
        keep = (x >= 0) & (x < cols)
        r, x = r[keep], x[keep]
        v = src[r, x]
        for dr, dx, weight, shift in gather:
            p = err[r + 2 + dr, x + 2 + dx] * weight
            v = np.clip(v + np.where(p >= 0, p >> shift, (p + (1 << shift) - 1) >> shift), 0, 255)
        q = pal[lut[(v[:, 0] >> 3) << 10 | (v[:, 1] >> 3) << 5 | (v[:, 2] >> 3)]]
        out[r, x] = q
        err[r + 2, x + 2] = v - q
    return out


def dither(img: np.ndarray, palette: np.ndarray, lut: np.ndarray, mode: int) -> np.ndarray:
    """dither.apply (dither.zig:34-41)."""
    if mode in (NONE, AUTO):
        return img.copy()
    if mode == ORDERED:
        return dither_ordered(img, palette, lut)
    return dither_gather(img, palette, lut, mode)


# ---- mapImageToPalette (gif.zig:875-920) ------------------------------------------------------------------------------------------
def map_to_palette(img: np.ndarray, palette: np.ndarray, use_dither: bool, transparent_index=None) -> np.ndarray:
    lookup_palette = palette[:-1] if transparent_index is not None else palette
    lut = palette_lut(lookup_palette)
    work = to_rgb(img)
    if use_dither:
        work = dither_gather(work, lookup_palette, lut, FLOYD_STEINBERG)
    indices = lookup(lut, work)
    if transparent_index is not None and img.ndim == 3 and img.shape[2] == 4:
        indices = np.where(img[:, :, 3] < 128, np.uint8(transparent_index), indices)
    return indices.astype(np.uint8)

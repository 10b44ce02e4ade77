"""CPU restatements of the reference's seam_carve example (examples/src/seam_carving.zig), test infrastructure only.

The *_literal functions follow computeEnergy (:22-45), computeSeam (:47-74) and removeSeam (:76-102) loop by loop, with the reference's
own index arithmetic; the *_fast ones are numpy forms of the same for the larger cases. The edge map of an iteration comes from the
oracle's sobel (oracle.pyoracle.sobel), which is read and not modified.

compute_seam_literal takes deliberately wrong rules too (`back`, `bottom`, `cols_rule`), so that the tests can show that a case tells
the reference's rule from its neighbours."""
import numpy as np

U32_MAX = 0xFFFFFFFF


def _at_or_null(img, r, c):
    """Image.atOrNull: None outside the image."""
    if r < 0 or c < 0 or r >= img.shape[0] or c >= img.shape[1]:
        return None
    return int(img[r, c])


def compute_energy_literal(edges):
    edges = np.asarray(edges)
    assert edges.dtype == np.uint8 and edges.ndim == 2
    rows, cols = edges.shape
    energy = np.zeros((rows, cols), np.uint32)
    for c in range(cols):
        energy[0, c] = edges[0, c]
    for r in range(1, rows):
        for c in range(cols):
            least = U32_MAX
            for i in (-1, 0, 1):
                x = c + i
                if x == cols:
                    x = cols - 1
                y = r - 1
                val = _at_or_null(energy, y, x)
                if val is not None:
                    least = min(val, least)
            energy[r, c] = int(edges[r, c]) + least
    return energy


def compute_seam_literal(energy, back="reference", bottom="first", cols_rule="duplicate"):
    """computeSeam. back: "reference" (the strict compare in the order left, centre, right, starting from the centre), "leftmost" /
    "rightmost" (the first / last of the three that holds their minimum). bottom: "first" (the reference) or "last" minimum of the
    bottom row. cols_rule: "duplicate" (the reference: column `cols` reads cols - 1), "skip" (it does not exist) or "packed" (no rule:
    the packed map is read at that index, which is the next row's first sum)."""
    energy = np.asarray(energy)
    rows, cols = energy.shape
    flat = energy.reshape(-1)
    seam = [0] * rows
    row = rows - 1
    seam[row] = 0
    for c in range(cols):
        if bottom == "first":
            if energy[row, c] < energy[row, seam[row]]:
                seam[row] = c
        elif energy[row, c] <= energy[row, seam[row]]:
            seam[row] = c
    y = rows - 2
    while y >= 0:
        r = y
        seam[r] = seam[r + 1]
        candidates = []
        for i in (-1, 0, 1):
            x = seam[r + 1] + i
            if x == cols:
                if cols_rule == "duplicate":
                    x = cols - 1
                elif cols_rule == "skip":
                    continue
            if cols_rule == "packed" and x == cols:
                curr = int(flat[y * cols + x]) if y * cols + x < flat.size else None
            else:
                curr = _at_or_null(energy, y, x)
            if curr is None:
                continue
            candidates.append((x, curr))
            if back == "reference":
                prev = int(flat[y * cols + seam[r]]) if seam[r] == cols else _at_or_null(energy, y, seam[r])
                if prev is not None and curr < prev:
                    seam[r] = x
        if back != "reference":
            least = min(v for _, v in candidates)
            holders = [x for x, v in candidates if v == least]
            seam[r] = holders[0] if back == "leftmost" else holders[-1]
        y -= 1
    return np.asarray(seam, np.uint32)


def remove_seam(image, seam):
    """removeSeam: row r without column seam[r]; an entry >= cols drops the row's last pixel (the device entry point's rule)."""
    image = np.asarray(image)
    rows, cols = image.shape[:2]
    out = np.empty((rows, cols - 1) + image.shape[2:], image.dtype)
    for r in range(rows):
        s = min(int(seam[r]), cols - 1)
        out[r, :s] = image[r, :s]
        out[r, s:] = image[r, s + 1:]
    return out


def compute_energy_fast(edges):
    edges = np.asarray(edges)
    rows, cols = edges.shape
    energy = np.empty((rows, cols), np.uint32)
    if rows == 0 or cols == 0:
        return energy
    energy[0] = edges[0]
    for r in range(1, rows):
        above = energy[r - 1]
        least = above.copy()
        least[1:] = np.minimum(least[1:], above[:-1])   # column -1 does not exist
        least[:-1] = np.minimum(least[:-1], above[1:])  # column `cols` is column cols - 1 again: the centre
        energy[r] = least + edges[r]
    return energy


def compute_seam_fast(energy):
    energy = np.asarray(energy)
    rows, cols = energy.shape
    seam = np.empty(rows, np.uint32)
    s = int(np.argmin(energy[rows - 1]))  # the first minimum
    seam[rows - 1] = s
    for r in range(rows - 2, -1, -1):
        row = energy[r]
        best = s
        if s >= 1 and row[s - 1] < row[best]:
            best = s - 1
        if s + 1 < cols and row[s + 1] < row[best]:
            best = s + 1
        s = best
        seam[r] = s
    return seam


def carve(image, n, sobel, literal=False):
    """n iterations of seam_carve (:104-144) on a copy; returns (carved image, (n, rows) seams)."""
    image = np.array(image, copy=True)
    seams = np.empty((n, image.shape[0]), np.uint32)
    for k in range(n):
        edges = sobel(np.ascontiguousarray(image))
        if literal:
            seam = compute_seam_literal(compute_energy_literal(edges))
        else:
            seam = compute_seam_fast(compute_energy_fast(edges))
        seams[k] = seam
        image = remove_seam(image, seam)
    return image, seams


def transpose(image):
    """t[c][r] = s[r][c]"""
    image = np.asarray(image)
    return np.ascontiguousarray(image.transpose((1, 0) + tuple(range(2, image.ndim))))


def carve_horizontal(image, n, sobel):
    """The library's definition of horizontal seams: transpose, carve vertically, transpose back. Seams are (n, cols)."""
    out, seams = carve(transpose(image), n, sobel)
    return transpose(out), seams

"""The reference's image metrics (src/image/metrics.zig) restated in numpy f64, twice each: plain Python loops that follow the source line
by line, and whole-array forms that keep every pixel's operation order and add the final sums left to right (np.cumsum; np.sum adds
pairwise and is never used for a sum whose bits matter). The two are held to each other in tests/test_metrics_oracle.py. At the end: the
chunked, speculative form of the sequential f64 sum (zignal_amd/csrc/metrics.hip) as an executable model."""
import math
import struct

import numpy as np

WINDOW = 11
RADIUS = WINDOW // 2
LUMA = (0.2126, 0.7152, 0.0722)  # src/color.zig:64-66


def component_max(a) -> float:
    """componentMaxValue (metrics.zig:177-186)."""
    return 255.0 if a.dtype == np.uint8 else 1.0


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def sequential_sum(values) -> float:
    """for (values) |v| s += v, from +0.0."""
    s = 0.0
    for v in np.asarray(values, np.float64).ravel().tolist():
        s += v
    return s


def left_to_right(values) -> float:
    """The same sum through np.cumsum, which adds in index order."""
    values = np.ascontiguousarray(values, np.float64).ravel()
    return float(np.cumsum(values)[-1]) + 0.0 if values.size else 0.0


def _fields(a):
    """(rows, cols, channels) view of an image array."""
    return a.reshape(a.shape[0], a.shape[1], -1)


# ---- psnr and meanPixelError ----------------------------------------------------------------------------------------------------------
def difference_terms(a, b, squared: bool) -> np.ndarray:
    """Every term in the reference's order (rows, then columns, then fields): d * d (:25-26,31-32) or |d| (:130-131,136-140)."""
    d = _fields(a).astype(np.float64) - _fields(b).astype(np.float64)
    return (d * d if squared else np.abs(d)).ravel()


def mse(a, b) -> float:
    t = difference_terms(a, b, True)
    with np.errstate(invalid="ignore"):
        return float(np.float64(left_to_right(t)) / np.float64(t.size))  # :48


def psnr_from_mse(m: float, max_value: float) -> float:
    if m == 0.0:
        return math.inf  # :49
    return 20.0 * math.log10(max_value) - 10.0 * math.log10(m)  # :53; log10 is the one function not restated bit for bit


def psnr(a, b) -> float:
    return psnr_from_mse(mse(a, b), component_max(a))


def mean_pixel_error(a, b) -> float:
    t = difference_terms(a, b, False)
    if t.size == 0:
        return 0.0  # :159
    return (left_to_right(t) / float(t.size)) / component_max(a)  # :160-165


def mse_loops(a, b) -> float:
    fa, fb = _fields(a), _fields(b)
    total, count = 0.0, 0
    for r in range(fa.shape[0]):
        for c in range(fa.shape[1]):
            for f in range(fa.shape[2]):
                diff = float(fa[r, c, f]) - float(fb[r, c, f])
                total += diff * diff
                count += 1
    return total / count if count else math.nan


def mean_pixel_error_loops(a, b) -> float:
    fa, fb = _fields(a), _fields(b)
    total, count = 0.0, 0
    for r in range(fa.shape[0]):
        for c in range(fa.shape[1]):
            for f in range(fa.shape[2]):
                total += abs(float(fa[r, c, f]) - float(fb[r, c, f]))
                count += 1
    if count == 0:
        return 0.0
    return (total / count) / component_max(a)


# ---- ssim ------------------------------------------------------------------------------------------------------------------------------
def ssim_window() -> np.ndarray:
    """generateSsimWindow (:230-249) with the correctly rounded exponential (mpmath): (121,) f64."""
    import mpmath
    mpmath.mp.prec = 200
    w = np.empty(WINDOW * WINDOW, np.float64)
    total = 0.0
    for dy in range(WINDOW):
        for dx in range(WINDOW):
            y, x = float(dy) - float(RADIUS), float(dx) - float(RADIUS)
            g = float(mpmath.exp(mpmath.mpf(-(x * x + y * y) / (2.0 * 1.5 * 1.5))))
            w[dy * WINDOW + dx] = g
            total += g
    return w / total


def pixel_scalar(a) -> np.ndarray:
    """getPixelScalar (:188-203) of every pixel: (rows, cols) f64."""
    f = _fields(a)
    if f.shape[2] == 1:
        return f[:, :, 0].astype(np.float64)
    if a.dtype == np.uint8:  # rgbLuma(r, g, b) * max_val, src/color.zig:1021-1027; alpha is not looked at
        r, g, b = (f[:, :, i].astype(np.float64) / 255.0 for i in range(3))
        return (LUMA[0] * r + LUMA[1] * g + LUMA[2] * b) * 255.0
    total = np.zeros(f.shape[:2], np.float64)
    for i in range(f.shape[2]):
        total = total + f[:, :, i].astype(np.float64)
    return total / float(f.shape[2])


def _constants(a):
    l = component_max(a)
    return (0.01 * l) * (0.01 * l), (0.03 * l) * (0.03 * l)  # :64-68


def ssim_map(a, b, window=None) -> np.ndarray:
    """numerator / denominator (:104-106) of every window: (rows - 10, cols - 10) f64. The 121 taps are stepped through with whole-plane
    operations, so every pixel sees the loop's operations in the loop's order."""
    w = ssim_window() if window is None else np.asarray(window, np.float64).ravel()
    x, y = pixel_scalar(a), pixel_scalar(b)
    rows, cols = x.shape[0] - 2 * RADIUS, x.shape[1] - 2 * RADIUS
    assert rows >= 1 and cols >= 1, "error.ImageTooSmall"
    c1, c2 = _constants(a)
    mu_x, mu_y, mu_x_sq, mu_y_sq, mu_xy = (np.zeros((rows, cols), np.float64) for _ in range(5))
    for dy in range(WINDOW):
        for dx in range(WINDOW):
            weight = w[dy * WINDOW + dx]
            vx, vy = x[dy:dy + rows, dx:dx + cols], y[dy:dy + rows, dx:dx + cols]
            mu_x = mu_x + weight * vx
            mu_y = mu_y + weight * vy
            mu_x_sq = mu_x_sq + weight * vx * vx
            mu_y_sq = mu_y_sq + weight * vy * vy
            mu_xy = mu_xy + weight * vx * vy
    sigma_x_sq = np.maximum(0.0, mu_x_sq - mu_x * mu_x)
    sigma_y_sq = np.maximum(0.0, mu_y_sq - mu_y * mu_y)
    sigma_xy = mu_xy - mu_x * mu_y
    numerator = (2.0 * mu_x * mu_y + c1) * (2.0 * sigma_xy + c2)
    denominator = (mu_x * mu_x + mu_y * mu_y + c1) * (sigma_x_sq + sigma_y_sq + c2)
    with np.errstate(all="ignore"):
        return numerator / denominator


def ssim(a, b, window=None) -> float:
    m = ssim_map(a, b, window)
    return left_to_right(m) / float(m.size)  # weight_sum is a sum of 1.0s: exact


def ssim_loops(a, b, window=None) -> float:
    w = (ssim_window() if window is None else np.asarray(window, np.float64).ravel()).tolist()
    x, y = pixel_scalar(a).tolist(), pixel_scalar(b).tolist()
    rows, cols = len(x), len(x[0])
    c1, c2 = _constants(a)
    ssim_sum, weight_sum = 0.0, 0.0
    for row in range(RADIUS, rows - RADIUS):
        for col in range(RADIUS, cols - RADIUS):
            mu_x = mu_y = mu_x_sq = mu_y_sq = mu_xy = 0.0
            for dy in range(WINDOW):
                for dx in range(WINDOW):
                    weight = w[dy * WINDOW + dx]
                    val_x, val_y = x[row - RADIUS + dy][col - RADIUS + dx], y[row - RADIUS + dy][col - RADIUS + dx]
                    mu_x += weight * val_x
                    mu_y += weight * val_y
                    mu_x_sq += weight * val_x * val_x
                    mu_y_sq += weight * val_y * val_y
                    mu_xy += weight * val_x * val_y
            sigma_x_sq = max(0.0, mu_x_sq - mu_x * mu_x)
            sigma_y_sq = max(0.0, mu_y_sq - mu_y * mu_y)
            sigma_xy = mu_xy - mu_x * mu_y
            numerator = (2.0 * mu_x * mu_y + c1) * (2.0 * sigma_xy + c2)
            denominator = (mu_x * mu_x + mu_y * mu_y + c1) * (sigma_x_sq + sigma_y_sq + c2)
            ssim_sum += numerator / denominator
            weight_sum += 1.0
    return ssim_sum / weight_sum


# ---- the sequential sum, chunked -----------------------------------------------------------------------------------------------------------
E_MIN, E_MAX = 1, 2046  # the biased exponents a guess may have: every normal f64 (metrics.hip)
ONE52, ONE53, MANT = 1 << 52, 1 << 53, (1 << 52) - 1


def chunk_record(v: np.ndarray, e: int, chunk_log2: int = 12):
    """The transducer of one chunk for the guessed biased exponent e: for each parity of S = s / g on entry, (total, lowest prefix,
    highest prefix) of the q, the empty prefix included; None when a term is too large for the integers used."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        x = np.ldexp(v, 1075 - e)  # v / g, g = 2^(e - 1023 - 52): exact, or too small to matter
        if not np.all(np.abs(x) < 2.0 ** min(52, 62 - chunk_log2)):  # q exact, totals and prefixes below 2^62
            return None
    r = np.rint(x)
    k = np.floor(x).astype(np.int64)
    q = r.astype(np.int64)
    ties = np.flatnonzero(np.abs(x - r) == 0.5)
    out = []
    for p in (0, 1):
        qq = q.copy()
        total, start = 0, 0
        for t in ties:  # round-to-even at a tie looks at the parity of the sum so far
            total += int(qq[start:t].sum())
            parity = (p + total) & 1
            qq[t] = int(k[t]) + (parity ^ (int(k[t]) & 1))
            total += int(qq[t])
            start = t + 1
        prefix = np.cumsum(qq)
        out.append((int(prefix[-1]), min(0, int(prefix.min())), max(0, int(prefix.max()))))
    return out


def chunked_sum(values, chunk: int):
    """(sum, serial_terms): the sum of `values` from +0.0 in index order with the bits of sequential_sum(), by the chunked algorithm."""
    values = np.ascontiguousarray(values, np.float64).ravel()
    n = values.size
    starts = list(range(0, n, chunk))
    with np.errstate(all="ignore"):
        approx = [float(np.sum(values[c:c + chunk])) for c in starts]  # any parallel sum will do
        before = np.concatenate(([0.0], np.cumsum(approx)[:-1])) if starts else []
    s, serial = 0.0, 0
    for c, prefix in zip(starts, before):
        v = values[c:c + chunk]
        if not np.any(v.view(np.uint64) << np.uint64(1)):
            continue  # a chunk of zeros leaves s alone (s is never -0.0)
        e = bits(prefix) >> 52  # the sign bit included: a negative prefix is out of range
        u = bits(s)
        if E_MIN <= e <= E_MAX and (u >> 52) == e:
            rec = chunk_record(v, e, max(6, (chunk - 1).bit_length()))
            if rec is not None:
                S = (u & MANT) | ONE52
                total, lo, hi = rec[S & 1]
                if S + lo > ONE52 and S + hi < ONE53:
                    s = struct.unpack("<d", struct.pack("<Q", (u & ~MANT) | ((S + total) & MANT)))[0]
                    continue
        for t in v.tolist():
            s += t
        serial += v.size
    return s, serial


def sum_inputs(seed: int, n: int = 1 << 20):
    """The inputs the sequential sum is tested on: (name, f64 array, non-negative?)."""
    rng = np.random.default_rng(seed)
    f32a, f32b = rng.random(n, np.float32), rng.random(n, np.float32)
    d = f32a.astype(np.float64) - f32b.astype(np.float64)
    ka = (rng.integers(0, 256, n).astype(np.float32) / np.float32(255)).astype(np.float64)
    kb = (rng.integers(0, 256, n).astype(np.float32) / np.float32(255)).astype(np.float64)
    return [
        ("uniform", rng.random(n), True),
        ("ssim_like", 1.0 - rng.random(n) * 1e-3, True),
        ("squared_f32_differences", d * d, True),
        ("absolute_f32_differences", np.abs(d), True),
        ("squared_k255_differences", (ka - kb) * (ka - kb), True),
        ("mixed_signs", rng.standard_normal(n), False),
        ("all_negative", -rng.random(n), False),
        ("scaled_1e-12", rng.random(n) * 1e-12, True),
        ("n_1089", rng.random(1089), True),
    ]


# ---- the sequential sum outside ordinary terms: infinities, NaN, overflow, subnormals, ties, 2^53 --------------------------------------
DOMAIN_SUM_INPUTS = ("inf_in_the_middle", "nan_in_the_middle", "inf_then_minus_inf", "finite_overflow", "subnormal_sum", "subnormal_into_normal",
                     "every_term_a_tie", "reaches_2^53_in_a_chunk", "chunk_ends_at_2^53-1", "negative_zeros", "alternating_positive_sum")
DOMAIN_SUM_N = 5 * 4096 + 17


def domain_sum_input(name: str, n: int, chunk: int = 4096) -> np.ndarray:
    """n f64 terms of the named kind (read-only); every kind is defined for every n, 0 and 1 included."""
    rng = np.random.default_rng(DOMAIN_SUM_INPUTS.index(name) * 7919 + n)
    tiny = 2.0 ** -1074
    if name in ("inf_in_the_middle", "nan_in_the_middle"):
        v = rng.random(n)
        if n:
            v[n // 2] = math.inf if name == "inf_in_the_middle" else math.nan
    elif name == "inf_then_minus_inf":  # inf + -inf: NaN from the second one on
        v = rng.random(n)
        if n >= 2:
            v[n // 3], v[n // 3 + max(1, n // 3)] = math.inf, -math.inf
    elif name == "finite_overflow":  # every term finite, the sum infinite after a few of them
        v = (rng.random(n) + 0.5) * 1e308
    elif name == "subnormal_sum":  # at most 2^20 units of 2^-1074 each: the whole sum stays below 2^36 units, subnormal
        v = rng.integers(0, 1 << 20, n).astype(np.float64) * tiny
    elif name == "subnormal_into_normal":  # about 2^41 units each: the sum passes 2^52 units (the smallest normal) after some 2000 terms
        v = rng.integers(0, 1 << 42, n).astype(np.float64) * tiny
    elif name == "every_term_a_tie":  # the sum sits in [2^52, 2^53), where one unit is 1: every k + 0.5 is a tie, decided by the sum's parity
        v = rng.integers(0, 8, n).astype(np.float64) + 0.5
        if n:
            v[0] = 2.0 ** 52 + 2.0 ** 20 + 1.0
    elif name == "reaches_2^53_in_a_chunk":  # 2^53 at term 1000; from there on each + 1.0 is a tie that rounds back to even
        v = np.ones(n)
        if n:
            v[0] = 2.0 ** 53 - 1000.0
    elif name == "chunk_ends_at_2^53-1":  # the first chunk of `chunk` terms ends one below 2^53, the next term reaches it
        v = np.ones(n)
        if n:
            v[0] = 2.0 ** 53 - float(chunk)
    elif name == "negative_zeros":
        v = rng.random(n)
        v[rng.random(n) < 0.3] = -0.0
    elif name == "alternating_positive_sum":
        v = rng.random(n) + 1.0
        v[1::2] = -rng.random(v[1::2].size)
    else:
        raise KeyError(name)
    v.setflags(write=False)
    return v


def same_bits_nan_class(got: float, want: float) -> bool:
    """Bit equality of two f64, with every NaN one class."""
    return (got != got and want != want) or bits(got) == bits(want)

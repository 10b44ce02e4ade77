"""The device ops merged after FAST under the conditions of tests/test_gpu_concurrency.py: two streams of the library in flight at once, and
eight host threads inside libzignal_hip.so at once. The harness (Op, Case, handover, rotation, run_threads, the child processes) is that
module's, unchanged; this one adds ops and cases.

Per op: the owner of the scratch block it takes (a ScratchBlock on the call's stream) and the CPU reference its results are held to.

  orb_detect_and_compute_into        orb.hip detect_and_compute: [pyramid][per-level candidates][counts][histograms][selection][weights]
                                     -> tests/orb_ref.py detect_and_compute_fast
  match_into_ratio_cross_check       match.hip match: [forward partials][reverse partials][cand][keep] -> tests/match_ref.py match_fast
  knn_match_into_k2                  match.hip knn: none (one launch into the caller's rows; it shares the streams) -> match_ref.knn_fast
  radius_match_into                  match.hip radius: the row offsets between its three launches -> match_ref.radius_fast
  hough_compute_find_lines           hough.hip compute: [count][edge list] (size 128: the LDS-strip route); find_lines: [row counts][row
                                     offsets][candidates][sorted][kept ...] -> tests/hough_ref.py compute_fast, find_lines on oracle.canny's edges
  flood_fill_seed, _neighbor         flood.hip flood: [links][labels] of the union-find -> tests/flood_ref.py flood_fill_fast
  psnr_, mean_pixel_error_rgba_f32   metrics.hip sum_terms: [approximate sums][guesses][records] of the speculative chunked sum (33 chunks)
                                     -> tests/metrics_ref.py difference_terms, left_to_right, mse, mean_pixel_error
  ssim_rgba_f32                      metrics.hip ssim: the map, then sum_terms' block -> metrics_ref.ssim_map, ssim with the library's window
  psnr_rgba_u8                       metrics.hip difference_metric: the one 64-bit accumulator every workgroup adds to -> metrics_ref
  color_histogram                    quantize.hip histogram: none (the caller's tensors; it shares the streams) -> tests/quantize_ref.py histogram
  dither_floyd_steinberg             quantize.hip error_diffusion: the carry rows between two launches (more than 1024 rows) -> quantize_ref.dither
  map_to_palette_dither_transparent  quantize.hip zg_palette_map: [lut][work frame] -> quantize_ref.map_to_palette
  median_blur_20_in_place            order_stat.hip order_stat_impl: the copy of the source that k_order_stat_hist reads -> oracle.order_statistic_blur
  canvas_draw_mixed, _curves         canvas.hip canvas_draw: the commands' boxes -> tests/canvas_ref.py, tests/canvas_curves_ref.py on
                                     tests/canvas_cases.py's random list
  canny_hough_lines_draw             Canny's planes, hough.hip's two blocks and canvas.hip's, taken and freed in a row on one stream
                                     -> the references above, composed
Host-synchronous forms (section B only: synchronous by their headers' contract, so handover's window cannot be open for them): their
ScratchBlock has no stream and their work runs on the default stream while the other threads run their own.

Every expected value is computed serially before any concurrent work starts; every comparison is bit for bit, order of lists, count words
and result records included."""
import threading
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import zignal_amd as zg  # noqa: E402
from zignal_amd import canvas as ZC  # noqa: E402
from tests import test_gpu_concurrency as H  # noqa: E402
from tests.test_gpu_concurrency import Case, Op, _child, _cuda, _err, _op_case, _same, _st, _want, handover, rotation, run_threads  # noqa: E402

pytestmark = pytest.mark.gpu
MODULE = "tests.test_gpu_concurrency_features"
KP = zg.KEYPOINT_DTYPE.itemsize
CMD = zg.DRAW_CMD_DTYPE.itemsize
LINE = zg.HOUGH_LINE_DTYPE.itemsize
T = zg.canvas_tile()  # host constants of the library: no GPU needed to read them
BAND, PHASE, ROWS_PER_LAUNCH = zg.dither_geometry()
FLOOD_TILE = zg.flood_fill_tile()
HOUGH_SIZE, HOUGH_BOX, HOUGH_SHAPE, HOUGH_CAP, HOUGH_THRESHOLD = 128, (30, 10, 158, 138), (150, 203), 256, 45
LINE_COLOR = (255, 40, 0, 160)
PALETTE16 = np.random.default_rng(1016).integers(0, 256, (16, 3), dtype=np.uint8)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _zeros(n, dtype=torch.uint8):
    return torch.zeros(n, dtype=dtype, device="cuda")


def _bits64(*values):
    """f64 values and counts as one uint64 array: the doubles by their bits."""
    return np.array([np.float64(v).view(np.uint64) if isinstance(v, float) else np.uint64(v) for v in values], np.uint64)


class IoOp(Op):
    """An op whose compared arrays come from its inputs and its outputs both (a frame drawn on in place and the count word beside it):
    post(arrays of ins + arrays of outs) -> the arrays compared with want()."""

    def fetch(self, ins, outs):
        return self.post([t.cpu().numpy() for t in list(ins) + list(outs)])


_HANDLES = {}
_HANDLES_LOCK = threading.Lock()


def _hough():
    """One HoughTransform handle for every stream and thread of the process."""
    with _HANDLES_LOCK:
        if "h" not in _HANDLES:
            _HANDLES["h"] = zg.HoughTransform(HOUGH_SIZE)
        return _HANDLES["h"]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _scene(seed, shape=HOUGH_SHAPE):
    """A grey frame with a few bright and dark rectangles and one slanted band on light noise: long straight edges for Canny and Hough."""
    rng = np.random.default_rng(7000 + seed)
    rows, cols = shape
    img = rng.integers(90, 110, shape).astype(np.uint8)
    for _ in range(3):
        r0, c0 = int(rng.integers(5, rows - 40)), int(rng.integers(5, cols - 50))
        img[r0:r0 + int(rng.integers(20, 60)), c0:c0 + int(rng.integers(30, 80))] = int(rng.integers(180, 255) if rng.random() < 0.6 else rng.integers(10, 50))
    rr, cc = np.indices(shape)
    slope, offset = float(rng.uniform(-0.8, 0.8)), float(rng.uniform(0.3, 0.7)) * rows
    img[np.abs(rr - (offset + slope * (cc - cols / 2))) < 4] = 20
    return img


def _rgba_of(gray):
    frame = np.repeat(gray[..., None], 4, axis=2).copy()
    frame[..., 3] = 255
    return frame


def _flood_plane(seed, rows, cols):
    """Patches of 100 .. 103 and 105 three pixels wide with a tenth of the pixels redrawn. Threshold 1: mode "neighbor" joins 100-101-102-103
    in a chain, mode "seed" from a 101 joins 100, 101 and 102 only. The seed is the 101 nearest the centre whose "seed" component (the
    smaller of the two) reaches into a second tile each way."""
    from tests.flood_ref import filled_mask
    rng = np.random.default_rng(900 + seed)
    coarse = rng.integers(0, 5, ((rows + 2) // 3, (cols + 2) // 3))
    idx = np.kron(coarse, np.ones((3, 3), np.int64))[:rows, :cols]
    idx = np.where(rng.random((rows, cols)) < 0.1, rng.integers(0, 5, (rows, cols)), idx)
    plane = np.array([100, 101, 102, 103, 105], np.uint8)[idx]
    rr, cc = np.nonzero(plane == 101)
    for k in np.argsort((rr - rows // 2) ** 2 + (cc - cols // 2) ** 2, kind="stable")[:64]:
        fr, fc = np.nonzero(filled_mask(plane, int(rr[k]), int(cc[k]), 1.0, 8, "seed"))
        if fr.min() // FLOOD_TILE != fr.max() // FLOOD_TILE and fc.min() // FLOOD_TILE != fc.max() // FLOOD_TILE:
            return plane, np.array([rr[k], cc[k]], np.int32)
    raise AssertionError(f"flood plane {seed}: no component near the centre crosses a tile border each way")


def _background(seed, rows, cols):
    """An Rgba(u8) frame with structure in every channel and transparent, translucent and opaque pixels (tests/test_gpu_canvas.py's)."""
    img = np.random.default_rng(3000 + seed).integers(0, 256, (rows, cols, 4)).astype(np.uint8)
    img[..., 3] = np.where(img[..., 3] < 64, 0, np.where(img[..., 3] > 160, 255, img[..., 3]))
    return img


def _curve_commands(seed, rows, cols):
    """Mixed commands with Béziers, a spline outline and a filled spline polygon in between, soft and translucent ones included."""
    from tests import canvas_cases as K
    from tests import canvas_curves_ref as CR
    rng = np.random.default_rng(5000 + seed)
    w, h = float(cols), float(rows)
    p = lambda: (float(np.float32(rng.uniform(-4, w + 4))), float(np.float32(rng.uniform(-4, h + 4))))  # noqa: E731
    ring = [(float(np.float32(w / 2 + 0.4 * w * np.cos(a) * r)), float(np.float32(h / 2 + 0.4 * h * np.sin(a) * r)))
            for a, r in zip(np.linspace(0, 2 * np.pi, 7)[:-1], rng.uniform(0.5, 1.0, 6))]
    base = K.random_commands(24, rows, cols, 6000 + seed)
    return (base[:8] + [CR.fill_spline_polygon(ring, (30, 200, 90, 120), 0.5, CR.SOFT), CR.quad_bezier(p(), p(), p(), (250, 20, 20, 200), 2, CR.SOFT)]
            + base[8:16] + [CR.cubic_bezier(p(), p(), p(), p(), (20, 20, 250, 255), 1, CR.FAST), CR.spline_polygon(ring[::-1], (240, 240, 10, 150), 3, 0.7, CR.SOFT)]
            + base[16:] + [CR.cubic_bezier(p(), p(), p(), p(), (10, 220, 220, 90), 5, CR.SOFT)])


def _metric_pair(seed, shape, dtype):
    """Two images: b is a disturbed a, most components equal or close (tests/test_gpu_metrics.py's pairs)."""
    rng = np.random.default_rng(8000 + seed)
    if dtype == np.uint8:
        a = rng.integers(0, 256, shape).astype(np.uint8)
        b = np.clip(a.astype(np.int32) + rng.integers(-9, 10, shape) * (rng.random(shape) < 0.6), 0, 255).astype(np.uint8)
    else:
        a = rng.random(shape, np.float32)
        b = (a + (rng.random(shape, np.float32) - np.float32(0.5)) * np.float32(0.1) * (rng.random(shape) < 0.6)).astype(np.float32)
    return [a, b]


# ---- the ops ---------------------------------------------------------------------------------------------------------------------------
def _orb_op(o, shape, cap=500):
    from tests import fast_ref as F
    from tests import orb_ref as R

    def want(h):
        k, d, _ = R.detect_and_compute_fast(h[0], R.Params())
        assert 0 < len(k) <= cap and len(np.unique(k["octave"])) >= 3, "keypoints on several pyramid levels"
        return [np.array([len(k)], np.int32), _bytes(k), _bytes(d)]

    def post(got):
        n = min(int(got[2][0]), cap)
        return [got[2], got[0][:n * KP], got[1][:n * 32]]
    return Op("orb_detect_and_compute_into", lambda seed: [F.photo_like(o.synth_u8(800 + seed, shape))],
              lambda ins, outs: zg.Orb().detect_and_compute_into(zg.Image(ins[0]), outs[0], outs[1], outs[2], cap), want,
              lambda ins: [_zeros(cap * KP), _zeros(cap * 32), _zeros(1, torch.int32)], post=post)


def _rows_want(rows):
    """A list of per-query rows as (lengths, the rows back to back)."""
    return np.array([len(r) for r in rows], np.int32), (_bytes(np.concatenate(rows)) if rows else np.zeros(0, np.uint8))


def _match_ops(nq, nt, radius_cap=8192):
    from tests import match_ref as M
    make = lambda seed: [M.bits(d).reshape(-1) for d in M.clustered(seed, nq, nt)]  # noqa: E731
    sets = lambda h: (h[0].reshape(-1, 32), h[1].reshape(-1, 32))  # noqa: E731
    strict, plain = M.Params(cross_check=True, max_distance=64, ratio_threshold=0.8), M.Params()

    def want_match(h):
        m, c = M.match_fast(*sets(h), strict)
        assert len(m) > 0 and c["ratio"] > 0 and c["cross_rej"] > 0, "the ratio test and the cross-check both reject some"
        return [np.array([len(m)], np.int32), _bytes(m)]

    def want_knn(h):
        lengths, flat = _rows_want(M.knn_fast(*sets(h), plain, 2))
        assert {0, 1, 2} <= set(lengths.tolist())
        return [lengths, flat]

    def post_knn(got):
        rows = got[1]
        m = got[0].reshape(nq, 2 * 12)
        return [rows, np.concatenate([m[i, :int(rows[i]) * 12] for i in range(nq)])]

    def want_radius(h):
        lengths, flat = _rows_want(M.radius_fast(*sets(h), 40.0))
        assert 0 < lengths.sum() <= radius_cap
        return [np.array([lengths.sum()], np.int32), lengths, flat]

    def post_radius(got):
        return [got[2], got[1], got[0][:min(int(got[2][0]), radius_cap) * 12]]
    return [
        Op("match_into_ratio_cross_check", make,
           lambda ins, outs: zg.BruteForceMatcher(**strict.kwargs()).match_into(ins[0], ins[1], outs[0], outs[1], nq), want_match,
           lambda ins: [_zeros(nq * 12), _zeros(1, torch.int32)], post=lambda got: [got[1], got[0][:int(got[1][0]) * 12]]),
        Op("knn_match_into_k2", make, lambda ins, outs: zg.BruteForceMatcher(**plain.kwargs()).knn_match_into(ins[0], ins[1], 2, outs[0], outs[1]), want_knn,
           lambda ins: [_zeros(nq * 2 * 12), _zeros(nq, torch.int32)], post=post_knn),
        Op("radius_match_into", make,
           lambda ins, outs: zg.BruteForceMatcher().radius_match_into(ins[0], ins[1], 40.0, outs[0], outs[1], outs[2], radius_cap), want_radius,
           lambda ins: [_zeros(radius_cap * 12), _zeros(nq, torch.int32), _zeros(1, torch.int32)], post=post_radius),
    ]


def _hough_want(edges, threshold):
    """(accumulator as the device's int32 words, [candidates, lines], the lines' bytes, the lines) of HOUGH_BOX of an edge map."""
    from tests import hough_ref as R
    acc = R.compute_fast(edges, HOUGH_BOX, np.zeros((HOUGH_SIZE, HOUGH_SIZE), np.uint32), HOUGH_SIZE)
    n, lines = R.find_lines(acc, HOUGH_SIZE, threshold, 5.0, 5.0)
    assert 0 < len(lines) <= HOUGH_CAP, f"{len(lines)} lines"
    return acc.view(np.int32), np.array([n, len(lines)], np.int32), _bytes(lines), lines


def _hough_op(o):
    """accumulator.zero_() -> compute_into -> find_lines_into as one call; size 128 is on the LDS-strip route; the threshold is a device word."""
    def call(ins, outs):
        outs[0].zero_()
        _hough().compute_into(ins[0], outs[0], HOUGH_BOX)
        _hough().find_lines_into(outs[0], ins[1], 5.0, 5.0, outs[1], outs[2], HOUGH_CAP)

    def post(got):
        n = min(int(got[4].view(np.uint32)[1]), HOUGH_CAP)
        return [got[2], got[4], got[3][:n * LINE]]
    return IoOp("hough_compute_find_lines", lambda seed: [o.canny(_scene(seed), 1.0, 40, 120), np.array([HOUGH_THRESHOLD], np.int32)], call,
                lambda h: list(_hough_want(h[0], HOUGH_THRESHOLD)[:3]),
                lambda ins: [_zeros((HOUGH_SIZE, HOUGH_SIZE), torch.int32), _zeros(HOUGH_CAP * LINE), _zeros(2, torch.int32)], post=post)


def _flood_op(mode, shape):
    from tests import flood_ref as R

    def want(h):
        out, n = R.flood_fill_fast(h[0], int(h[1][0]), int(h[1][1]), 200, 1.0, 8, mode)
        rr, cc = np.nonzero(out != h[0])
        assert n == len(rr) and rr.min() // FLOOD_TILE != rr.max() // FLOOD_TILE and cc.min() // FLOOD_TILE != cc.max() // FLOOD_TILE, "crosses tile borders"
        return [out, np.array([n], np.int32)]
    return IoOp(f"flood_fill_{mode}", lambda seed: list(_flood_plane(seed, *shape)),
                lambda ins, outs: zg.Image(ins[0]).flood_fill(0, 0, 200, 1.0, 8, mode, seed=ins[1], count=outs[0]), want,
                lambda ins: [_zeros(1, torch.int32)], post=lambda got: [got[0], got[2]])


def _metric_ops(shape):
    from tests import metrics_ref as R

    def record(got):
        r = got[0].view(zg.METRIC_RESULT_DTYPE)[0]
        return [_bits64(float(r["sum"]), int(r["count"]), float(r["value"]))]

    def want_psnr(h):
        t = R.difference_terms(h[0], h[1], True)
        assert t.size > 4096
        return [_bits64(R.left_to_right(t), t.size, R.mse(h[0], h[1]))]

    def want_mpe(h):
        t = R.difference_terms(h[0], h[1], False)
        return [_bits64(R.left_to_right(t), t.size, R.mean_pixel_error(h[0], h[1]))]

    def want_ssim(h):
        m = R.ssim_map(h[0], h[1], zg.ssim_window())
        assert m.size > 4096
        return [_bits64(R.left_to_right(m), m.size, R.ssim(h[0], h[1], zg.ssim_window()))]
    result = lambda ins: [torch.full((4,), -1.0, dtype=torch.float64, device="cuda")]  # noqa: E731
    f32, u8 = (lambda seed: _metric_pair(seed, shape + (4,), np.float32)), (lambda seed: _metric_pair(seed, shape + (4,), np.uint8))
    return [
        Op("psnr_rgba_f32", f32, lambda ins, outs: zg.Image(ins[0]).psnr(zg.Image(ins[1]), result=outs[0]), want_psnr, result, post=record),
        Op("mean_pixel_error_rgba_f32", f32, lambda ins, outs: zg.Image(ins[0]).mean_pixel_error(zg.Image(ins[1]), result=outs[0]), want_mpe, result, post=record),
        Op("ssim_rgba_f32", f32, lambda ins, outs: zg.Image(ins[0]).ssim(zg.Image(ins[1]), result=outs[0]), want_ssim, result, post=record),
        Op("psnr_rgba_u8", u8, lambda ins, outs: zg.Image(ins[0]).psnr(zg.Image(ins[1]), result=outs[0]), want_psnr, result, post=record),
    ]


def _quantize_ops(hist_shape, dither_shape, map_shape):
    from tests import quantize_ref as R
    noise = lambda base, shape: (lambda seed: [np.random.default_rng(base + seed).integers(0, 256, shape, dtype=np.uint8)])  # noqa: E731
    lut = {}

    def table():  # the reference's table of the palette, computed once and handed to dither, as a caller that keeps its own would
        if "t" not in lut:
            lut["t"] = R.palette_lut(PALETTE16)
        return lut["t"]

    def want_hist(h):
        counts, first = R.histogram(h[0])
        return [np.ascontiguousarray(counts, np.uint32).view(np.int32), np.ascontiguousarray(first, np.uint32).view(np.int32)]

    def make_map(seed):
        a = noise(9300, map_shape + (4,))(seed)[0]
        a[..., 3] = np.where(a[..., 3] < 128, 127, 128)  # either side of the alpha test
        return [a]
    assert dither_shape[0] > ROWS_PER_LAUNCH, "error diffusion takes its carry rows only across a launch boundary"
    return [
        Op("color_histogram", noise(9100, hist_shape + (3,)), lambda ins, outs: zg.Image(ins[0]).color_histogram(outs[0], outs[1]), want_hist,
           lambda ins: [_zeros(R.CELLS, torch.int32), _zeros(R.CELLS, torch.int32)]),
        IoOp("dither_floyd_steinberg", noise(9200, dither_shape + (3,)),
             lambda ins, outs: zg.Image(ins[0]).dither(outs[0], outs[1], zg.DitherMode.floyd_steinberg),
             lambda h: [R.dither(h[0], PALETTE16, table(), R.FLOYD_STEINBERG)], lambda ins: [_cuda(PALETTE16.reshape(-1)), _cuda(table())],
             post=lambda got: [got[0]]),
        Op("map_to_palette_dither_transparent", make_map,
           lambda ins, outs: zg.Image(ins[0]).map_to_palette(outs[1], True, 15, out=zg.Image(outs[0])),
           lambda h: [R.map_to_palette(h[0], PALETTE16, True, 15)],
           lambda ins: [_zeros(tuple(ins[0].shape[:2])), _cuda(PALETTE16.reshape(-1))], post=lambda got: [got[0]]),
    ]


def _median_op(o, shape):
    return Op("median_blur_20_in_place", lambda seed: [o.synth_u8(9400 + seed, shape)],
              lambda ins, outs: zg.Image(ins[0]).median_blur(20, out=zg.Image(ins[0])), lambda h: [o.order_statistic_blur(h[0], 20, 0, 0.5, 2)], inplace=True)


def _canvas_op(name, commands_of, run, shape):
    """Canvas.draw of a device command list on an Rgba(u8) frame in place. The packed list and its vertices are inputs, another for every
    seed; the seed rides along as a fourth input, so that want() rebuilds the command dicts the packed list came from."""
    def make(seed):
        cmds, vertices = ZC.pack_commands(commands_of(seed, *shape))
        assert len(vertices) > 0
        return [_background(seed, *shape), cmds.view(np.uint8).reshape(-1).copy(), np.ascontiguousarray(vertices, np.float32), np.array([seed], np.int32)]
    return IoOp(name, make, lambda ins, outs: zg.Canvas(ins[0]).draw(ins[1], vertices=ins[2]),
                lambda h: [run(h[0], commands_of(int(h[3][0]), *shape))], lambda ins: [], post=lambda got: [got[0]])


def _canvas_ops(shape, n):
    from tests import canvas_cases as K
    from tests import canvas_curves_ref as CR
    from tests import canvas_ref as R
    return [_canvas_op("canvas_draw_mixed", lambda seed, rows, cols: K.random_commands(n, rows, cols, 4000 + seed), R.run, shape),
            _canvas_op("canvas_draw_curves", _curve_commands, CR.run, shape)]


def _chain_want(o, gray, frame, threshold):
    """canny -> compute -> find_lines -> one soft line of width 2 per Hough line -> draw onto the frame, from the references of each step."""
    from tests import canvas_cases as K
    from tests import canvas_ref as R
    edges = o.canny(gray, 1.0, 40, 120)
    acc, counts, line_bytes, lines = _hough_want(edges, threshold)
    commands = [K.line(float(l["p1"][0]), float(l["p1"][1]), float(l["p2"][0]), float(l["p2"][1]), LINE_COLOR, 2, R.SOFT) for l in lines]
    drawn = R.run(frame, commands)
    assert not np.array_equal(drawn, frame)
    return [drawn, edges, acc, counts, line_bytes, np.array([len(lines)], np.int32), _bytes(ZC.pack_commands(commands)[0])]


def _chain_op(o):
    """Canny -> zeroed accumulator -> compute_into -> find_lines_into -> cmds_from_hough_lines -> Canvas.draw onto the source frame, one
    stream, no host round trip: one scratch block after another taken and freed on it."""
    def call(ins, outs):
        edges, acc, lines, counts, cmds, count = outs
        zg.Image(ins[0]).canny(1.0, 40, 120, out=zg.Image(edges))
        acc.zero_()
        _hough().compute_into(edges, acc, HOUGH_BOX)
        _hough().find_lines_into(acc, ins[2], 5.0, 5.0, lines, counts, HOUGH_CAP)
        ZC.cmds_from_hough_lines(lines, counts, LINE_COLOR, 2, "soft", cmds_out=cmds, count_out=count)
        zg.Canvas(ins[1]).draw(cmds, count=count)

    def alloc(ins):
        return [_zeros(HOUGH_SHAPE), _zeros((HOUGH_SIZE, HOUGH_SIZE), torch.int32), _zeros(HOUGH_CAP * LINE), _zeros(2, torch.int32),
                _zeros(HOUGH_CAP * CMD), _zeros(1, torch.int32)]

    def post(got):
        gray, frame, thr, edges, acc, lines, counts, cmds, count = got
        n = min(int(counts.view(np.uint32)[1]), HOUGH_CAP)
        return [frame, edges, acc, counts, lines[:n * LINE], count, cmds[:n * CMD]]

    def make(seed):
        gray = _scene(seed)
        return [gray, _rgba_of(gray), np.array([HOUGH_THRESHOLD], np.int32)]
    return IoOp("canny_hough_lines_draw", make, call, lambda h: _chain_want(o, h[0], h[1], HOUGH_THRESHOLD), alloc, post=post)


def feature_ops(o, small=False):
    """The ops of section A. small: the sizes section B mixes in, each still past the seam that makes the op take its scratch."""
    ops = [_orb_op(o, (160, 200) if small else (360, 480))]
    ops += _match_ops(*((33, 129) if small else (129, 513)))
    ops += [_hough_op(o)]
    ops += [_flood_op(mode, (FLOOD_TILE + 6, 2 * FLOOD_TILE + 3) if small else (2 * FLOOD_TILE + 3, 4 * FLOOD_TILE + 1)) for mode in ("seed", "neighbor")]
    ops += _metric_ops((75, 85) if small else (129, 257))
    ops += _quantize_ops((40, 50) if small else (150, 131), (ROWS_PER_LAUNCH + 6, 16 if small else 48), (BAND + 3, 33) if small else (BAND + 9, 77))
    ops += [_median_op(o, (45, 70) if small else (70, 131))]
    ops += _canvas_ops((2 * T + 9, 3 * T + 2) if small else (4 * T + 9, 6 * T + 2), 40 if small else 120)
    ops += [_chain_op(o)]
    return {op.name: op for op in ops}


A_NAMES = ("orb_detect_and_compute_into", "match_into_ratio_cross_check", "knn_match_into_k2", "radius_match_into", "hough_compute_find_lines",
           "flood_fill_seed", "flood_fill_neighbor", "psnr_rgba_f32", "mean_pixel_error_rgba_f32", "ssim_rgba_f32", "psnr_rgba_u8", "color_histogram",
           "dither_floyd_steinberg", "map_to_palette_dither_transparent", "median_blur_20_in_place", "canvas_draw_mixed", "canvas_draw_curves",
           "canny_hough_lines_draw")
ROTATION_NAMES = ("flood_fill_neighbor", "canny_hough_lines_draw")


# ---- section A -------------------------------------------------------------------------------------------------------------------------
def section_a_all(o, check_window):
    """Every new scenario of section A in this process (the child whose cache holds nothing)."""
    ops = feature_ops(o)
    for name in A_NAMES:
        handover(ops[name], check_window=check_window)
    for name in ROTATION_NAMES:
        rotation(ops[name], check_window=check_window)


@pytest.mark.parametrize("name", A_NAMES)
def test_a_block_freed_on_one_stream_is_handed_to_another(oracle, name):
    handover(feature_ops(oracle)[name])


@pytest.mark.parametrize("name", ROTATION_NAMES)
def test_a_block_goes_round_three_streams_twice(oracle, name):
    rotation(feature_ops(oracle)[name])


def test_a_cache_that_holds_nothing_changes_no_result():
    """ZIGNAL_HIP_SCRATCH_CACHE_MB=0 in a child process: every block goes back to the driver while the call that used it is still queued,
    so nothing is handed over and the window conditions do not apply; every result must still equal its reference."""
    H._share_wants()
    print(_child("T.section_a_all(o, check_window=False)", {"ZIGNAL_HIP_SCRATCH_CACHE_MB": "0"}, module=MODULE))


# ---- section B -------------------------------------------------------------------------------------------------------------------------
def _own_stream():
    """The host-synchronous forms work on the default stream; the thread that calls them has another one current."""
    assert _st().value, "the calling thread's current stream is the default stream"


def _per_thread_case(op, base, threads):
    """One input and one expected result per thread: a block or a table that leaks between threads shows as one thread's result in another's."""
    hosts = [op.make(base + t) for t in range(threads)]
    wants = [op.want([x.copy() for x in h]) for h in hosts]
    assert all(any(not np.array_equal(a, b) for a, b in zip(wants[0], w)) for w in wants[1:])

    def run(tid):
        ins = [_cuda(x) for x in hosts[tid]]
        outs = op.alloc(ins)
        op.call(ins, outs)
        return op.fetch(ins, outs)
    return Case(f"{op.name}, an input per thread", run, wants, per_thread=True)


def _keypoint_draw_case(name, gray, keypoints, detect, cap=64):
    """A detector's device list -> cmds_from_keypoints -> draw, nothing synchronised in between; fewer slots than keypoints."""
    from tests import canvas_cases as K
    from tests import canvas_ref as R
    color = (0, 255, 64, 128)
    frame = _rgba_of(gray)
    n = min(len(keypoints), cap)
    assert n > 0
    want = [R.run(frame, [K.circle(float(k["x"]), float(k["y"]), 3.0, color, 1, R.FAST) for k in keypoints[:n]]), np.array([n], np.int32)]

    def run(tid):
        src, dev = _cuda(gray), _cuda(frame)
        kps, count, cmds, ccount = _zeros(cap * KP), _zeros(1, torch.int32), _zeros(cap * CMD), _zeros(1, torch.int32)
        detect(zg.Image(src), kps, count, cap)
        ZC.cmds_from_keypoints(kps, count, 3.0, color, 1, "fast", cmds_out=cmds, count_out=ccount)
        ZC.draw(dev, cmds, count=ccount)
        return [dev.cpu().numpy(), ccount.cpu().numpy()]
    return Case(name, run, want)


def _host_cases(o, threads):
    """The host-synchronous forms: synchronous by their headers' contract, so they are in section B only."""
    from tests import canvas_cases as K
    from tests import canvas_ref as CR
    from tests import fast_ref as F
    from tests import flood_ref as FR
    from tests import match_ref as M
    from tests import metrics_ref as MR
    from tests import orb_ref as R
    from tests import quantize_ref as Q
    cases = []
    gray = F.photo_like(o.synth_u8(870, (160, 200)))
    k, d, _ = R.detect_and_compute_fast(gray, R.Params())
    assert len(k) > 0

    def run_orb(tid):
        _own_stream()
        gk, gd = zg.Orb().detect_and_compute(gray)
        return [_bytes(gk), _bytes(gd)]
    cases.append(Case("Orb.detect_and_compute, host image", run_orb, [_bytes(k), _bytes(d)]))
    cases.append(_keypoint_draw_case("Orb list -> cmds_from_keypoints -> draw", gray, k,
                                     lambda img, kps, count, cap: zg.Orb().detect_and_compute_into(img, kps, None, count, cap)))
    noise = o.synth_u8(871, (96, 120))
    cases.append(_keypoint_draw_case("Fast list -> cmds_from_keypoints -> draw", noise, F.detect_fast(noise, 20, 9, True),
                                     lambda img, kps, count, cap: zg.Fast(20, True).detect_into(img, kps, count, cap)))
    q, t = M.clustered(7, 65, 257)
    strict = M.Params(cross_check=True)
    want = [_bytes(M.match_fast(q, t, strict)[0]), *_rows_want(M.knn_fast(q, t, M.Params(), 2)), *_rows_want(M.radius_fast(q, t, 40.0))]

    def run_match(tid):
        _own_stream()
        return [_bytes(zg.BruteForceMatcher(**strict.kwargs()).match(q, t)), *_rows_want(zg.BruteForceMatcher().knn_match(q, t, 2)),
                *_rows_want(zg.BruteForceMatcher().radius_match(q, t, 40.0))]
    cases.append(Case("BruteForceMatcher.match, knn_match, radius_match, host arrays", run_match, want))
    edges = o.canny(_scene(71), 1.0, 40, 120)
    acc, _, line_bytes, _ = _hough_want(edges, HOUGH_THRESHOLD)

    def run_hough(tid, shared):
        _own_stream()
        h = _hough() if shared else zg.HoughTransform(HOUGH_SIZE)
        got = h.compute(edges, HOUGH_BOX)
        lines = h.find_lines(got, HOUGH_THRESHOLD, 5.0, 5.0)
        if not shared:
            h.close()
        return [got.view(np.int32), _bytes(lines)]
    cases.append(Case("HoughTransform.compute + find_lines, host arrays, one handle for all threads", lambda tid: run_hough(tid, True), [acc, line_bytes]))
    cases.append(Case("HoughTransform.compute + find_lines, host arrays, a handle per thread", lambda tid: run_hough(tid, False), [acc, line_bytes]))
    rgba = np.random.default_rng(72).integers(0, 256, (64, 64, 4), dtype=np.uint8)
    boxed = o.box_blur(rgba, 1)

    def run_palette(tid):
        _own_stream()
        frame = zg.Image(_cuda(rgba)).box_blur(1)  # produced on this thread's stream ...
        torch.cuda.current_stream().synchronize()  # ... and complete before the default-stream forms read it, as their header requires
        return [frame.median_cut(16), zg.build_palette(zg.PaletteMode.adaptive, frame, 8)]
    cases.append(Case("median_cut and build_palette(adaptive) of a frame made on the thread's stream", run_palette, [Q.median_cut(boxed, 16), Q.median_cut(boxed, 8)]))
    rows, cols = 2 * T + 9, 3 * T + 2
    lists = [K.random_commands(30, rows, cols, 4100 + t) for t in range(threads)]
    frames = [_background(80 + t, rows, cols) for t in range(threads)]

    def run_draw_host(tid):
        _own_stream()
        frame = frames[tid].copy()
        ZC.draw_host(frame, *ZC.pack_commands(lists[tid]))
        return [frame]
    cases.append(Case("draw_host, a list and a frame per thread", run_draw_host, [[CR.run(f, l)] for f, l in zip(frames, lists)], per_thread=True))
    planes = [_flood_plane(60 + t, FLOOD_TILE + 6, 2 * FLOOD_TILE + 3) for t in range(threads)]
    wants = []
    for plane, at in planes:
        out, n = FR.flood_fill_fast(plane, int(at[0]), int(at[1]), 200, 1.0, 8, "neighbor")
        wants.append([out, np.array([n], np.int64)])

    def run_flood_host(tid):
        _own_stream()
        plane, at = planes[tid]
        frame = plane.copy()
        n = zg.Image(frame).flood_fill(int(at[0]), int(at[1]), 200, 1.0, 8, "neighbor")
        return [frame, np.array([n], np.int64)]
    cases.append(Case("flood_fill, a host image per thread", run_flood_host, wants, per_thread=True))
    a, b = _metric_pair(73, (37, 53, 4), np.float32)

    def run_ssim_host(tid):
        _own_stream()
        return [_bits64(zg.Image(a).ssim(zg.Image(b)))]
    cases.append(Case("ssim, host images", run_ssim_host, [_bits64(MR.ssim(a, b, zg.ssim_window()))]))
    return cases


_CASES = {}


def section_b_cases(o, threads=8):
    """Built once per process (the references are pure Python): the tests of sections B and C share the list and leave it unchanged."""
    if "b" not in _CASES:
        small = feature_ops(o, small=True)
        cases = [_op_case(small[name], 20 + i, "small") for i, name in enumerate(A_NAMES)]
        cases += [_per_thread_case(small[name], 100, threads) for name in ("flood_fill_seed", "canvas_draw_mixed", "canvas_draw_curves")]
        _CASES["b"] = cases + _host_cases(o, threads)
    return _CASES["b"]


def test_b_eight_threads_each_on_its_own_stream(oracle):
    cases = section_b_cases(oracle)
    assert len(cases) >= len(A_NAMES) + 12
    run_threads(oracle, cases)


def test_b_first_calls_contended_in_a_fresh_process():
    """In a fresh process the first call of every one of these ops (code objects, handles, first-use tables) is made by eight threads at once."""
    _child("T.run_threads(o, T.section_b_cases(o))", module=MODULE)


# ---- section C -------------------------------------------------------------------------------------------------------------------------
def test_c_chain_capture_and_replay_beside_eager_threads(oracle):
    """The chain of section A recorded with zg_graph_* on one thread and replayed three times on changed frames while three other threads
    run the eager cases of section B."""
    from tests.test_gpu_graph_replay import Capture, _sentinel
    o = oracle
    lib = zg.lib()
    op = feature_ops(o)["canny_hough_lines_draw"]
    hosts, wants = zip(*[_want(op, 30 + s) for s in range(3)])
    eager = section_b_cases(o)
    ins = [_cuda(x) for x in hosts[0]]
    outs = op.alloc(ins)
    torch.cuda.synchronize()
    stop, counters = threading.Event(), [0, 0, 0]
    pool, futures = H._eager_threads(o, eager, 3, stop, counters, release_on=1)
    cap = Capture()
    try:
        deadline = time.monotonic() + 120
        while min(counters) < 1 and time.monotonic() < deadline and not any(f.done() for f in futures):
            time.sleep(0.01)  # the eager threads are under way before the capture begins
        with torch.cuda.stream(cap.stream):
            op.call(ins, outs)  # warm-up: the Hough handle, code objects
        cap.stream.synchronize()
        cap.record(lambda: op.call(ins, outs))
        at_capture = list(counters)
        rounds = 0
        while rounds < 3 or (min(c - a for c, a in zip(counters, at_capture)) < 3 and time.monotonic() < deadline and not any(f.done() for f in futures)):
            k = (1, 2, 0)[rounds % 3]
            with torch.cuda.stream(cap.stream):
                for t, h in zip(ins, hosts[k]):  # the frame is drawn on in place: it is loaded again for every replay
                    t.copy_(torch.from_numpy(h))
                for t in outs:
                    _sentinel(t)
            cap.launch()
            for n, (g, w) in enumerate(zip(op.fetch(ins, outs), wants[k])):
                _same(g, w, f"replay {rounds} on input {'ABC'[k]} beside eager threads, output {n}")
            rounds += 1
        overlap = [c - a for c, a in zip(counters, at_capture)]
    finally:
        stop.set()
        results = []
        for t, f in enumerate(futures):
            try:
                results.append(f.result(timeout=600))
            except Exception as e:  # noqa: BLE001
                results.append(f"thread {t}: {type(e).__name__}: {e}")
        pool.shutdown()
        cap.destroy()
    assert all(isinstance(r, int) for r in results), results
    assert min(overlap) >= 3, f"eager cases finished per thread while the graph replayed: {overlap}"
    torch.cuda.synchronize()
    assert lib.zg_release_graph_scratch() == 0, _err(lib)

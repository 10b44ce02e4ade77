"""zg_trace_paths and zg_canvas_cmds_from_paths on the device against tests/tracer_ref.py, byte for byte: counts, path_offsets and points
are compared as uint32 words. The frames and what they are there for: tests/tracer_cases.py; what stands behind the restatement:
tests/test_tracer_oracle.py. The reference records no expected output for Tracer, so the restatement is what the device is held to."""
import ctypes as C

import numpy as np
import pytest

import zignal_amd as zg
from tests import canvas_cases as CK
from tests import canvas_ref as CR
from tests import tracer_cases as K
from tests import tracer_ref as R
from tests.canvas_cases import same_bytes
from zignal_amd import _lib as L
from zignal_amd import canvas

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

GUARD, FILL = 16, 0x5A5A5A5A


class Out:
    """Device buffers for one trace with guard words behind both lists, everything pre-filled with FILL."""

    def __init__(self, point_capacity, path_capacity):
        self.pt_cap, self.pa_cap = point_capacity, path_capacity
        self.points = torch.full((2 * point_capacity + GUARD,), FILL, dtype=torch.int32, device="cuda")
        self.offsets = torch.full((path_capacity + 1 + GUARD,), FILL, dtype=torch.int32, device="cuda")
        self.counts = torch.full((4,), FILL, dtype=torch.int32, device="cuda")

    def run(self, tracer, edges):
        tracer.trace_into(edges, self.points if self.pt_cap else None, self.offsets, self.counts, self.pt_cap, self.pa_cap)
        return self

    def host(self):
        return tuple(t.cpu().numpy().view(np.uint32) for t in (self.counts, self.offsets, self.points))


def check(name, out, want_paths):
    """`out` against the whole list `want_paths` under the capacity rule: only whole paths, stopping at the first that does not fit."""
    counts, offsets, points = out.host()
    full_counts, full_offsets, full_points = R.pack(want_paths)
    written = 0
    while written < len(want_paths) and written < out.pa_cap and full_offsets[written + 1] <= out.pt_cap:
        written += 1
    n_pts = int(full_offsets[written])
    assert list(counts) == [full_counts[0], full_counts[1], written, n_pts], name
    assert np.array_equal(offsets[:written + 1], full_offsets[:written + 1]), name
    assert np.array_equal(points[:2 * n_pts], full_points[:n_pts].reshape(-1).view(np.uint32)), name
    assert (offsets[written + 1:] == np.uint32(FILL)).all() and (points[2 * n_pts:] == np.uint32(FILL)).all(), f"{name}: written past the lists"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def room(edges):
    n = int(np.count_nonzero(edges))  # a path has a pixel of its own, and a pixel is a point once
    return n, n


# ---- every frame, default options -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(K.FRAMES))
def test_frames_equal_the_restatement(name):
    edges = K.frame(name)
    want = K.want(name)
    tracer = zg.Tracer()
    check(name, Out(*room(edges)).run(tracer, dev(edges)), want)
    if edges.size <= 70 * 70:  # the host form and the two-call wrapper, on both kinds of memory
        for got in (tracer.trace(np.array(edges)), tracer.trace(dev(edges))):
            assert len(got) == len(want) and all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("serpentine_260", "serpentine_260_t"))
def test_one_raw_path_past_2_to_the_15_points(name):
    edges = K.frame(name)
    want = K.want(name, 5, 0.0)
    assert len(want) == 1 and len(want[0]) > 1 << 15
    check(name, Out(*room(edges)).run(zg.Tracer(5, 0.0), dev(edges)), want)


@pytest.mark.gpu
def test_canny_then_trace_without_leaving_the_device():
    src = zg.Image(dev(K.photo()))
    edges = zg.Image(torch.zeros((384, 512), dtype=torch.uint8, device="cuda"))
    src.canny(1.4, 10, 30, out=edges)
    out = Out(1 << 16, 1 << 14).run(zg.Tracer(), edges)  # enqueued behind canny, nothing in between
    host = edges.to_numpy()
    want = R.trace(host)
    assert len(want) > 50 and max(len(p) for p in R.trace_raw(host)) > 100
    check("photo", out, want)


# ---- options ------------------------------------------------------------------------------------------------------------------------
OPTION_FRAMES = ("noise_0.3_0", "noise_0.6_1", "spiral_130")
MIN_LENGTHS = (0, 1, 2, 5, 10, 10 ** 6)
EPSILONS = (0.0, -1.0, float("nan"), 0.25, 1.0, 1.5, 10.0, 1e9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", OPTION_FRAMES)
def test_min_path_length_and_epsilon(name):
    edges = K.frame(name)
    d = dev(edges)
    pairs = [(m, 1.0) for m in MIN_LENGTHS] + [(5, e) for e in EPSILONS] + [(0, 0.0), (2, 0.25), (10, 10.0), (1, float("nan"))]
    for m, e in pairs:
        check(f"{name} min {m} eps {e}", Out(*room(edges)).run(zg.Tracer(m, e), d), K.want(name, m, e))


@pytest.mark.gpu
def test_any_value_above_zero_is_an_edge():
    base = K.frame("noise_0.45_0")
    rng = np.random.default_rng(4)
    want = K.want("noise_0.45_0")
    for name, values in (("ones", np.ones(base.shape, np.uint8)), ("mixed", rng.integers(1, 256, base.shape).astype(np.uint8))):
        edges = np.where(base > 0, values, 0).astype(np.uint8)
        check(name, Out(*room(edges)).run(zg.Tracer(), dev(edges)), want)


# ---- views --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_window_of_a_frame_of_edges_and_a_padded_stride():
    inner = K.frame("junctions")
    rows, cols = inner.shape
    want = K.want("junctions")
    big = torch.full((rows + 9, cols + 14), 255, dtype=torch.uint8, device="cuda")  # what lies around the window would be followed
    big[4:4 + rows, 5:5 + cols] = dev(inner)
    check("window", Out(*room(inner)).run(zg.Tracer(), big[4:4 + rows, 5:5 + cols]), want)
    padded = torch.full((rows, cols + 3), 255, dtype=torch.uint8, device="cuda")
    padded[:, :cols] = dev(inner)
    check("stride", Out(*room(inner)).run(zg.Tracer(), padded[:, :cols]), want)
    host = np.full((rows + 2, cols + 3), 255, np.uint8)
    host[1:1 + rows, :cols] = inner
    got = zg.Tracer().trace(host[1:1 + rows, :cols])
    assert len(got) == len(want) and all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


# ---- capacity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capacities_stop_at_whole_paths_and_report_the_full_need():
    name = "noise_0.3_1"
    edges, want = K.frame(name), K.want(name)
    d = dev(edges)
    _, offsets, _ = R.pack(want)
    n_paths, n_points = len(want), int(offsets[-1])
    mid = n_paths // 2
    cases = [(int(offsets[mid]) - 1, n_paths), (int(offsets[mid]), n_paths), (0, n_paths), (n_points, mid - 1), (n_points, mid), (n_points, 0), (0, 0),
             (int(offsets[1]) - 1, n_paths), (n_points - 1, n_paths), (n_points, n_paths - 1), (n_points, n_paths)]
    for pt_cap, pa_cap in cases:
        check(f"capacities {pt_cap} {pa_cap}", Out(pt_cap, pa_cap).run(zg.Tracer(), d), want)
    first = Out(0, 0).run(zg.Tracer(), d).host()[0]
    assert list(first) == [n_paths, n_points, 0, 0]
    check("second call", Out(int(first[1]), int(first[0])).run(zg.Tracer(), d), want)  # counts[0..1] as capacities return everything
    counts = np.zeros(4, np.uint32)
    host_image = zg.Image(np.array(edges))  # kept alive: the descriptor points into it
    desc = host_image._desc()
    assert zg.lib().zg_trace_paths_host(C.byref(desc), None, None, 0, None, 0, counts.ctypes.data_as(L._U32P)) == 0  # counts alone, default options
    assert list(counts) == [n_paths, n_points, 0, 0]


# ---- the builder ----------------------------------------------------------------------------------------------------------------------
def segments(paths, color, width, mode):
    return [CK.line(float(a[0]), float(a[1]), float(b[0]), float(b[1]), color, width, mode) for p in paths for a, b in zip(p[:-1], p[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,min_len", [("junctions", 5), ("noise_0.3_2", 1)])  # min 1: paths of one point among the others
def test_builder_gives_the_segments_and_drawing_them_is_the_references_preview(name, min_len):
    edges = K.frame(name)
    want = K.want(name, min_len, 1.0)
    assert min_len != 1 or any(len(p) == 1 for p in want)
    out = Out(*room(edges)).run(zg.Tracer(min_len, 1.0), dev(edges))
    color = (255, 40, 10, 255)
    commands = segments(want, color, 1, CR.FAST)
    cmds, count = canvas.cmds_from_paths(out.points[:2 * out.pt_cap], out.offsets, out.counts, color, 1, "fast")
    frame_host = np.zeros(edges.shape + (3,), np.uint8)
    frame = dev(frame_host)
    canvas.draw(frame, cmds, count=count)
    torch.cuda.synchronize()
    assert int(count.item()) == len(commands) > 0
    assert cmds.cpu().numpy()[:len(commands) * 40].tobytes() == canvas.pack_commands(commands)[0].tobytes()
    assert same_bytes(frame.cpu().numpy(), CR.run(frame_host, commands))
    # a list shorter than the segments: the first `cap` of them, and nothing behind
    cap = len(commands) // 2
    small = torch.full(((cap + 2) * 40,), 0x77, dtype=torch.uint8, device="cuda")
    _, count2 = canvas.cmds_from_paths(out.points[:2 * out.pt_cap], out.offsets, out.counts, color, 1, "fast", cmds_out=small[:cap * 40])
    got = small.cpu().numpy()
    assert int(count2.item()) == cap and got[:cap * 40].tobytes() == canvas.pack_commands(commands[:cap])[0].tobytes() and (got[cap * 40:] == 0x77).all()


# ---- graph ----------------------------------------------------------------------------------------------------------------------------
class Chain:
    """Canny -> trace -> builder -> clear -> draw on the current stream, without a synchronisation."""
    SHAPE, POINTS, PATHS = (120, 160), 8192, 2048
    COLOR = (0, 255, 0, 255)

    def __init__(self):
        self.src = torch.zeros(self.SHAPE, dtype=torch.uint8, device="cuda")
        self.edges = zg.Image(torch.zeros(self.SHAPE, dtype=torch.uint8, device="cuda"))
        self.out = Out(self.POINTS, self.PATHS)
        self.cmds = torch.zeros(self.POINTS * 40, dtype=torch.uint8, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.frame = torch.zeros(self.SHAPE + (3,), dtype=torch.uint8, device="cuda")
        self.tracer = zg.Tracer(3, 1.0)

    def enqueue(self):
        zg.Image(self.src).canny(1.0, 40, 120, out=self.edges)
        self.out.run(self.tracer, self.edges)
        canvas.cmds_from_paths(self.out.points[:2 * self.POINTS], self.out.offsets, self.out.counts, self.COLOR, 1, "fast", cmds_out=self.cmds, count_out=self.count)
        self.frame.zero_()
        canvas.draw(self.frame, self.cmds, count=self.count)

    def check(self, name):
        want = R.trace(self.edges.to_numpy(), 3, 1.0)
        counts, offsets, points = self.out.host()
        _, full_offsets, full_points = R.pack(want)
        assert list(counts) == [len(want), len(full_points), len(want), len(full_points)], name
        assert np.array_equal(offsets[:len(want) + 1], full_offsets) and np.array_equal(points[:2 * len(full_points)], full_points.reshape(-1).view(np.uint32)), name
        commands = segments(want, self.COLOR, 1, CR.FAST)
        assert int(self.count.item()) == len(commands), name
        assert same_bytes(self.frame.cpu().numpy(), CR.run(np.zeros(self.SHAPE + (3,), np.uint8), commands)), name
        return len(want)


def chain_frame(kind):
    rng = np.random.default_rng(7)
    img = np.full(Chain.SHAPE, 100, np.uint8)
    if kind == "flat":
        return img  # no edges at all
    img[20:70, 30:110] = 200
    if kind == "busy":
        for _ in range(14):
            r, c = rng.integers(5, 100), rng.integers(5, 140)
            img[r:r + 9, c:c + 12] = rng.integers(0, 255)
    return img


@pytest.mark.gpu
def test_the_chain_from_canny_to_drawn_contours_replays_from_a_graph():
    chain = Chain()
    side = torch.cuda.Stream()
    chain.src.copy_(dev(chain_frame("box")))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        chain.enqueue()
    side.synchronize()
    assert chain.check("eager") >= 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain.enqueue()
    seen = []
    for kind in ("flat", "box", "busy"):
        chain.src.copy_(dev(chain_frame(kind)))
        for t in (chain.out.points, chain.out.offsets, chain.out.counts):
            t.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        seen.append(chain.check(f"replay on {kind}"))
    assert seen[0] == 0 and seen[2] > seen[1] >= 1  # none, then some, then more than the replay before
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0


# ---- status codes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_status_codes_are_decided_before_anything_is_enqueued():
    lib = zg.lib()
    edges = dev(K.frame("junctions"))
    out = Out(64, 64)
    args = (C.c_void_p(out.points.data_ptr()), 64, C.c_void_p(out.offsets.data_ptr()), 64, C.c_void_p(out.counts.data_ptr()), None)
    rgb = zg.Image(torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"))._desc()
    f32 = zg.Image(torch.zeros((8, 8), dtype=torch.float32, device="cuda"))._desc()
    assert lib.zg_trace_paths(C.byref(rgb), None, *args) == L.ERR_UNSUPPORTED
    assert lib.zg_trace_paths(C.byref(f32), None, *args) == L.ERR_UNSUPPORTED
    huge = zg.Image(edges)._desc()  # the descriptor alone: nothing of that size is allocated, and nothing is read
    huge.rows, huge.cols, huge.stride = 1 << 16, 1 << 15, 1 << 15
    assert lib.zg_trace_paths(C.byref(huge), None, *args) == L.ERR_UNSUPPORTED
    assert b"2^31" in lib.zg_last_error()
    d = zg.Image(edges)._desc()
    assert lib.zg_trace_paths(None, None, *args) == L.ERR_INVALID_ARGUMENT
    assert lib.zg_trace_paths(C.byref(d), None, None, 64, args[2], 64, args[4], None) == L.ERR_INVALID_ARGUMENT  # null points with a capacity
    assert lib.zg_trace_paths(C.byref(d), None, args[0], 64, None, 64, args[4], None) == L.ERR_INVALID_ARGUMENT  # null path_offsets
    assert lib.zg_trace_paths(C.byref(d), None, args[0], 64, args[2], 64, None, None) == L.ERR_INVALID_ARGUMENT  # null counts
    col = (C.c_uint8 * 4)(1, 2, 3, 255)
    cmds, count = torch.zeros(40 * 8, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    good = (args[0], args[2], args[4], 8, col, 1, 0, C.c_void_p(cmds.data_ptr()), C.c_void_p(count.data_ptr()), None)
    for i, bad in ((1, None), (2, None), (4, None), (5, 1 << 20), (6, 7), (7, None), (8, None)):
        a = list(good)
        a[i] = bad
        assert lib.zg_canvas_cmds_from_paths(*a) == L.ERR_INVALID_ARGUMENT, i
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.uint32) == np.uint32(FILL)).all() for t in (out.points, out.offsets, out.counts))  # nothing ran
    assert zg.tracer.scratch_bytes(1080, 1920) == lib.zg_trace_scratch_bytes(1080, 1920) > 30 * 1080 * 1920

"""zg_hough_* on the device against tests/hough_ref.py, byte for byte: compute in both of its forms, find_lines, their capacities,
the chain Canny -> clear -> compute -> max / 2 -> find_lines recorded into a graph and run on two streams, and a child process that
takes the direct voting form. The inputs and what they are there for: tests/hough_cases.py and tests/test_hough_oracle.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import zignal_amd as zg
from tests import hough_cases as K
from tests import hough_ref as R

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = zg.HOUGH_LINE_DTYPE
FILL = 0xAB


def limits():
    return int(zg.lib().zg_hough_lds_max_size()), int(zg.lib().zg_hough_pixel_chunk())


COMPUTE_NAMES = tuple(K.compute_cases(*limits()))  # host constants of the library: no GPU needed to read them
FIND_NAMES = tuple(K.find_cases(*limits()))


def device_acc(host):
    """A u32 accumulator on the device: an int32 tensor with the same bits."""
    return torch.from_numpy(np.array(host).view(np.int32)).cuda()


def acc_bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---- compute ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", COMPUTE_NAMES)
def test_compute_equals_the_reference(name):
    edges, box, size, start = K.compute_cases(*limits())[name]
    want = K.want_accumulator(name, *limits())
    h = zg.HoughTransform(size)
    acc = device_acc(np.zeros((size, size), np.uint32) if start is None else start)
    h.compute_into(torch.from_numpy(np.array(edges)).cuda(), acc, box)
    assert np.array_equal(acc_bits(acc), want), name
    if size <= 128:  # the host form: host pointers, the accumulator added to in place
        host = np.zeros((size, size), np.uint32) if start is None else start.copy()
        assert h.compute(np.array(edges), box, host) is host and np.array_equal(host, want), name


@pytest.mark.gpu
def test_compute_on_strided_views_of_both_images_and_two_calls_summing():
    lds_max, chunk = limits()
    edges, box, size, _ = K.compute_cases(lds_max, chunk)["lines97_box_inside"]
    want = K.want_accumulator("lines97_box_inside", lds_max, chunk)
    wide = torch.full((edges.shape[0], edges.shape[1] + 19), 255, dtype=torch.uint8, device="cuda")  # what lies beyond the view would vote
    wide[:, :edges.shape[1]] = torch.from_numpy(np.array(edges)).cuda()
    pad = torch.full((size, size + 5), 7, dtype=torch.int32, device="cuda")
    acc = pad[:, :size]
    acc.zero_()
    h = zg.HoughTransform(size)
    h.compute_into(wide[:, :edges.shape[1]], acc, box)
    assert np.array_equal(acc_bits(acc), want) and (pad[:, size:] == 7).all()
    h.compute_into(wide[:, :edges.shape[1]], acc, box)  # nothing is cleared: the second call adds
    assert np.array_equal(acc_bits(acc), 2 * want) and (pad[:, size:] == 7).all()
    host_pad = np.full((size, size + 3), 9, np.uint32)
    host_pad[:, :size] = 0
    wide_host = np.full((edges.shape[0], edges.shape[1] + 4), 255, np.uint8)
    wide_host[:, :edges.shape[1]] = edges
    h.compute(wide_host[:, :edges.shape[1]], box, host_pad[:, :size])
    assert np.array_equal(host_pad[:, :size], want) and (host_pad[:, size:] == 9).all()


@pytest.mark.gpu
def test_compute_default_box_and_returned_accumulator():
    edges = np.zeros((64, 64), np.uint8)
    edges[32, :] = 255
    acc = zg.HoughTransform(64).compute(torch.from_numpy(edges).cuda())
    assert int(acc.sum().item()) == 4096
    lines = zg.HoughTransform(64).find_lines(acc, 30, 10.0, 5.0)
    assert len(lines) == 1 and lines[0]["angle"] == np.float32(1.40625) and lines[0]["radius"] == np.float32(0.70710677) and lines[0]["score"] == 64


# ---- find_lines ------------------------------------------------------------------------------------------------------------------
def run_find(h, acc, thr, a, r, capacity, max_candidates=65536):
    lines = torch.full((max(capacity, 1) * 28,), FILL, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    h.find_lines_into(acc, thr, a, r, lines, counts, capacity, max_candidates)
    return acc_bits(counts), lines.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIND_NAMES)
def test_find_lines_equals_the_reference(name):
    size, acc, thr, a, r = K.find_cases(*limits())[name]
    n, want, _ = K.want_lines(name, *limits())
    h = zg.HoughTransform(size)
    dacc = device_acc(acc)
    counts, raw = run_find(h, dacc, thr, a, r, len(want) + 3)
    assert list(counts) == [n, len(want)], name
    assert raw[:len(want) * 28].tobytes() == want.tobytes(), name
    assert (raw[len(want) * 28:] == FILL).all(), name
    for got in (h.find_lines(dacc, thr, a, r), h.find_lines(np.array(acc), thr, a, r)):  # the synchronous forms: device and host pointers
        assert got.dtype == LINE and got.tobytes() == want.tobytes(), name
    if len(want) > 1:  # a capacity below the line count: the prefix and the full count
        k = len(want) // 2
        counts, raw = run_find(h, dacc, thr, a, r, k)
        assert list(counts) == [n, len(want)] and raw[:k * 28].tobytes() == want[:k].tobytes() and (raw[k * 28:] == FILL).all(), name
    thr_dev = torch.tensor([thr if thr < 1 << 31 else thr - (1 << 32)], dtype=torch.int32, device="cuda")
    counts, raw2 = run_find(h, dacc, thr_dev, a, r, len(want) + 3)  # the threshold read on the device
    counts1, raw1 = run_find(h, dacc, thr, a, r, len(want) + 3)
    assert list(counts) == list(counts1) == [n, len(want)] and raw2.tobytes() == raw1.tobytes(), name


@pytest.mark.gpu
def test_more_candidates_than_max_candidates_gives_no_lines_and_the_wrapper_asks_again():
    n, want, _ = K.want_lines("ties9_default", *limits())
    h = zg.HoughTransform(9)
    dacc = device_acc(np.zeros((9, 9), np.uint32))
    counts, raw = run_find(h, dacc, 0, 10.0, 5.0, 64, max_candidates=8)
    assert list(counts) == [49, 0] and (raw == FILL).all()
    counts, raw = run_find(h, dacc, 0, 10.0, 5.0, 64, max_candidates=0)
    assert list(counts) == [49, 0] and (raw == FILL).all()
    counts, raw = run_find(h, dacc, 0, 10.0, 5.0, 64, max_candidates=49)
    assert list(counts) == [49, 14] and raw[:14 * 28].tobytes() == want.tobytes()
    from zignal_amd import hough
    first = hough._FIRST_CANDIDATES
    hough._FIRST_CANDIDATES = 8  # the synchronous form starts below the candidate count and still returns the reference's list
    try:
        assert h.find_lines(dacc, 0, 10.0, 5.0).tobytes() == want.tobytes()
        assert h.find_lines(np.zeros((9, 9), np.uint32), 0, 10.0, 5.0).tobytes() == want.tobytes()
    finally:
        hough._FIRST_CANDIDATES = first
    lib = zg.lib()
    c = np.zeros(2, np.uint32)
    import ctypes as C
    acc = np.zeros((9, 9), np.uint32)
    assert lib.zg_hough_find_lines_host(h._h, acc.ctypes.data, 9, 0, 10.0, 5.0, 64, None, 0, c.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert list(c) == [49, 14]  # lines == NULL with capacity 0 asks for the counts


# ---- the chain -------------------------------------------------------------------------------------------------------------------
SIZE, BOX, SHAPE = 128, (30, 10, 158, 138), (150, 203)


def frame(seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(90, 110, SHAPE).astype(np.uint8)
    for _ in range(3):
        r0, r1 = sorted(rng.integers(5, SHAPE[0] - 5, 2))
        c0, c1 = sorted(rng.integers(5, SHAPE[1] - 5, 2))
        img[r0:r1 + 8, c0:c1 + 8] = rng.integers(180, 255)
    for _ in range(2):
        K.draw_line(img, (rng.integers(0, SHAPE[0]), 0), (rng.integers(0, SHAPE[0]), SHAPE[1] - 1), 20)
    return img


class Chain:
    """Canny -> zero-fill -> compute -> torch max // 2 clamped to 1 -> find_lines, on the current stream, without a synchronisation."""
    CAPACITY = 512

    def __init__(self):
        self.h = zg.HoughTransform(SIZE)
        self.src = torch.zeros(SHAPE, dtype=torch.uint8, device="cuda")
        self.edges = zg.Image(torch.zeros(SHAPE, dtype=torch.uint8, device="cuda"))
        self.acc = torch.zeros((SIZE, SIZE), dtype=torch.int32, device="cuda")
        self.thr = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.lines = torch.zeros(self.CAPACITY * 28, dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(2, dtype=torch.int32, device="cuda")

    def enqueue(self):
        zg.Image(self.src).canny(1.0, 40, 120, out=self.edges)
        self.acc.zero_()
        self.h.compute_into(self.edges, self.acc, BOX)
        self.thr.copy_(torch.clamp(torch.div(self.acc.max(), 2, rounding_mode="floor"), min=1).reshape(1))
        self.h.find_lines_into(self.acc, self.thr, 5.0, 5.0, self.lines, self.counts, self.CAPACITY)

    def check(self, name):
        edges = self.edges.to_numpy()
        assert np.count_nonzero(edges) > 100, name
        acc = R.compute_fast(edges, BOX, np.zeros((SIZE, SIZE), np.uint32), SIZE)
        assert np.array_equal(acc_bits(self.acc), acc), name
        thr = max(1, int(acc.max()) // 2)
        assert int(self.thr.item()) == thr, name
        n, want = R.find_lines(acc, SIZE, thr, 5.0, 5.0)
        assert 0 < len(want) <= self.CAPACITY and list(acc_bits(self.counts)) == [n, len(want)], name
        assert self.lines.cpu().numpy()[:len(want) * 28].tobytes() == want.tobytes(), name


@pytest.mark.gpu
def test_the_chain_from_canny_to_lines_replays_from_a_graph_on_changed_frames():
    chain = Chain()
    side = torch.cuda.Stream()
    chain.src.copy_(torch.from_numpy(frame(1)))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        chain.enqueue()  # warm-up outside the capture
    side.synchronize()
    chain.check("eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain.enqueue()
    for seed in (2, 3):
        chain.src.copy_(torch.from_numpy(frame(seed)))
        chain.lines.fill_(FILL)
        chain.counts.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        chain.check(f"replay on frame {seed}")
    del graph
    torch.cuda.synchronize()
    assert zg.lib().zg_release_graph_scratch() == 0


@pytest.mark.gpu
def test_the_chain_on_two_streams_at_once():
    chains = [Chain(), Chain()]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for c, seed in zip(chains, (4, 5)):
        c.src.copy_(torch.from_numpy(frame(seed)))
    torch.cuda.synchronize()
    for _ in range(4):  # both streams stay busy: each call is enqueued behind the other stream's, none is waited for
        for c, s in zip(chains, streams):
            with torch.cuda.stream(s):
                c.enqueue()
    torch.cuda.synchronize()
    for i, c in enumerate(chains):
        c.check(f"stream {i}")


# ---- the direct form -------------------------------------------------------------------------------------------------------------
CHILD_CASES = ("random5", "random64", "random97", "dense64", "lines97_box_past_right", "starts_non_zero", "box_past_corner")

CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import zignal_amd as zg
from tests import hough_cases as K
limits = (int(zg.lib().zg_hough_lds_max_size()), int(zg.lib().zg_hough_pixel_chunk()))
out = {}
for name in sys.argv[3:]:
    edges, box, size, start = K.compute_cases(*limits)[name]
    acc = torch.from_numpy((np.zeros((size, size), np.uint32) if start is None else np.array(start)).view(np.int32)).cuda()
    zg.HoughTransform(size).compute_into(torch.from_numpy(np.array(edges)).cuda(), acc, box)
    out[name] = acc.cpu().numpy().view(np.uint32)
np.savez(sys.argv[2], **out)
print("ok")
'''


@pytest.mark.gpu
def test_a_child_process_with_the_direct_form_gives_the_same_bytes():
    names = list(CHILD_CASES) + [n for n in K.compute_cases(*limits()) if n.startswith("edges")]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.npz")
        out = subprocess.run([sys.executable, "-c", CHILD, ROOT, path] + names, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, ZIGNAL_HIP_HOUGH_DIRECT="1"))
        assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-400:], out.stderr[-1500:])
        other = np.load(path)
        for name in names:
            assert np.array_equal(other[name], K.want_accumulator(name, *limits())), name

"""tests/tracer_ref.py, the numpy restatement of the reference's Tracer, held to what follows from the reference's code
(src/features/Tracer.zig): the reference records no expected output for Tracer, so these properties are what stands behind the
restatement the device is compared with."""
import numpy as np
import pytest

from tests import tracer_ref as R


def _noise(seed, density, shape=(60, 80)):
    return ((np.random.default_rng(seed).random(shape) < density) * 255).astype(np.uint8)


FRAMES = [("noise_%g" % d, _noise(int(d * 100), d)) for d in (0.1, 0.3, 0.45, 0.6)] + [("cpp", R.cpp_frame()), ("full", np.full((20, 23), 9, np.uint8))]


@pytest.fixture(scope="module", params=FRAMES, ids=[n for n, _ in FRAMES])
def traced(request):
    edges = request.param[1]
    return edges, R.trace_raw(edges)


def test_raw_points_are_edge_pixels_each_visited_once(traced):
    edges, raw = traced
    flat = np.concatenate([np.asarray(p) for p in raw])
    assert (edges.ravel()[flat] > 0).all()
    assert len(np.unique(flat)) == len(flat)  # dropped paths are among `raw`
    assert len(flat) == int((edges > 0).sum())  # and the scan leaves no edge pixel unvisited


def test_consecutive_raw_points_are_8_adjacent_and_starts_increase(traced):
    edges, raw = traced
    cols = edges.shape[1]
    for p in raw:
        idx = np.asarray(p)
        r, c = idx // cols, idx % cols
        assert (np.maximum(np.abs(np.diff(r)), np.abs(np.diff(c))) == 1).all() if len(p) > 1 else True
    starts = [p[0] for p in raw]
    assert all(a < b for a, b in zip(starts, starts[1:]))


def test_a_path_ends_only_where_no_open_neighbour_is_left(traced):
    edges, raw = traced
    rows, cols = edges.shape
    visited = np.zeros(edges.shape, bool)
    for p in raw:  # in scan order: what is visited when path i ends is the paths up to i
        idx = np.asarray(p)
        visited.ravel()[idx] = True
        r, c = divmod(p[-1], cols)
        for dr, dc in R.OFFSETS:
            rr, cc = r + dr, c + dc
            if 0 <= rr < rows and 0 <= cc < cols:
                assert not (edges[rr, cc] > 0 and not visited[rr, cc])


@pytest.mark.parametrize("eps", [0.25, 1.0, 1.5, 10.0])
def test_simplified_paths_keep_the_ends_a_subsequence_and_stay_within_epsilon(traced, eps):
    edges, raw = traced
    cols = edges.shape[1]
    for p in raw:
        pts = R.points_of(p, cols)
        if len(pts) < 3:
            assert np.array_equal(R.simplify_path(pts, eps), pts)
            continue
        keep = R.douglas_peucker_stack(pts, eps)
        assert keep[0] and keep[-1]
        out = R.simplify_path(pts, eps)
        assert np.array_equal(out, pts[keep])
        kept = np.nonzero(keep)[0]
        for a, b in zip(kept, kept[1:]):  # every dropped point lies within epsilon of the segment between the kept points around it
            if b > a + 1:
                d, _ = R.distance_to_segment(pts[a + 1:b], pts[a], pts[b])
                assert (d <= np.float32(eps)).all()


def test_whole_frame_equals_per_component_then_sorted(traced):
    edges, raw = traced
    assert R.trace_raw_by_components(edges) == raw


@pytest.mark.parametrize("eps", [0.25, 1.0, 3.0])
def test_rdp_from_a_stack_equals_rdp_level_by_level(traced, eps):
    edges, raw = traced
    for p in raw:
        if len(p) >= 3:
            pts = R.points_of(p, edges.shape[1])
            assert np.array_equal(R.douglas_peucker_stack(pts, eps), R.douglas_peucker_levels(pts, eps))


def test_the_step_frame_holds_every_decision_the_reference_can_meet():
    from tests import tracer_cases as K
    events = set()
    R.trace_raw(K.step_frame(), events)
    pairs = set(K.step_pairs())
    assert len(pairs) == 16 + 8 * 128 and pairs <= events
    # and nothing else can be met: the neighbour a step came from is visited, and a start has no unvisited edge before it in raster order
    for _, frame in FRAMES:
        seen = set()
        R.trace_raw(frame, seen)
        assert seen <= pairs
    assert K.step_frame().shape == (368, 368)


def test_trace_options():
    edges = _noise(5, 0.3)
    raw = R.trace_raw(edges)
    assert len(R.trace(edges, 0, 0.0)) == len(raw)
    assert [len(p) for p in R.trace(edges, 7, -1.0)] == [len(p) for p in raw if len(p) >= 7]  # the raw length decides, raw paths come back
    assert [len(p) for p in R.trace(edges, 7, float("nan"))] == [len(p) for p in raw if len(p) >= 7]
    assert all(len(p) == 2 for p in R.trace(edges, 3, 1e9))
    assert R.trace(np.zeros((4, 5), np.uint8)) == []
    one = R.trace(np.array([[0, 0], [0, 3]], np.uint8), 1, 1.0)
    assert len(one) == 1 and one[0].tolist() == [[1.0, 1.0]]  # (x = col, y = row)


def test_the_scores_are_the_f32_values_the_reference_computes():
    d = np.float32(1.0) / np.sqrt(np.float32(2.0))
    assert d == np.float32(0.70710677) and R.SCORE[0][0] == d * d + d * d == np.float32(0.99999994)
    assert R.SCORE[1][1] == np.float32(1.0) and R.SCORE[1][6] == np.float32(-1.0) and R.SCORE[1][3] == 0
    assert len({float(s) for row in R.SCORE for s in row}) == 7

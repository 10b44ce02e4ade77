"""The matcher on the MI355X (zg_match_descriptors / zg_match_knn / zg_match_radius and their _host forms) against the CPU restatement
of BruteForceMatcher (tests/match_ref.py): every comparison is of whole output arrays' bytes, order included."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from zignal_amd.match import train_chunk
from tests import match_ref as R
from tests.test_match_oracle import MAX_DISTANCES, RADII, SIZES, case, hand_made, ks, match_params, same_descriptor_at, train_sizes

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = zg.MATCH_DTYPE
FILL = 0xAB


def _dev(des) -> "torch.Tensor":
    return torch.from_numpy(R.bits(des).copy()).cuda()


def _word(v: int) -> "torch.Tensor":
    return torch.from_numpy(np.array([v], np.uint32).view(np.int32)).cuda()


def _u32(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def _matcher(p: R.Params) -> "zg.BruteForceMatcher":
    return zg.BruteForceMatcher(**p.kwargs())


def _rows_equal(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} rows, {len(want)} expected"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == M and g.tobytes() == w.tobytes(), f"{what}: row {i}: {g} vs {w}"


def _raw_match(m, q, t, cap, qc=None, tc=None):
    """match_into into cap + 1 entries pre-filled with 0xAB: (count, bytes)."""
    out = torch.full(((cap + 1) * 12,), FILL, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    m.match_into(q, t, out, count, cap, qc, tc)
    torch.cuda.synchronize()
    return int(_u32(count)[0]), out.cpu().numpy()


def _check_match(m, q, t, want, what, cap=None, qc=None, tc=None):
    cap = len(want) + 2 if cap is None else cap
    n, raw = _raw_match(m, q, t, cap, qc, tc)
    k = min(cap, len(want))
    assert n == len(want), f"{what}: count {n}, {len(want)} expected"
    assert raw[:k * 12].tobytes() == want[:k].tobytes(), f"{what}: {raw[:k * 12].view(M)} vs {want[:k]}"
    assert (raw[k * 12:] == FILL).all(), f"{what}: written past min(count, capacity)"


def _raw_knn(m, q, t, k, cq, qc=None, tc=None):
    """knn_match_into with the buffers pre-filled: (row_counts[cq] and one guard word, the cq x k entries and one guard entry)."""
    out = torch.full(((cq * k + 1) * 12,), FILL, dtype=torch.uint8, device="cuda")
    rows = torch.full((cq + 1,), -1, dtype=torch.int32, device="cuda")
    m.knn_match_into(q, t, k, out, rows, qc, tc)
    torch.cuda.synchronize()
    return _u32(rows), out.cpu().numpy()


def _check_knn(m, q, t, k, want, what, cq=None, qc=None, tc=None):
    """want: the restatement's rows (an empty list when a side is empty or k == 0: every row then has length 0)."""
    cq = len(want) if cq is None else cq
    rows, raw = _raw_knn(m, q, t, k, cq, qc, tc)
    assert rows[cq] == 0xFFFFFFFF, f"{what}: row_counts written past the query capacity"
    expect = np.full(cq * k * 12 + 12, FILL, np.uint8)
    for i in range(cq):
        w = want[i] if i < len(want) else np.zeros(0, M)
        assert rows[i] == len(w), f"{what}: row {i} has {rows[i]} entries, {len(w)} expected"
        expect[i * k * 12: i * k * 12 + len(w) * 12] = np.frombuffer(w.tobytes(), np.uint8)
    assert raw.tobytes() == expect.tobytes(), f"{what}: rows differ, or something was written outside them"


def _raw_radius(m, q, t, r, cap, cq, qc=None, tc=None):
    out = torch.full(((cap + 1) * 12,), FILL, dtype=torch.uint8, device="cuda")
    rows = torch.full((cq + 1,), -1, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    m.radius_match_into(q, t, r, out, rows, count, cap, qc, tc)
    torch.cuda.synchronize()
    return int(_u32(count)[0]), _u32(rows), out.cpu().numpy()


def _check_radius(m, q, t, r, want, what, cq=None, cap=None, qc=None, tc=None):
    cq = len(want) if cq is None else cq
    flat = np.concatenate(want) if want else np.zeros(0, M)
    cap = len(flat) + 2 if cap is None else cap
    n, rows, raw = _raw_radius(m, q, t, r, cap, cq, qc, tc)
    assert n == len(flat), f"{what}: count {n}, {len(flat)} expected"
    assert rows[cq] == 0xFFFFFFFF and list(rows[:cq]) == [len(w) for w in want] + [0] * (cq - len(want)), f"{what}: row_counts {rows}"
    k = min(cap, len(flat))
    assert raw[:k * 12].tobytes() == flat[:k].tobytes(), f"{what}: entries differ"
    assert (raw[k * 12:] == FILL).all(), f"{what}: written past min(count, capacity)"


# ---- shapes and parameters ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nq", SIZES)
def test_match_shapes_and_parameters(nq):
    for i, nt in enumerate(train_sizes(train_chunk())):
        q, t, _ = case(nq, nt)
        dq, dt = _dev(q), _dev(t)
        for p in match_params(i):
            want, _ = R.match_fast(q, t, p)
            _check_match(_matcher(p), dq, dt, want, f"{nq}x{nt} {p}")
        p = match_params(i)[i % 24]
        got = _matcher(p).match(q, t)  # the _host form
        assert got.dtype == M and got.tobytes() == R.match_fast(q, t, p)[0].tobytes(), f"host {nq}x{nt} {p}"


@pytest.mark.gpu
@pytest.mark.parametrize("nq", SIZES)
def test_knn_and_radius_shapes_and_parameters(nq):
    for i, nt in enumerate(train_sizes(train_chunk())):
        q, t, _ = case(nq, nt)
        dq, dt = _dev(q), _dev(t)
        for j, k in enumerate(ks(nt)):
            p = R.Params(max_distance=MAX_DISTANCES[(i + j) % 4])
            _check_knn(_matcher(p), dq, dt, k, R.knn_fast(q, t, p, k), f"knn {nq}x{nt} k={k} {p}")
        for r in RADII:
            _check_radius(zg.BruteForceMatcher(), dq, dt, r, R.radius_fast(q, t, r), f"radius {nq}x{nt} r={r}", cq=nq)
        k, r = ks(nt)[i % 5], RADII[i % 6]
        p = R.Params(max_distance=MAX_DISTANCES[i % 4])
        _rows_equal(_matcher(p).knn_match(q, t, k), R.knn_fast(q, t, p, k), f"host knn {nq}x{nt} k={k}")
        _rows_equal(_matcher(p).radius_match(q, t, r), R.radius_fast(q, t, r), f"host radius {nq}x{nt} r={r}")
        _rows_equal(_matcher(p).knn_match(dq, dt, k), R.knn_fast(q, t, p, k), f"device knn_match {nq}x{nt} k={k}")
        _rows_equal(_matcher(p).radius_match(dq, dt, r), R.radius_fast(q, t, r), f"device radius_match {nq}x{nt} r={r}")


@pytest.mark.gpu
def test_1000_by_1500():
    q, t, _ = case(1000, 1500)
    dq, dt = _dev(q), _dev(t)
    for p in (R.Params(), R.Params(cross_check=True), R.Params(True, 256, 2.0), R.Params(False, 0xFFFFFFFF, float("inf"))):
        want, _ = R.match_fast(q, t, p)
        assert len(want) > 0
        _check_match(_matcher(p), dq, dt, want, f"1000x1500 {p}")
        assert _matcher(p).match(dq, dt).tobytes() == want.tobytes()
    assert zg.BruteForceMatcher(cross_check=True).match(q, t).tobytes() == R.match_fast(q, t, R.Params(cross_check=True))[0].tobytes()
    for k in (2, 3):
        _check_knn(zg.BruteForceMatcher(), dq, dt, k, R.knn_fast(q, t, R.Params(), k), f"1000x1500 knn {k}")
    _check_knn(_matcher(R.Params(max_distance=256)), dq, dt, 3, R.knn_fast(q, t, R.Params(max_distance=256), 3), "1000x1500 knn 3, no cut")
    for r in (40.0, 64.5):
        _check_radius(zg.BruteForceMatcher(), dq, dt, r, R.radius_fast(q, t, r), f"1000x1500 radius {r}")
    _rows_equal(zg.BruteForceMatcher().radius_match(q, t, 40.0), R.radius_fast(q, t, 40.0), "1000x1500 host radius")


@pytest.mark.gpu
def test_more_chunks_than_workgroups_share():
    """Past 64 chunks a workgroup of the nearest kernel takes several, a stride apart: 65 chunks and one entry on either side (the
    train side, and the query side under the cross-check), with copies of one descriptor in two chunks of the same workgroup."""
    c = train_chunk()
    big = 65 * c + 1
    q, t, _ = case(65, big)
    for p in (R.Params(), R.Params(False, 256, 2.0)):
        _check_match(_matcher(p), _dev(q), _dev(t), R.match_fast(q, t, p)[0], f"65x{big} {p}")
    q, t, _ = case(big, 300)
    p = R.Params(cross_check=True)
    want, counters = R.match_fast(q, t, p)
    assert counters["cross_rej"] > 0 and counters["cross_acc"] > 0
    _check_match(_matcher(p), _dev(q), _dev(t), want, f"{big}x300 {p}")
    tb = R.bits(case(65, big)[1]).copy()
    first = 5
    tb[c + 100] = tb[first]
    tb[33 * c + first] = tb[first]  # 66 chunks over 33 workgroups: chunks 0 and 33 meet in one
    tb[64 * c + 7] = tb[first]
    one = R.as_descriptors(R.flip(tb[first], [3])[None])
    got = zg.BruteForceMatcher(ratio_threshold=2.0).match(_dev(one), _dev(tb))
    assert got.tobytes() == R.match_fast(one, tb, R.Params(False, 64, 2.0))[0].tobytes() and got[0]["train_idx"] == first and got[0]["distance"] == 1


# ---- hand-made cases -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hand_made_cases():
    c = train_chunk()
    for name, q, t, p in hand_made(c):
        want, _ = R.match_fast(q, t, p)
        _check_match(_matcher(p), _dev(q), _dev(t), want, name)
        assert _matcher(p).match(q, t).tobytes() == want.tobytes(), "host " + name
    q, t, where = same_descriptor_at(c)
    got = zg.BruteForceMatcher(ratio_threshold=2.0).match(_dev(same_descriptor_at(c, [5])[0]), _dev(t))
    assert len(got) == 1 and got[0]["train_idx"] == 0 and got[0]["distance"] == 1  # the lowest index across wave and chunk borders
    row = zg.BruteForceMatcher().knn_match(_dev(q), _dev(t), len(where))[0]
    assert list(row["train_idx"]) == where
    _check_knn(zg.BruteForceMatcher(), _dev(q), _dev(t), len(where) + 3, R.knn_fast(q, t, R.Params(), len(where) + 3), "copies, knn")
    _check_radius(zg.BruteForceMatcher(), _dev(q), _dev(t), 0.0, R.radius_fast(q, t, 0.0), "copies, radius 0")


# ---- device counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_counts_clamping_and_empty_sides():
    q, t, _ = case(65, 129)
    nq, nt, cq, ct = 40, 100, 65, 129
    bq, bt = R.bits(q).copy(), R.bits(t).copy()
    bq[nq:] = bq[:cq - nq]  # the tails hold copies of the queries: they would win if read
    bt[nt:] = bq[:ct - nt]
    dq, dt = _dev(bq), _dev(bt)
    wide = R.Params(False, 0xFFFFFFFF, 2.0)
    for p in (R.Params(), R.Params(cross_check=True), wide):
        m = _matcher(p)
        for (a, b) in ((nq, nt), (cq + 9, nt), (nq, ct + 1000), (0, nt), (nq, 0), (0, 0), (1, 1)):  # a count above its capacity is clamped
            sq, st = bq[:min(a, cq)], bt[:min(b, ct)]
            what = f"counts {a}, {b} {p}"
            _check_match(m, dq, dt, R.match_fast(sq, st, p)[0], what, qc=_word(a), tc=_word(b))
            _check_knn(m, dq, dt, 3, R.knn_fast(sq, st, p, 3), "knn " + what, cq=cq, qc=_word(a), tc=_word(b))
            _check_radius(m, dq, dt, 64.5, R.radius_fast(sq, st, 64.5), "radius " + what, cq=cq, qc=_word(a), tc=_word(b))
            _rows_equal(m.knn_match(dq, dt, 3, _word(a), _word(b)), R.knn_fast(sq, st, p, 3), "knn_match " + what)
    n, raw = _raw_match(_matcher(wide), dq, dt, 8, _word(5), _word(0))
    assert n == 0 and (raw == FILL).all()  # an empty train set accepts nothing, whatever max_distance is
    # sets given as 32-byte-offset slices
    for p in (R.Params(), R.Params(cross_check=True)):
        _check_match(_matcher(p), dq[3:], dt[5:], R.match_fast(bq[3:], bt[5:], p)[0], f"slices {p}")
        _check_match(_matcher(p), dq[3:], dt[5:], R.match_fast(bq[3:3 + 30], bt[5:5 + 70], p)[0], f"slices with counts {p}", qc=_word(30), tc=_word(70))
    _check_knn(zg.BruteForceMatcher(), dq[3:], dt[5:], 2, R.knn_fast(bq[3:], bt[5:], R.Params(), 2), "slices knn")
    _check_radius(zg.BruteForceMatcher(), dq[3:], dt[5:], 40.0, R.radius_fast(bq[3:], bt[5:], 40.0), "slices radius")
    # k = 0: every row is empty
    _check_knn(zg.BruteForceMatcher(), dq, dt, 0, [], "k = 0", cq=cq)


@pytest.mark.gpu
def test_output_capacity_below_count():
    q, t, _ = case(129, 257)
    dq, dt = _dev(q), _dev(t)
    p = R.Params(False, 256, 2.0)
    want, _ = R.match_fast(q, t, p)
    assert len(want) > 20
    for cap in (0, 1, len(want) // 2, len(want) - 1, len(want)):
        _check_match(_matcher(p), dq, dt, want, f"capacity {cap}", cap=cap)
    rows = R.radius_fast(q, t, 64.5)
    total = sum(len(r) for r in rows)
    assert total > 20
    for cap in (0, 1, total // 2, total - 1, total):
        _check_radius(zg.BruteForceMatcher(), dq, dt, 64.5, rows, f"radius capacity {cap}", cap=cap)
    lib = L.lib()
    n = C.c_uint32(0)
    qs = L.ZgDescriptorSet(q.ctypes.data, len(q), None)
    ts = L.ZgDescriptorSet(t.ctypes.data, len(t), None)
    pp = L.ZgMatcherParams(0, 256, 2.0)
    assert lib.zg_match_descriptors_host(C.byref(qs), C.byref(ts), C.byref(pp), None, 0, C.byref(n)) == 0 and n.value == len(want)
    half = np.full(len(want), 0xAB, np.uint8).repeat(12).view(M)
    assert lib.zg_match_descriptors_host(C.byref(qs), C.byref(ts), C.byref(pp), half.ctypes.data, len(want) // 2, C.byref(n)) == 0
    assert n.value == len(want) and half[:len(want) // 2].tobytes() == want[:len(want) // 2].tobytes()
    assert (half[len(want) // 2:].view(np.uint8) == FILL).all()


# ---- ORB chain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_orb_on_two_frames_then_match_without_a_synchronisation(oracle):
    a = oracle.synth_u8(21, (240, 320))
    b = np.roll(a, (3, 5), axis=(0, 1))
    cap = 500
    bufs = []
    orb, m = zg.Orb(), zg.BruteForceMatcher(cross_check=True)
    out = torch.full((cap * 12,), FILL, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    for img in (a, b):
        src = zg.Image(torch.from_numpy(np.ascontiguousarray(img)).cuda())
        kps = torch.zeros(cap * zg.KEYPOINT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        des = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
        n = torch.zeros(1, dtype=torch.int32, device="cuda")
        bufs.append((src, kps, des, n))
    torch.cuda.synchronize()
    for src, kps, des, n in bufs:
        orb.detect_and_compute_into(src, kps, des, n, cap)
    m.match_into(bufs[0][2], bufs[1][2], out, count, cap, bufs[0][3], bufs[1][3])
    torch.cuda.synchronize()
    des = [d.cpu().numpy().reshape(-1, 32)[:int(n.item())] for _, _, d, n in bufs]
    want, _ = R.match_fast(des[0], des[1], R.Params(cross_check=True))
    got = int(count.item())
    assert got == len(want) and got > 0
    assert out.cpu().numpy()[:got * 12].tobytes() == want.tobytes()


# ---- graph replay ---------------------------------------------------------------------------------------------------------
_CHILD = r"""
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import zignal_amd as zg
from zignal_amd import _lib as L
from tests import match_ref as R

lib = L.lib()
M = zg.MATCH_DTYPE
cq, ct, k, r = 300, 330, 3, 64.5
sets = [R.clustered(70 + i, cq, ct) for i in range(3)]
dq = torch.zeros(cq * 32, dtype=torch.uint8, device="cuda")
dt = torch.zeros(ct * 32, dtype=torch.uint8, device="cuda")
qc = torch.zeros(1, dtype=torch.int32, device="cuda")
tc = torch.zeros(1, dtype=torch.int32, device="cuda")
m = zg.BruteForceMatcher(cross_check=True, max_distance=64, ratio_threshold=0.8)
p = R.Params(True, 64, 0.8)
out = [torch.zeros(cq * 12, dtype=torch.uint8, device="cuda"), torch.zeros(cq * k * 12, dtype=torch.uint8, device="cuda"),
       torch.zeros(4000 * 12, dtype=torch.uint8, device="cuda")]
count = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3)]
rows = [None, torch.zeros(cq, dtype=torch.int32, device="cuda"), torch.zeros(cq, dtype=torch.int32, device="cuda")]


def record(i):
    if i == 0:
        m.match_into(dq, dt, out[0], count[0], cq, qc, tc)
    elif i == 1:
        m.knn_match_into(dq, dt, k, out[1], rows[1], qc, tc)
    else:
        m.radius_match_into(dq, dt, r, out[2], rows[2], count[2], 4000, qc, tc)


stream = torch.cuda.Stream()
torch.cuda.synchronize()
graphs = []
for i in range(3):  # i == 0: the process's first matcher call is this recorded one
    with torch.cuda.stream(stream):
        assert lib.zg_graph_begin_capture(C.c_void_p(stream.cuda_stream)) == 0
        try:
            record(i)
        finally:
            g = C.c_void_p()
            rc = lib.zg_graph_end_capture(C.c_void_p(stream.cuda_stream), C.byref(g))
        assert rc == 0, lib.zg_last_error()
    graphs.append(g)
# changed descriptors and changed count words: 300 -> 0 -> 1 -> capacity (and an empty train side)
for step, (si, nq, nt) in enumerate(((0, 300, 330), (1, 0, 330), (2, 1, 200), (1, cq, ct), (0, 17, 0), (2, 299, 1))):
    q, t = sets[si]
    with torch.cuda.stream(stream):
        dq.copy_(torch.from_numpy(R.bits(q).reshape(-1).copy()))
        dt.copy_(torch.from_numpy(R.bits(t).reshape(-1).copy()))
        qc.fill_(nq)
        tc.fill_(nt)
        for o in out:
            o.fill_(0xAB)
        for c in count + rows[1:]:
            c.fill_(-1)
    for g in graphs:
        assert lib.zg_graph_launch(g, C.c_void_p(stream.cuda_stream)) == 0
    stream.synchronize()
    sq, st = q[:nq], t[:nt]
    want = R.match_fast(sq, st, p)[0]
    n = int(count[0].item())
    assert n == len(want), ("replayed match count", step, n, len(want))
    assert out[0].cpu().numpy()[:n * 12].tobytes() == want.tobytes(), ("replayed match", step)
    assert (out[0].cpu().numpy()[n * 12:] == 0xAB).all(), ("replayed match wrote past its count", step)
    wk = R.knn_fast(sq, st, p, k)
    got_rows = rows[1].cpu().numpy()
    raw = out[1].cpu().numpy()
    for i in range(cq):
        w = wk[i] if i < len(wk) else np.zeros(0, M)
        assert got_rows[i] == len(w), ("replayed knn row length", step, i)
        assert raw[i * k * 12: i * k * 12 + len(w) * 12].tobytes() == w.tobytes(), ("replayed knn row", step, i)
    wr = R.radius_fast(sq, st, r)
    flat = np.concatenate(wr) if wr else np.zeros(0, M)
    assert len(flat) <= 4000
    assert int(count[2].item()) == len(flat), ("replayed radius count", step)
    assert list(rows[2].cpu().numpy()) == [len(w) for w in wr] + [0] * (cq - len(wr)), ("replayed radius rows", step)
    assert out[2].cpu().numpy()[:len(flat) * 12].tobytes() == flat.tobytes(), ("replayed radius", step)
    eager = m.match(dq, dt, qc, tc)
    assert eager.tobytes() == want.tobytes(), ("eager", step)
for g in graphs:
    assert lib.zg_graph_destroy(g) == 0
print("graph ok")
"""


@pytest.mark.gpu
def test_graph_capture_as_the_first_matcher_call_of_a_process(tmp_path):
    """A fresh child process (started, not exec'ed into) whose first matcher call is recorded into a graph; the three device entry
    points are each recorded once and replayed on changed descriptors and changed count words, and compared with the restatement."""
    script = tmp_path / "match_graph_child.py"
    script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "graph ok" in r.stdout, f"child exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


# ---- streams and threads -----------------------------------------------------------------------------------------------
def _stream_jobs():
    jobs = []
    for (nq, nt), p in zip(((129, 513), (65, 257)), (R.Params(cross_check=True), R.Params(False, 256, 2.0))):
        q, t, _ = case(nq, nt)
        want = (R.match_fast(q, t, p)[0], R.knn_fast(q, t, p, 3), R.radius_fast(q, t, 40.0))
        flat = np.concatenate(want[2]) if want[2] else np.zeros(0, M)
        bufs = {"q": _dev(q), "t": _dev(t), "m": torch.zeros(nq * 12, dtype=torch.uint8, device="cuda"), "mc": torch.zeros(1, dtype=torch.int32, device="cuda"),
                "k": torch.zeros(nq * 3 * 12, dtype=torch.uint8, device="cuda"), "kr": torch.zeros(nq, dtype=torch.int32, device="cuda"),
                "r": torch.zeros((len(flat) + 1) * 12, dtype=torch.uint8, device="cuda"), "rr": torch.zeros(nq, dtype=torch.int32, device="cuda"),
                "rc": torch.zeros(1, dtype=torch.int32, device="cuda")}
        jobs.append((p, bufs, want, flat))
    return jobs


def _enqueue(p, b):
    m = _matcher(p)
    m.match_into(b["q"], b["t"], b["m"], b["mc"])
    m.knn_match_into(b["q"], b["t"], 3, b["k"], b["kr"])
    m.radius_match_into(b["q"], b["t"], 40.0, b["r"], b["rr"], b["rc"])


def _check_job(p, b, want, flat, name):
    n = int(b["mc"].item())
    assert n == len(want[0]) and b["m"].cpu().numpy()[:n * 12].tobytes() == want[0].tobytes(), name
    rows, raw = _u32(b["kr"]), b["k"].cpu().numpy()
    for i, w in enumerate(want[1]):
        assert rows[i] == len(w) and raw[i * 36: i * 36 + len(w) * 12].tobytes() == w.tobytes(), f"{name}: knn row {i}"
    assert int(b["rc"].item()) == len(flat) and list(_u32(b["rr"])) == [len(w) for w in want[2]], name
    assert b["r"].cpu().numpy()[:len(flat) * 12].tobytes() == flat.tobytes(), name


@pytest.mark.gpu
def test_two_streams_on_different_sets():
    jobs = _stream_jobs()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(6):  # both streams stay busy: each call is enqueued behind the other stream's, none is waited for
        for s, (p, b, _, _) in zip(streams, jobs):
            with torch.cuda.stream(s):
                _enqueue(p, b)
    torch.cuda.synchronize()
    for i, (p, b, want, flat) in enumerate(jobs):
        _check_job(p, b, want, flat, f"stream {i}")


@pytest.mark.gpu
def test_two_host_threads_on_different_sets():
    jobs = _stream_jobs()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    errors = []
    torch.cuda.synchronize()

    def work(s, p, b):
        try:
            with torch.cuda.stream(s):
                for _ in range(6):
                    _enqueue(p, b)
            s.synchronize()
        except Exception as e:  # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(s, p, b)) for s, (p, b, _, _) in zip(streams, jobs)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    torch.cuda.synchronize()
    for i, (p, b, want, flat) in enumerate(jobs):
        _check_job(p, b, want, flat, f"thread {i}")

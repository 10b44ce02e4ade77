"""The matcher without a GPU: the two CPU restatements of BruteForceMatcher (tests/match_ref.py) against each other and against the
reference's own unit tests, the inputs of tests/test_gpu_match.py against the branches they are there for, zg_match_stats and the
argument checks of the zg_match_* entry points, and the module's boundary (header, bindings, Zig file)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import zignal_amd as zg
from zignal_amd import _lib as L
from tests import match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 63, 64, 65, 129)
SEED = 5
RATIOS = (0.8, 0.5, 1.0, 2.0, 0.0, float("inf"), float("nan"), -1.0)
MAX_DISTANCES = (0, 64, 256, 0xFFFFFFFF)
RADII = (-1.0, 0.0, 40.0, 64.5, 300.0, float("nan"))


def chunk() -> int:
    """The train chunk of the implementation (host arithmetic: no GPU needed)."""
    return int(zg.lib().zg_match_train_chunk())


def train_sizes(chunk: int):
    return SIZES + (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)


@functools.lru_cache(maxsize=None)
def case(nq: int, nt: int):
    """The input of shape nq x nt every matcher test uses, and its distance matrix. Shared: leave it unchanged."""
    q, t = R.clustered(SEED + 1000 * nq + nt, nq, nt)
    d = R.distance_matrix(q, t)
    for a in (q, t, d):
        a.setflags(write=False)
    return q, t, d


def match_params(i: int):
    """The parameter sets shape number i runs match with: every ratio with both cross_check values (max_distance taking its turn),
    and every max_distance at the default ratio."""
    out = [R.Params(bool(c), MAX_DISTANCES[(i + j) % 4], r) for j, r in enumerate(RATIOS) for c in (0, 1)]
    out += [R.Params(bool(c), m, 0.8) for m in MAX_DISTANCES for c in (0, 1)]
    return out


def ks(nt: int):
    return (1, 2, 3, nt, nt + 5)


def same_descriptor_at(chunk: int, flipped=()):
    """One descriptor at train indices {0, 63, 64, 65, chunk - 1, chunk, last} among random ones, and the query equal to it but for the
    `flipped` bits. The equal query ties at distance 0, which no ratio accepts (0 < r * 0); one flipped bit ties at distance 1,
    which ratio 2 accepts, and then the train index says which of the copies won."""
    rng = np.random.default_rng(17)
    nt = max(2 * chunk, 64) + 7
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    where = sorted({0, 63, 64, 65, chunk - 1, chunk, nt - 1})
    t[where] = t[0]
    return R.as_descriptors(R.flip(t[0], flipped)[None]), R.as_descriptors(t), where


def boundary_20_40():
    """best = 20, second = 40: with ratio 0.5 the test reads 20 < 20 and rejects."""
    q = np.zeros((1, 32), np.uint8)
    t = np.zeros((3, 32), np.uint8)
    t[0] = R.flip(q[0], range(40))
    t[1] = R.flip(q[0], range(100, 120))
    t[2] = R.flip(q[0], range(0, 256, 2))
    return R.as_descriptors(q), R.as_descriptors(t)


def shared_nearest():
    """Queries 1 and 3 are the same descriptor, one bit from train 2: the cross-check keeps query 1 alone."""
    rng = np.random.default_rng(23)
    t = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    q[1] = R.flip(t[2], [7])
    q[3] = q[1]
    return R.as_descriptors(q), R.as_descriptors(t)


def hand_made(chunk: int):
    """(name, query, train, Params) of the hand-made match cases."""
    q, t, _ = same_descriptor_at(chunk)
    q1 = same_descriptor_at(chunk, [5])[0]
    one = R.as_descriptors(np.full((1, 32), 0x5A, np.uint8))
    rng = np.random.default_rng(29)
    some = R.as_descriptors(rng.integers(0, 256, (70, 32), dtype=np.uint8))
    return [("copies across wave and chunk borders", q, t, R.Params(False, 64, 2.0)),
            ("copies, cross-check", q, t, R.Params(True, 64, 2.0)),
            ("copies one bit away", q1, t, R.Params(False, 64, 2.0)),
            ("copies one bit away, cross-check", q1, t, R.Params(True, 64, 2.0)),
            ("20 against 40 at ratio 0.5", *boundary_20_40(), R.Params(False, 64, 0.5)),
            ("20 against 40 at ratio 0.51", *boundary_20_40(), R.Params(False, 64, 0.51)),
            ("one train entry", some, one, R.Params(False, 256, 0.0)),
            ("one train entry, cross-check", some, one, R.Params(True, 256, 0.8)),
            ("all-equal train", some, R.as_descriptors(np.repeat(some["bits"][:1], 130, axis=0)), R.Params(False, 256, 2.0)),
            ("all-equal train, default ratio", some, R.as_descriptors(np.repeat(some["bits"][:1], 130, axis=0)), R.Params(False, 256, 0.8)),
            ("two queries, one nearest", *shared_nearest(), R.Params(True, 64, 0.8)),
            ("two queries, one nearest, no cross-check", *shared_nearest(), R.Params(False, 64, 0.8))]


def _same_rows(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), f"{what}: row {i}"


# ---- the restatements -----------------------------------------------------------------------------------------------------
def test_the_two_restatements_agree():
    for i, (nq, nt) in enumerate([(1, 1), (2, 1), (1, 2), (7, 5), (20, 33), (65, 129), (40, 70), (0, 5), (5, 0)]):
        q, t = R.clustered(100 + i, nq, nt)
        for p in match_params(i):
            a, ca = R.match_loops(q, t, p)
            b, cb = R.match_fast(q, t, p)
            assert a.tobytes() == b.tobytes() and ca == cb, (nq, nt, p)
        for k in (0, 1, 2, 3, nt, nt + 5):
            for m in MAX_DISTANCES:
                _same_rows(R.knn_loops(q, t, R.Params(max_distance=m), k), R.knn_fast(q, t, R.Params(max_distance=m), k), f"knn {nq}x{nt} k={k} max={m}")
        for r in RADII + (float("inf"), 128.0):
            _same_rows(R.radius_loops(q, t, r), R.radius_fast(q, t, r), f"radius {nq}x{nt} r={r}")
    for name, q, t, p in hand_made(16):
        a, ca = R.match_loops(q, t, p)
        b, cb = R.match_fast(q, t, p)
        assert a.tobytes() == b.tobytes() and ca == cb, name


def test_hand_made_cases_say_what_they_are_for():
    q, t, where = same_descriptor_at(chunk())
    m, c = R.match_fast(q, t, R.Params(False, 64, 2.0))
    assert len(m) == 0 and c["tie"] == 1 and c["ratio"] == 1  # 0 < 2 * 0 never passes
    m, c = R.match_fast(same_descriptor_at(chunk(), [5])[0], t, R.Params(False, 64, 2.0))
    assert len(m) == 1 and m[0]["train_idx"] == 0 and m[0]["distance"] == 1 and c["tie"] == 1
    assert len(R.match_fast(same_descriptor_at(chunk(), [5])[0], t, R.Params(False, 64, 1.0))[0]) == 0  # 1 < 1 * 1 does not pass
    row = R.knn_fast(q, t, R.Params(), len(where))[0]
    assert list(row["train_idx"]) == where and not row["distance"].any()
    m, c = R.match_fast(*boundary_20_40(), R.Params(False, 64, 0.5))
    assert len(m) == 0 and c["ratio"] == 1
    m, _ = R.match_fast(*boundary_20_40(), R.Params(False, 64, 0.51))
    assert len(m) == 1 and m[0]["train_idx"] == 1 and m[0]["distance"] == 20
    cases = {name: (q, t, p) for name, q, t, p in hand_made(chunk())}
    m, c = R.match_fast(*cases["one train entry"])
    assert c["lone"] == 70 and len(m) == 70  # a ratio of 0 rejects nothing when there is no second
    m, c = R.match_fast(*cases["one train entry, cross-check"])
    assert len(m) == 1 and c["cross_rej"] == 69
    m, c = R.match_fast(*cases["all-equal train"])
    assert c["tie"] == 70 and len(m) == 69 and not m["train_idx"].any()  # query 0 is the train descriptor: 0 < 2 * 0 fails
    assert len(R.match_fast(*cases["all-equal train, default ratio"])[0]) == 0
    m, c = R.match_fast(*cases["two queries, one nearest"])
    assert 1 in m["query_idx"] and 3 not in m["query_idx"] and c["cross_rej"] >= 1
    m, _ = R.match_fast(*cases["two queries, one nearest, no cross-check"])
    assert {1, 3} <= set(m["query_idx"])


def test_gpu_suite_inputs_cover_every_counter():
    """A condition on the inputs of tests/test_gpu_match.py, checked here on the CPU: SEED is chosen so that it holds."""
    total = dict.fromkeys(R.COUNTERS, 0)
    for nq in SIZES:
        for nt in train_sizes(chunk()):
            q, t, _ = case(nq, nt)
            for p in (R.Params(), R.Params(cross_check=True)):
                for k, v in R.match_fast(q, t, p)[1].items():
                    total[k] += v
    assert all(total[k] > 0 for k in R.COUNTERS), total
    q, t, _ = case(1000, 1500)
    c = R.match_fast(q, t, R.Params(cross_check=True))[1]
    assert all(c[k] > 0 for k in R.COUNTERS if k != "lone") and c["lone"] == 0, c
    n40 = sum(len(r) for r in R.radius_fast(q, t, 40.0))
    assert 0 < n40 < 1000 * 1500 // 100
    rows = R.knn_fast(q, t, R.Params(), 3)
    assert sum(len(r) < 3 for r in rows) > 500  # most rows are cut short by max_distance
    d = case(1000, 1500)[2]
    srt = np.sort(d, axis=1)
    assert int((srt[:, 2] == srt[:, 3]).sum()) > 0  # ties exactly at the k = 3 cut


def _desc():
    import types
    d = types.SimpleNamespace(bits=np.zeros(32, np.uint8))
    d.set = lambda *bits_: [d.bits.__setitem__(b // 8, d.bits[b // 8] | (1 << (b % 8))) for b in bits_]
    return d


def _set_of(*descs):
    return R.as_descriptors(np.stack([d.bits for d in descs]))


def test_the_reference_unit_tests_hold_on_the_restatement():
    # "BruteForceMatcher basic matching" (matcher.zig:273-313)
    a0, a1, b0, b1 = _desc(), _desc(), _desc(), _desc()
    a0.set(0, 10), a1.set(5, 15), b0.set(0, 11), b1.set(100, 200)
    for fn in (R.match_loops, R.match_fast):
        m, _ = fn(_set_of(a0, a1), _set_of(b0, b1), R.Params(False, 100))
        assert len(m) > 0 and m[0]["query_idx"] == 0 and m[0]["train_idx"] == 0
    # "BruteForceMatcher cross-check" (:315-358)
    a0, a1, b0, b1 = _desc(), _desc(), _desc(), _desc()
    a0.set(0), b0.set(0), a1.set(*range(100)), b1.set(*range(100, 200))
    for fn in (R.match_loops, R.match_fast):
        assert len(fn(_set_of(a0, a1), _set_of(b0, b1), R.Params(True, 256))[0]) <= len(fn(_set_of(a0, a1), _set_of(b0, b1), R.Params(False, 256))[0])
    # "BruteForceMatcher kNN matching" (:360-398)
    q, t0, t1, t2 = _desc(), _desc(), _desc(), _desc()
    q.set(0), t0.set(1), t1.set(1, 2), t2.set(1, 2, 3)
    for fn in (R.knn_loops, R.knn_fast):
        rows = fn(_set_of(q), _set_of(t0, t1, t2), R.Params(), 2)
        assert len(rows) == 1 and len(rows[0]) == 2 and list(rows[0]["distance"]) == [2.0, 3.0] and list(rows[0]["train_idx"]) == [0, 1]
    # "MatchStats computation" (:400-413)
    m = np.array([(0, 0, 10), (1, 1, 20), (2, 2, 30)], R.MATCH_DTYPE)
    assert R.stats(m) == (3, 20.0, 10.0, 30.0)


# ---- the library's host arithmetic and argument checks ----------------------------------------------------------------------
def test_match_stats_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 3, 100, 5000):
        m = np.zeros(n, zg.MATCH_DTYPE)
        m["distance"] = rng.integers(0, 257, n)
        if n == 100:
            m["distance"] += np.float32(0.1)  # sums that round
        got, want = zg.MatchStats.compute(m), R.stats(m)
        assert got.total_matches == want[0]
        assert np.array(got[1:], np.float32).tobytes() == np.array(want[1:], np.float32).tobytes(), n
    assert zg.MatchStats.compute(np.zeros(0, zg.MATCH_DTYPE)) == (0, 0.0, 0.0, 0.0)
    assert zg.MATCH_DTYPE == R.MATCH_DTYPE and zg.BINARY_DESCRIPTOR_DTYPE == R.DESC_DTYPE


def _set(data=0x10000, capacity=8, count=None):
    return L.ZgDescriptorSet(data, capacity, count)


def test_match_arguments_without_a_gpu():
    lib = zg.lib()
    p = L.ZgMatcherParams()
    lib.zg_matcher_default_params(ctypes.byref(p))
    assert (p.cross_check, p.max_distance) == (0, 64) and np.float32(p.ratio_threshold) == np.float32(0.8)
    assert lib.zg_match_train_chunk() >= 64
    out, cnt, rows = ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000), ctypes.c_void_p(0x40000)
    n = ctypes.c_uint32(7)
    ok, odd, big = _set(), _set(data=0x10001), _set(capacity=65536)
    B = ctypes.byref
    INV, UNS = L.ERR_INVALID_ARGUMENT, L.ERR_UNSUPPORTED
    for q, t in ((odd, ok), (ok, odd), (_set(data=0x10002), ok)):  # data that is not 4-byte aligned
        assert lib.zg_match_descriptors(B(q), B(t), B(p), out, 4, cnt, None) == INV
        assert b"aligned" in lib.zg_last_error()
        assert lib.zg_match_knn(B(q), B(t), B(p), 2, out, rows, None) == INV
        assert lib.zg_match_radius(B(q), B(t), 40.0, out, 4, rows, cnt, None) == INV
        assert lib.zg_match_descriptors_host(B(q), B(t), B(p), None, 0, B(n)) == INV
        assert lib.zg_match_knn_host(B(q), B(t), B(p), 2, None, rows) == INV
        assert lib.zg_match_radius_host(B(q), B(t), 40.0, None, 0, None, B(n)) == INV
    # the two 2^32 limits
    assert lib.zg_match_knn(B(big), B(ok), B(p), 65536, out, rows, None) == UNS
    assert lib.zg_match_knn_host(B(big), B(ok), B(p), 65536, None, rows) == UNS
    assert lib.zg_match_radius(B(big), B(big), 40.0, out, 4, rows, cnt, None) == UNS
    assert lib.zg_match_radius_host(B(big), B(big), 40.0, None, 0, None, B(n)) == UNS
    # NULL sets, parameters and outputs
    assert lib.zg_match_descriptors(None, B(ok), B(p), out, 4, cnt, None) == INV
    assert lib.zg_match_descriptors(B(ok), None, B(p), out, 4, cnt, None) == INV
    assert lib.zg_match_descriptors(B(ok), B(ok), None, out, 4, cnt, None) == INV
    assert lib.zg_match_descriptors(B(ok), B(ok), B(p), out, 4, None, None) == INV
    assert lib.zg_match_descriptors(B(ok), B(ok), B(p), None, 4, cnt, None) == INV
    assert lib.zg_match_descriptors(B(_set(data=None)), B(ok), B(p), out, 4, cnt, None) == INV
    assert lib.zg_match_knn(B(ok), B(ok), B(p), 2, None, rows, None) == INV
    assert lib.zg_match_knn(B(ok), B(ok), B(p), 2, out, None, None) == INV
    assert lib.zg_match_knn(B(ok), B(ok), None, 2, out, rows, None) == INV
    assert lib.zg_match_radius(B(ok), B(ok), 40.0, None, 4, rows, cnt, None) == INV
    assert lib.zg_match_radius(B(ok), B(ok), 40.0, out, 4, None, cnt, None) == INV
    assert lib.zg_match_radius(B(ok), B(ok), 40.0, out, 4, rows, None, None) == INV
    assert lib.zg_match_descriptors_host(B(ok), B(ok), B(p), None, 4, B(n)) == INV
    assert lib.zg_match_descriptors_host(B(ok), B(ok), B(p), None, 0, None) == INV
    assert lib.zg_match_knn_host(B(ok), B(ok), B(p), 2, None, None) == INV
    assert lib.zg_match_radius_host(B(ok), B(ok), 40.0, None, 4, None, B(n)) == INV
    assert lib.zg_match_stats(None, 3, B(L.ZgMatchStatistics())) == INV
    assert lib.zg_match_stats(None, 0, None) == INV
    assert n.value == 7  # nothing written


def test_python_binding_raises_before_device_work():
    q = np.zeros(3, zg.BINARY_DESCRIPTOR_DTYPE)
    with pytest.raises(zg.InvalidArgument):
        zg.BruteForceMatcher(max_distance=-1).match(q, q)
    with pytest.raises(zg.InvalidArgument):
        zg.BruteForceMatcher(max_distance=1 << 32).knn_match(q, q, 2)
    with pytest.raises(ValueError):
        zg.BruteForceMatcher().match(q, q, query_count=3)
    with pytest.raises(ValueError):
        zg.BruteForceMatcher().match_into(q, q, None, None)
    m = zg.BruteForceMatcher()
    assert (m.cross_check, m.max_distance, m.ratio_threshold) == (False, 64, 0.8)
    assert m.knn_match(q[:0], q, 2) == [] and m.knn_match(q, q, 0) == [] and m.radius_match(q, q[:0], 40.0) == []


# ---- the module's boundary: include/zignal_hip_match.h, _lib._MATCH_SIGNATURES and zig/zignal_hip_match.zig in step --------------
def _match_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zignal_hip_match.h")).read(), flags=re.S)
    protos = re.findall(r"ZG_API\s+[\w\s\*]+?\b(zg_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return {name: ([] if args.strip() == "void" else args.split(",")) for name, args in protos}


def test_match_header_bindings_and_zig_file_declare_the_same_symbols():
    protos = _match_header()
    assert sorted(protos) == sorted(L.MATCH_EXPORTED_SYMBOLS) and len(protos) == 9
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in protos.items():
        assert hasattr(raw, name), f"{name} declared in include/zignal_hip_match.h but not exported"
        assert len(L._MATCH_SIGNATURES[name]) == len(args), name
    assert not set(L.MATCH_EXPORTED_SYMBOLS) & (set(L.EXPORTED_SYMBOLS) | set(L.ORB_EXPORTED_SYMBOLS))
    shim = open(os.path.join(ROOT, "zig", "zignal_hip_match.zig")).read()
    externs = dict(re.findall(r"pub extern fn (zg_\w+)\(([^)]*)\)", shim))
    assert set(externs) == set(protos)
    for name, args in externs.items():
        assert len([a for a in args.split(",") if a.strip()]) == len(protos[name]), name
    main = open(os.path.join(ROOT, "include", "zignal_hip.h")).read()
    assert main.index('#include "zignal_hip_orb.h"') < main.index('#include "zignal_hip_match.h"')
    assert ctypes.sizeof(L.ZgMatch) == 12 and ctypes.sizeof(L.ZgMatcherParams) == 12
    assert ctypes.sizeof(L.ZgDescriptorSet) == 24 and L.ZgDescriptorSet.count.offset == 16
    assert ctypes.sizeof(L.ZgMatchStatistics) == 24
    makefile = open(os.path.join(ROOT, "zignal_amd", "csrc", "Makefile")).read()  # both object rules depend on every header of include/
    assert "$(wildcard ../../include/*.h)" in makefile and makefile.count("$(HEADERS)") == 2
    assert os.path.isfile(os.path.join(ROOT, "include", "zignal_hip_match.h"))


def test_every_match_entry_point_has_a_graph_replay_test_or_a_reason():
    """The rule of tests/test_gpu_graph_replay.py for this module: an asynchronous entry point is replayed from a graph on changed
    inputs somewhere, here in tests/test_gpu_match.py; the rest are host arithmetic or synchronous by contract."""
    replayed = {"zg_match_descriptors": "match_into", "zg_match_knn": "knn_match_into", "zg_match_radius": "radius_match_into"}
    host_math = {"zg_matcher_default_params", "zg_match_train_chunk", "zg_match_stats"}
    missing = [ep for ep in _match_header() if ep not in replayed and ep not in host_math and not ep.endswith("_host")]
    assert not missing, missing
    child = open(os.path.join(ROOT, "tests", "test_gpu_match.py")).read()
    assert "zg_graph_begin_capture" in child and "zg_graph_end_capture" in child and "zg_graph_launch" in child
    binding = open(os.path.join(ROOT, "zignal_amd", "match.py")).read()
    for ep, method in replayed.items():
        assert f"m.{method}(" in child, method
        assert re.search(rf"def {method}\(.*?lib\(\)\.{ep}\(", binding, flags=re.S), ep

"""CPU restatements of BruteForceMatcher (reference src/features/matcher.zig), twice and independently:

  *_loops   a literal transcription of the Zig loops (:44-233), one descriptor pair at a time;
  *_fast    numpy: a distance matrix from a 256-entry popcount table, np.partition-free min / second-min, argsort(kind="stable").

Both return MATCH_DTYPE arrays (lists of them for knn and radius) and, for match, coverage counters (COUNTERS) that say which
branches an input reached. `clustered` is the input generator of the matcher tests."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

MATCH_DTYPE = np.dtype([("query_idx", "<u4"), ("train_idx", "<u4"), ("distance", "<f4")])
DESC_DTYPE = np.dtype([("bits", "u1", (32,))])
MAXINT = 0xFFFFFFFF
COUNTERS = ("accepted", "far", "ratio", "tie", "at_max", "lone", "cross_rej", "cross_acc")
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint16)


@dataclass
class Params:
    cross_check: bool = False
    max_distance: int = 64
    ratio_threshold: float = 0.8

    def kwargs(self):
        return {"cross_check": self.cross_check, "max_distance": self.max_distance, "ratio_threshold": self.ratio_threshold}


def bits(des) -> np.ndarray:
    """(n, 32) uint8 from a DESC_DTYPE array or anything shaped like it."""
    a = np.asarray(des)
    if a.dtype == DESC_DTYPE:
        a = a["bits"]
    return np.ascontiguousarray(a, np.uint8).reshape(-1, 32)


def as_descriptors(b: np.ndarray) -> np.ndarray:
    out = np.zeros(len(b), DESC_DTYPE)
    out["bits"] = b
    return out


def hamming(a: np.ndarray, b: np.ndarray) -> int:  # BinaryDescriptor.hammingDistance
    return int(POPCOUNT[a ^ b].sum())


def _counters() -> Dict[str, int]:
    return dict.fromkeys(COUNTERS, 0)


def _list(rows) -> np.ndarray:
    out = np.zeros(len(rows), MATCH_DTYPE)
    for i, (q, t, d) in enumerate(rows):
        out[i] = (q, t, np.float32(d))
    return out


# ---- the loops, as written -------------------------------------------------------------------------------------------------
def _find_best_loops(desc, others) -> int:  # :215-233
    best_dist, best_idx = MAXINT, 0
    for t_idx, t in enumerate(others):
        dist = hamming(desc, t)
        if dist < best_dist:
            best_dist, best_idx = dist, t_idx
    return best_idx


def match_loops(query, train, p: Params) -> Tuple[np.ndarray, Dict[str, int]]:
    q, t = bits(query), bits(train)
    c = _counters()
    if len(q) == 0 or len(t) == 0:
        return np.zeros(0, MATCH_DTYPE), c
    ratio = np.float32(p.ratio_threshold)
    rows = []
    for q_idx, qd in enumerate(q):
        best, second, best_idx = MAXINT, MAXINT, 0
        for t_idx, td in enumerate(t):
            dist = hamming(qd, td)
            if dist < best:
                second, best, best_idx = best, dist, t_idx
            elif dist < second:
                second = dist
        best_f, second_f = np.float32(best), np.float32(second)
        c["tie"] += best == second
        c["at_max"] += best == p.max_distance
        c["lone"] += second == MAXINT
        if best > p.max_distance:
            c["far"] += 1
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            passes = second == MAXINT or bool(best_f < ratio * second_f)
        if not passes:
            c["ratio"] += 1
            continue
        if p.cross_check:
            if _find_best_loops(t[best_idx], q) != q_idx:
                c["cross_rej"] += 1
                continue
            c["cross_acc"] += 1
        c["accepted"] += 1
        rows.append((q_idx, best_idx, best))
    return _list(rows), c


def _stable_sort_by_distance(rows):  # std.mem.sort is a stable insertion sort; so is this
    out = []
    for r in rows:
        i = len(out)
        while i > 0 and r[2] < out[i - 1][2]:
            i -= 1
        out.insert(i, r)
    return out


def knn_loops(query, train, p: Params, k: int) -> List[np.ndarray]:
    q, t = bits(query), bits(train)
    if len(q) == 0 or len(t) == 0 or k == 0:
        return []
    out = []
    for q_idx, qd in enumerate(q):
        distances = _stable_sort_by_distance([(q_idx, t_idx, hamming(qd, td)) for t_idx, td in enumerate(t)])
        out.append(_list([m for m in distances[: min(k, len(distances))] if np.float32(m[2]) <= np.float32(p.max_distance)]))
    return out


def radius_loops(query, train, max_dist: float) -> List[np.ndarray]:
    q, t = bits(query), bits(train)
    if len(q) == 0 or len(t) == 0:
        return []
    md = np.float32(max_dist)
    out = []
    for q_idx, qd in enumerate(q):
        rows = []
        for t_idx, td in enumerate(t):
            dist = hamming(qd, td)
            if np.float32(dist) <= md:  # False for NaN
                rows.append((q_idx, t_idx, dist))
        out.append(_list(_stable_sort_by_distance(rows)))
    return out


# ---- numpy -------------------------------------------------------------------------------------------------------------
def distance_matrix(query, train) -> np.ndarray:
    q, t = bits(query), bits(train)
    d = np.zeros((len(q), len(t)), np.int64)
    for j in range(32):
        d += POPCOUNT[q[:, j, None] ^ t[None, :, j]]
    return d


def match_fast(query, train, p: Params) -> Tuple[np.ndarray, Dict[str, int]]:
    c = _counters()
    d = distance_matrix(query, train)
    nq, nt = d.shape
    if nq == 0 or nt == 0:
        return np.zeros(0, MATCH_DTYPE), c
    best_idx = d.argmin(axis=1)  # the first of equals
    best = d[np.arange(nq), best_idx]
    if nt > 1:
        second = np.sort(d, axis=1)[:, 1]
    else:
        second = np.full(nq, MAXINT, np.int64)
    near = best <= p.max_distance
    with np.errstate(invalid="ignore", over="ignore"):
        passes = (second == MAXINT) | (best.astype(np.float32) < np.float32(p.ratio_threshold) * second.astype(np.float32))
    keep = near & passes
    c["tie"] = int((best == second).sum())
    c["at_max"] = int((best == p.max_distance).sum())
    c["lone"] = int((second == MAXINT).sum())
    c["far"] = int((~near).sum())
    c["ratio"] = int((near & ~passes).sum())
    if p.cross_check:
        mutual = d.argmin(axis=0)[best_idx] == np.arange(nq)
        c["cross_rej"] = int((keep & ~mutual).sum())
        c["cross_acc"] = int((keep & mutual).sum())
        keep &= mutual
    c["accepted"] = int(keep.sum())
    out = np.zeros(int(keep.sum()), MATCH_DTYPE)
    out["query_idx"] = np.nonzero(keep)[0]
    out["train_idx"] = best_idx[keep]
    out["distance"] = best[keep]
    return out, c


def _rows_fast(d: np.ndarray, lengths, order) -> List[np.ndarray]:
    out = []
    for qi in range(d.shape[0]):
        idx = order[qi, : lengths[qi]]
        r = np.zeros(len(idx), MATCH_DTYPE)
        r["query_idx"], r["train_idx"], r["distance"] = qi, idx, d[qi, idx]
        out.append(r)
    return out


def knn_fast(query, train, p: Params, k: int) -> List[np.ndarray]:
    d = distance_matrix(query, train)
    nq, nt = d.shape
    if nq == 0 or nt == 0 or k == 0:
        return []
    order = np.argsort(d, axis=1, kind="stable")
    top = np.take_along_axis(d, order[:, : min(k, nt)], axis=1)
    return _rows_fast(d, (top <= p.max_distance).sum(axis=1), order)  # sorted: the kept ones come first


def radius_fast(query, train, max_dist: float) -> List[np.ndarray]:
    d = distance_matrix(query, train)
    nq, nt = d.shape
    if nq == 0 or nt == 0:
        return []
    order = np.argsort(d, axis=1, kind="stable")
    with np.errstate(invalid="ignore"):
        inside = d.astype(np.float32) <= np.float32(max_dist)
    return _rows_fast(d, inside.sum(axis=1), order)


def stats(matches) -> Tuple[int, np.float32, np.float32, np.float32]:  # MatchStats.compute (:243-269)
    m = np.asarray(matches)
    if len(m) == 0:
        return 0, np.float32(0), np.float32(0), np.float32(0)
    s, lo, hi = np.float32(0), np.finfo(np.float32).max, np.float32(0)
    for v in m["distance"]:
        s = np.float32(s + v)
        lo, hi = min(lo, v), max(hi, v)
    return len(m), np.float32(s / np.float32(len(m))), np.float32(lo), np.float32(hi)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def flip(desc: np.ndarray, positions) -> np.ndarray:
    out = desc.copy()
    for b in positions:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def clustered(seed: int, nq: int, nt: int) -> Tuple[np.ndarray, np.ndarray]:
    """(query, train) as DESC_DTYPE arrays whose distances spread over the matcher's branches: random train descriptors of which about
    4 % are exact copies of an earlier one and about 6 % copies with 1 .. 39 bits flipped; a fifth of the queries random, the others
    a train entry with one of {0, 3, 10, 30, 60, 64, 65, 90} bits flipped; a tenth of the queries then overwritten with an earlier
    query. (Uniformly random descriptors alone sit near distance 128 and fail the default max_distance = 64 every time.)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for i in range(1, nt):
        u = rng.random()
        if u < 0.04:
            t[i] = t[rng.integers(0, i)]
        elif u < 0.10:
            t[i] = flip(t[rng.integers(0, i)], rng.choice(256, int(rng.integers(1, 40)), replace=False))
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    flips = (0, 3, 10, 30, 60, 64, 65, 90)
    for i in range(nq):
        if nt and rng.random() >= 0.2:
            q[i] = flip(t[rng.integers(0, nt)], rng.choice(256, flips[int(rng.integers(0, len(flips)))], replace=False))
    for i in range(1, nq):
        if rng.random() < 0.1:
            q[i] = q[rng.integers(0, i)]
    return as_descriptors(q), as_descriptors(t)

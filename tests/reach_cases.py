"""What the mutual-reachability forest tests hold an answer to (tests/test_gpu_reach_forest.py, tests/reach_worker.py,
tests/test_reach_model.py).

Nothing here comes from the code under test.  The pairs are self_join_cases.brute_pairs — brute force on the code bytes; a
row's core distance is the (M - 1)-th smallest distance among the pairs it is in, NONE where it is in fewer; a pair's weight is
max(distance, core[a], core[b]); the partition at t is components_cases.labels_from_pairs — a plain union-find — over the pairs
of weight <= t.  The forest itself is not unique (which of several pairs of equal weight joins two sets is free), so it is held
to its contract and never to bytes."""
import hashlib

import numpy as np

from smafa_amd import HIT_DTYPE
from components_cases import labels_from_pairs, labels_from_pairs_numpy
from forest_cases import walk_forest
from self_join_cases import brute_pairs

NONE = 0xFFFFFFFF
_EXPECTED = {}


def cores_from_pairs(n, pairs, M):
    """pairs (HIT_DTYPE, each unordered pair once, every pair within the bound) -> uint32 core[n]"""
    M = max(int(M), 1)
    if M == 1:
        return np.zeros(n, dtype=np.uint32)
    who = np.concatenate([pairs["query"], pairs["subject"]]).astype(np.int64)
    dist = np.concatenate([pairs["dist"], pairs["dist"]]).astype(np.int64)
    order = np.lexsort((dist, who))  # by row, then by distance
    who, dist = who[order], dist[order]
    degree = np.bincount(who, minlength=n)
    start = np.concatenate([[0], np.cumsum(degree)[:-1]])
    cores = np.full(n, NONE, dtype=np.uint32)
    full = degree >= M - 1  # the row and M - 1 others: the ball holds M
    cores[full] = dist[start[full] + M - 2]
    return cores


def brute_cores(codes, D, M):
    """per row the (M - 1)-th smallest distance to another row within D, or NONE"""
    n, L = codes.shape
    return cores_from_pairs(n, brute_pairs(codes, min(D, L)), M)


def weighted_pairs(codes, D, M):
    """-> (cores, the brute pairs whose ends are both not sparse, their weights int64)"""
    n, L = codes.shape
    pairs = brute_pairs(codes, min(D, L))
    cores = cores_from_pairs(n, pairs, M)
    ca, cb = cores[pairs["query"]].astype(np.int64), cores[pairs["subject"]].astype(np.int64)
    w = np.maximum(pairs["dist"].astype(np.int64), np.maximum(ca, cb))
    live = w <= D  # (NONE is above every bound)
    return cores, pairs[live], w[live]


def expected_reach(codes, D, M):
    """(cores, labels (D + 1, n) uint32, set counts) by brute force, computed once per store, bound and min_pts"""
    key = (hashlib.sha1(np.ascontiguousarray(codes).tobytes()).hexdigest(), codes.shape, int(D), int(M))
    if key not in _EXPECTED:
        n = len(codes)
        cores, pairs, w = weighted_pairs(codes, D, M)
        labels = np.zeros((D + 1, n), dtype=np.uint32)
        for t in range(D + 1):
            cut = pairs[w <= t]  # (the same labels from either union-find; the Python loop is too slow for millions of pairs)
            labels[t] = labels_from_pairs(n, cut) if len(cut) < 500_000 else labels_from_pairs_numpy(n, cut)
        counts = [int((labels[t] == np.arange(n)).sum()) for t in range(D + 1)]
        cores.setflags(write=False)
        labels.setflags(write=False)
        _EXPECTED[key] = (cores, labels, counts)
    return _EXPECTED[key]


def check_reach_forest(codes, edges, level_ends, cores, D, M):
    """the whole contract of include/smafa_amd.h, against brute force on the code bytes; -> the set counts per level"""
    n = len(codes)
    want_cores, want, counts = expected_reach(codes, D, M)
    assert isinstance(edges, np.ndarray) and isinstance(level_ends, np.ndarray) and isinstance(cores, np.ndarray)
    assert edges.dtype == HIT_DTYPE and edges.ndim == 1, (edges.dtype, edges.shape)
    assert level_ends.dtype == np.uint64 and level_ends.shape == (D + 1,), (level_ends.dtype, level_ends.shape)
    assert cores.dtype == np.uint32 and cores.shape == (n,), (cores.dtype, cores.shape)
    assert cores.tobytes() == want_cores.tobytes(), "cores differ from brute force at rows %s" % np.flatnonzero(cores != want_cores)[:8]
    assert len(edges) <= max(n - 1, 0) and len(edges) == int(level_ends[-1])
    a, b, w = (edges[k].astype(np.int64) for k in ("query", "subject", "dist"))
    assert (a < b).all() and (b < n).all()
    true = (codes[a] != codes[b]).sum(axis=1) if len(edges) else np.zeros(0, dtype=np.int64)
    big = want_cores.astype(np.int64)
    assert (w == np.maximum(true, np.maximum(big[a], big[b]))).all(), "an edge's dist is not max(distance, core[a], core[b])"
    assert (w <= D).all()
    assert (np.diff(w) >= 0).all(), "the weight decreases along the list"
    for t in range(D + 1):
        assert int(level_ends[t]) == int((w <= t).sum()), (t, level_ends.tolist())
    for t, labels in walk_forest(n, edges, level_ends):  # (every edge joins two sets)
        assert labels.tobytes() == want[t].tobytes(), "level %d: the edges up to it do not connect the graph cut at weight %d" % (t, t)
        assert int(level_ends[t]) == n - counts[t], (t, level_ends.tolist(), counts)
    return counts

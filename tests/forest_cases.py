"""What the forest tests hold an answer to (tests/test_gpu_forest.py, tests/forest_worker.py, tests/test_forest_model.py).

Nothing here comes from the code under test: the expected partitions are levels_cases.brute_levels — brute force on the code
bytes, a plain union-find per level — and the distances of the edges are recomputed from the code bytes.  The forest itself
is not unique (which of several pairs of equal distance joins two sets is free), so it is held to its contract, not to
bytes: edges a < b at their true distance, ordered by distance, level_ends their counts per level, acyclic, and after the
edges of level t exactly the components at bound t."""
import hashlib

import numpy as np

from smafa_amd import HIT_DTYPE
from levels_cases import brute_levels

_EXPECTED = {}


def expected_levels(codes, D):
    """(labels, counts, number of pairs within min(D, L)) of brute_levels(codes, D), computed once per store and bound"""
    key = (hashlib.sha1(np.ascontiguousarray(codes).tobytes()).hexdigest(), codes.shape, int(D))
    if key not in _EXPECTED:
        labels, counts, pairs = brute_levels(codes, D)
        labels.setflags(write=False)
        _EXPECTED[key] = (labels, counts, len(pairs))
    return _EXPECTED[key]


def walk_forest(n, edges, level_ends):
    """The edges in the order given through a plain union-find (the larger root under the smaller, so a root is its set's
    minimum): asserts that EVERY edge joins two different sets, and yields (t, labels) after the edges of level t,
    labels[i] = the smallest member of i's set."""
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    a, b = edges["query"].tolist(), edges["subject"].tolist()
    done = 0
    for t, end in enumerate(int(e) for e in level_ends):
        for k in range(done, end):
            ra, rb = find(a[k]), find(b[k])
            assert ra != rb, "edge %d (%d, %d) closes a cycle" % (k, a[k], b[k])
            parent[max(ra, rb)] = min(ra, rb)
        done = max(done, end)
        labels = np.array(parent, dtype=np.int64) if n else np.zeros(0, dtype=np.int64)
        while True:  # every root is a minimum and parent[x] <= x: jumping ends at it
            jumped = labels[labels]
            if (jumped == labels).all():
                break
            labels = jumped
        yield t, labels.astype(np.uint32)


def check_shape(codes, edges, level_ends, D):
    """everything of the contract that needs no expected partition; -> edges as HIT_DTYPE"""
    n = len(codes)
    assert isinstance(edges, np.ndarray) and isinstance(level_ends, np.ndarray)
    assert edges.dtype == HIT_DTYPE and edges.ndim == 1, (edges.dtype, edges.shape)
    assert level_ends.dtype == np.uint64 and level_ends.shape == (D + 1,), (level_ends.dtype, level_ends.shape)
    assert len(edges) <= max(n - 1, 0) and len(edges) == (int(level_ends[-1]) if D >= 0 else 0)
    a, b, d = (edges[k].astype(np.int64) for k in ("query", "subject", "dist"))
    assert (a < b).all() and (b < n).all()
    true = (codes[a] != codes[b]).sum(axis=1) if len(edges) else np.zeros(0, dtype=np.int64)
    assert (d == true).all(), "an edge's dist is not the distance of its rows"
    assert (d <= D).all()
    assert (np.diff(d) >= 0).all(), "dist decreases along the list"
    for t in range(D + 1):
        assert int(level_ends[t]) == int((d <= t).sum()), (t, level_ends.tolist())
    return edges


def check_forest(codes, edges, level_ends, D):
    """the whole contract of include/smafa_amd.h, against brute force on the code bytes"""
    n = len(codes)
    want, counts, _ = expected_levels(codes, D)
    check_shape(codes, edges, level_ends, D)
    for t, labels in walk_forest(n, edges, level_ends):
        assert labels.tobytes() == want[t].tobytes(), "level %d: the edges up to it do not connect the components at bound %d" % (t, t)
        assert int(level_ends[t]) == n - counts[t], (t, level_ends.tolist(), counts)
    return counts


def as_edges(rows):
    """device or parsed rows (m x 3: a, b, dist) -> HIT_DTYPE, order kept"""
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 3)
    return rows.view(HIT_DTYPE).reshape(-1)


def sorted_inside_levels(edges):
    """the host form's order: (dist, query, subject)"""
    order = np.lexsort((edges["subject"], edges["query"], edges["dist"]))
    return bool((order == np.arange(len(edges))).all())

"""smafa_amd.forest_linkage (numpy only): the linkage matrix of a forest, in the layout scipy.cluster.hierarchy documents.

The cutter here is the test's own: clusters n, n + 1, .. are the merges in order, and cutting at height t takes every merge
with height <= t.  The partition it gives must be the union-find partition of the edges with dist <= t."""
import numpy as np
import pytest

import smafa_amd
from smafa_amd import HIT_DTYPE
from components_cases import labels_from_pairs


def edges_of(rows):
    out = np.zeros(len(rows), dtype=HIT_DTYPE)
    for k, (a, b, d) in enumerate(rows):
        out[k] = (a, b, d)
    return out


def cut(Z, n, height):
    """-> labels[n]: the smallest row of each cluster after the merges with height <= `height`, and the sizes checked on the way"""
    members = {i: [i] for i in range(n)}
    for k, (a, b, h, size) in enumerate(Z.tolist()):
        a, b = int(a), int(b)
        assert a < b < n + k and a in members and b in members, (k, a, b)  # both exist and neither was merged before
        assert size == len(members[a]) + len(members[b]), k
        if h <= height:
            members[n + k] = members.pop(a) + members.pop(b)
        else:  # (heights never decrease: nothing below is cut apart again)
            members[n + k] = []
            assert all(later[2] >= h for later in Z[k:].tolist())
            break
    labels = np.zeros(n, dtype=np.uint32)
    for rows in members.values():
        for i in rows:
            labels[i] = min(rows)
    return labels


# 9 rows: {0, 3, 4, 7} joined at 0, 0, 2; {1, 5} at 1; {2, 6, 8} at 1, 3 — three trees at bound 3
THREE_TREES = [(0, 4, 0), (3, 7, 0), (1, 5, 1), (2, 8, 1), (3, 4, 2), (6, 8, 3)]


@pytest.mark.parametrize("structured", [True, False])
def test_three_trees(structured):
    n, D = 9, 3
    edges = edges_of(THREE_TREES)
    given = edges if structured else np.array(THREE_TREES, dtype=np.uint32)
    Z = smafa_amd.forest_linkage(given, n, D)
    assert Z.shape == (n - 1, 4) and Z.dtype == np.float64
    assert Z[:6, 2].tolist() == [0, 0, 1, 1, 2, 3] and Z[6:, 2].tolist() == [D + 1, D + 1]  # the last merges are at D + 1
    assert Z[:, 3].tolist() == [2, 2, 2, 2, 4, 3, 6, 9]  # the trees in order of their smallest member: {0..} + {1, 5}, then + {2..}
    assert Z[0].tolist() == [0, 4, 0, 2] and Z[4].tolist() == [9, 10, 2, 4] and Z[6].tolist() == [11, 13, 4, 6] and Z[7].tolist() == [14, 15, 4, 9]
    for t in range(D + 1):
        assert cut(Z, n, t).tobytes() == labels_from_pairs(n, edges[edges["dist"] <= t]).tobytes(), t
    assert not cut(Z, n, D + 1).any()
    assert Z[-1, 3] == n  # sizes add up


def test_a_spanning_tree_and_the_order_given():
    """one tree: no merge above the bound; the edges are taken in the order given, also where that is not by height"""
    rows = [(0, 1, 2), (2, 3, 0), (1, 2, 1)]
    Z = smafa_amd.forest_linkage(edges_of(rows), 4, 2)
    assert Z.tolist() == [[0, 1, 2, 2], [2, 3, 0, 2], [4, 5, 1, 4]]


def test_random_forests():
    rng = np.random.default_rng(3)
    for _ in range(20):
        n, D = int(rng.integers(2, 40)), 5
        rows, seen = [], list(range(n))
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        for d in sorted(rng.integers(0, D + 1, size=n).tolist()):
            a, b = sorted(rng.choice(seen, size=2, replace=False).tolist())
            if find(a) != find(b):
                parent[find(b)] = find(a)
                rows.append((a, b, d))
        edges = edges_of(rows)
        Z = smafa_amd.forest_linkage(edges, n, D)
        assert Z.shape == (n - 1, 4) and Z[-1, 3] == n
        assert (Z[len(rows):, 2] == D + 1).all() and (Z[:len(rows), 2] == edges["dist"]).all()
        for t in range(D + 1):
            assert cut(Z, n, t).tobytes() == labels_from_pairs(n, edges[edges["dist"] <= t]).tobytes(), t


def test_edges_and_errors():
    assert smafa_amd.forest_linkage(edges_of([]), 0, 3).shape == (0, 4)
    assert smafa_amd.forest_linkage(edges_of([]), 1, 3).shape == (0, 4)
    assert smafa_amd.forest_linkage(edges_of([]), 3, 3).tolist() == [[0, 1, 4, 2], [2, 3, 4, 3]]
    with pytest.raises(ValueError):
        smafa_amd.forest_linkage(edges_of([(0, 1, 0), (1, 2, 0), (0, 2, 1)]), 3, 3)  # a cycle
    with pytest.raises(ValueError):
        smafa_amd.forest_linkage(edges_of([(0, 5, 0)]), 3, 3)

"""A host model of hook_levels_kernel's early stop (smafa_amd/csrc/levels.hip.h), CPU only.

Every lane is a generator that yields in front of each access to parent[] (load, atomicMin, atomicCAS — the operations of
smafa_cc::find_root / unite), and a random scheduler interleaves the lanes one access at a time.  A lane works its row
(a, b, d) upwards from level d and LEAVES THE ROW at the first level where it loads equal parents.  Whatever the interleaving,
every level must end as the components of the edges with dist <= t, each root its set's minimum — the claim the header
proves.  The expectation is components_cases.labels_from_pairs, nothing of the model's."""
import random

import numpy as np
import pytest

from components_cases import labels_from_pairs


def find_root(parent, x):
    while True:
        yield
        p = parent[x]
        if p == x:
            return x
        yield
        g = parent[p]
        if g == p:
            return p
        yield
        parent[x] = min(parent[x], g)  # atomicMin
        x = g


def unite(parent, a, b):
    ra = yield from find_root(parent, a)
    rb = yield from find_root(parent, b)
    while ra != rb:
        hi, lo = max(ra, rb), min(ra, rb)
        yield
        seen = parent[hi]  # atomicCAS(parent + hi, hi, lo)
        if seen == hi:
            parent[hi] = lo
            return
        ra = yield from find_root(parent, seen)
        rb = yield from find_root(parent, lo)


def lane(parents, a, b, d, early_stop):
    if a == b:
        return
    for t in range(d, len(parents)):
        if early_stop:
            yield
            pa = parents[t][a]
            yield
            pb = parents[t][b]
            if pa == pb:
                return
        yield from unite(parents[t], a, b)


def run(n, rows, E, seed, early_stop=True):
    rng = random.Random(seed)
    parents = [list(range(n)) for _ in range(E)]
    lanes = [lane(parents, a, b, d, early_stop) for a, b, d in rows]
    while lanes:
        k = rng.randrange(len(lanes))
        try:
            next(lanes[k])
        except StopIteration:
            lanes[k] = lanes[-1]
            lanes.pop()
    labels = np.zeros((E, n), dtype=np.uint32)
    for t in range(E):
        for i in range(n):
            x = i
            while parents[t][x] != x:
                x = parents[t][x]
            labels[t, i] = x
    return labels


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("early_stop", [True, False])
def test_every_level_under_random_interleavings(seed, early_stop):
    rng = np.random.default_rng(seed)
    n, E = 40, 5
    m = int(rng.integers(20, 120))
    a, b = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    d = rng.integers(0, E, size=m)
    # the list as the kernel receives it: mirror images and repeats of some rows, and self-pairs
    extra = rng.integers(0, m, size=m // 2)
    a, b, d = np.r_[a, b[extra], np.arange(5)], np.r_[b, a[extra], np.arange(5)], np.r_[d, d[extra], np.zeros(5, dtype=np.int64)]
    rows = list(zip(a.tolist(), b.tolist(), d.tolist()))
    got = run(n, rows, E, seed, early_stop)
    edges = np.zeros(len(rows), dtype=[("query", "<u4"), ("subject", "<u4"), ("dist", "<u4")])
    edges["query"], edges["subject"], edges["dist"] = a, b, d
    for t in range(E):
        want = labels_from_pairs(n, edges[edges["dist"] <= t])
        assert got[t].tobytes() == want.tobytes(), t
    assert len({int((got[t] == np.arange(n)).sum()) for t in range(E)}) >= 3  # the levels differ


def test_one_dense_family_many_lanes():
    """every pair of 12 rows at distance 1, with mirrors: most lanes meet joined sets at their own level and leave"""
    n, E = 12, 4
    rows = [(i, j, 1) for i in range(n) for j in range(n)]
    for seed in range(6):
        got = run(n, rows, E, seed)
        assert (got[0] == np.arange(n)).all() and not got[1:].any()

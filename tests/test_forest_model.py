"""A host model of span_edges_kernel's union (smafa_amd/csrc/forest.hip.h: unite_won), CPU only.

Every lane is a generator that yields in front of each access to parent[] (load, atomicMin, atomicCAS — the operations of
smafa_cc::find_root and of unite_won's hook), and a scheduler interleaves the lanes one access at a time, as
tests/test_levels_model.py does.  A lane whose own CAS made the hook appends its row to the edge list.
  * Class by class — every lane of distance t has finished before a lane of t + 1 starts, the kernel boundary of the host's
    schedule — the winners are a minimum spanning forest whatever the interleaving inside a class: they pass
    forest_cases.check_forest, whose expectation is brute force on the code bytes.
  * All classes interleaved — what ONE launch over all distances would do — the winners still span, acyclically, but the
    scheduler can be driven to a forest that is not minimum on two cliques of equal rows at distance 3 from each other: two
    heavy rows win while their ends are still alone, and a light row that would have been needed finds its ends joined.
    This is why the boundary is there.  It checks the argument, not the kernel."""
import random

import numpy as np
import pytest

from smafa_amd import HIT_DTYPE
from forest_cases import check_forest, check_shape, walk_forest
from self_join_cases import brute_pairs, planted_store


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


def unite_won(parent, a, b):
    ra = yield from find_root(parent, a)
    rb = yield from find_root(parent, b)
    while ra != rb:
        hi, lo = max(ra, rb), min(ra, rb)
        yield
        seen = parent[hi]  # atomicCAS(parent + hi, hi, lo)
        if seen == hi:
            parent[hi] = lo
            return True
        ra = yield from find_root(parent, seen)
        rb = yield from find_root(parent, lo)
    return False


def lane(parent, a, b, d, edges):
    if a == b:
        return
    yield
    pa = parent[a]
    yield
    pb = parent[b]
    if pa == pb:  # the early-out: one set already
        return
    if (yield from unite_won(parent, a, b)):
        edges.append((min(a, b), max(a, b), d))


def run_lanes(lanes, rng):
    while lanes:
        k = rng.randrange(len(lanes))
        try:
            next(lanes[k])
        except StopIteration:
            lanes[k] = lanes[-1]
            lanes.pop()


def finish(n, D, edges):
    out = np.zeros(len(edges), dtype=HIT_DTYPE)
    if edges:
        out["query"], out["subject"], out["dist"] = (np.array(c, dtype=np.uint32) for c in zip(*edges))
    ends = np.array([sum(1 for e in edges if e[2] <= t) for t in range(D + 1)], dtype=np.uint64)
    return out, ends


def span(n, rows, D, seed, by_class=True, first=()):
    """rows (a, b, d) -> (edges, level_ends) of the model; by_class: a boundary behind every distance; first: rows whose lanes run
    to their end, one after another, before the scheduler takes over (an interleaving like any other)"""
    rng = random.Random(seed)
    parent = list(range(n))
    edges = []
    for a, b, d in first:
        run_lanes([lane(parent, a, b, d, edges)], rng)
    for t in (range(D + 1) if by_class else [None]):
        run_lanes([lane(parent, a, b, d, edges) for a, b, d in rows if t is None or d == t], rng)
    if not by_class:  # one launch has no order among its rows: the list is ordered afterwards, as the host form would
        edges.sort(key=lambda e: e[2])
    return finish(n, D, edges)


def with_mirrors(pairs, rng):
    """the list as the kernel receives a raw piece: mirror images and repeats of some rows, and self-pairs"""
    rows = [(int(r["query"]), int(r["subject"]), int(r["dist"])) for r in pairs]
    rows += [(b, a, d) for a, b, d in rows if rng.random() < 0.5]
    rows += [rows[rng.randrange(len(rows))] for _ in range(len(rows) // 4)] if rows else []
    rows += [(i, i, 0) for i in range(5)]
    rng.shuffle(rows)
    return rows


@pytest.mark.parametrize("seed", range(12))
def test_class_by_class_is_a_minimum_forest(seed):
    D, L = 4, 8
    codes = planted_store(100 + seed, "nt", L, 5, members=8, max_subs=2, copies=6)  # 46 rows in 5 families
    n = len(codes)
    pairs = brute_pairs(codes, D)
    assert len(set(pairs["dist"].tolist())) >= 3
    rows = with_mirrors(pairs, random.Random(seed))
    edges, ends = span(n, rows, D, seed)
    counts = check_forest(codes, edges, ends, D)
    assert len(set(counts)) >= 3, counts  # the levels differ


def two_cliques(k=6):
    a = np.zeros(8, dtype=np.uint8)
    b = a.copy()
    b[[1, 4, 7]] = 1
    codes = np.array([a, b] * k, dtype=np.uint8)  # even rows: one clique, odd rows: the other, at distance 3
    return codes, brute_pairs(codes, 3)


@pytest.mark.parametrize("seed", range(6))
def test_two_cliques_class_by_class(seed):
    codes, pairs = two_cliques()
    n = len(codes)
    rows = with_mirrors(pairs, random.Random(seed))
    edges, ends = span(n, rows, 3, seed)
    check_forest(codes, edges, ends, 3)
    assert ends.tolist() == [n - 2, n - 2, n - 2, n - 1]


def test_all_classes_in_one_launch_can_miss_the_minimum():
    """two heavy rows, (0, 1) and (2, 3), run first: each finds its ends alone and wins.  The light row (0, 2) then joins the two
    pairs, and NO light row between 1 and 3 can win any more: one light edge fewer, one heavy edge more."""
    codes, pairs = two_cliques()
    n = len(codes)
    rows = [(int(r["query"]), int(r["subject"]), int(r["dist"])) for r in pairs]
    assert (0, 1, 3) in rows and (2, 3, 3) in rows and (0, 2, 0) in rows and (1, 3, 0) in rows
    edges, ends = span(n, rows, 3, 0, by_class=False, first=[(0, 1, 3), (2, 3, 3)])
    check_shape(codes, edges, ends, 3)                 # true distances, ordered, counted
    labels = [row for _, row in walk_forest(n, edges, ends)]  # acyclic
    assert not labels[3].any() and int(ends[3]) == n - 1      # and it spans
    assert int(ends[0]) < n - 2 and int((edges["dist"] == 3).sum()) >= 2  # but it is not minimum
    with pytest.raises(AssertionError):
        check_forest(codes, edges, ends, 3)
    # the same rows and the same two lanes first, with the boundary: the heavy lanes only START once every light lane has ended
    edges, ends = span(n, rows, 3, 0, by_class=True)
    check_forest(codes, edges, ends, 3)

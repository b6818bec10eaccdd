"""The stable-cluster selection without a GPU: tests/stable_cases.select_stable — the answer every GPU test is held to — on
hierarchies worked out by hand, the expected labels written out; and the GPU fixtures' expected answers held to what they must
contain, so that no fixture can quietly degrade to one cluster."""
import numpy as np

from reach_cases import NONE, expected_reach
from stable_cases import FIXTURES, expected_stable, select_stable, sizes, traits

X = NONE


def hierarchy(n, levels):
    """levels: per level the sets of more than one row -> the (levels, n) labels, the smallest row of every row's set"""
    labels = np.tile(np.arange(n, dtype=np.uint32), (len(levels), 1))
    for t, groups in enumerate(levels):
        for g in groups:
            labels[t, list(g)] = min(g)
    return labels


def select(n, levels, S, cores=None):
    cores = np.zeros(n, dtype=np.uint32) if cores is None else np.array(cores, dtype=np.uint32)
    labels, joined, count = select_stable(cores, hierarchy(n, levels), S)
    return labels.tolist(), joined.tolist(), count


def test_children_beat_the_parent():
    """two sets of three live three levels (9 each), their union one (6): 18 > 6"""
    a, b = (0, 1, 2), (3, 4, 5)
    got = select(8, [[a, b], [a, b], [a, b], [a + b]], 2)
    assert got == ([0, 0, 0, 3, 3, 3, X, X], [0, 0, 0, 0, 0, 0, X, X], 2)


def test_the_parent_beats_the_children():
    """two pairs live one level (2 each), their union with two more rows three (6 + 7 + 7 = 20); row 6 joins at level 2"""
    u = (0, 1, 2, 3, 4, 5)
    got = select(8, [[(0, 1), (2, 3)], [u], [u + (6,)], [u + (6,)]], 2)
    assert got == ([0, 0, 0, 0, 0, 0, 0, X], [1, 1, 1, 1, 1, 1, 2, X], 1)


def test_an_exact_tie_goes_to_the_parent():
    """2 + 2 against 4"""
    assert select(4, [[(0, 1), (2, 3)], [(0, 1, 2, 3)]], 2) == ([0, 0, 0, 0], [1, 1, 1, 1], 1)
    # one level more for the children: 4 + 4 against 4
    assert select(4, [[(0, 1), (2, 3)], [(0, 1), (2, 3)], [(0, 1, 2, 3)]], 2) == ([0, 0, 2, 2], [0, 0, 0, 0], 2)


def test_grandchildren_pass_through_a_losing_middle():
    """three sets of three; two of them (9 + 9 after three levels) merge into a middle cluster that lives one level (6), the third
    lives four (12); the root lives three levels (27).  The middle's own stability would lose to the root (6 + 12 <= 27), what
    passes through it does not (18 + 12 > 27)"""
    a, b, c = (0, 1, 2), (3, 4, 5), (6, 7, 8)
    low = [a, b, c]
    got = select(9, [low, low, low, [a + b, c], [a + b + c], [a + b + c], [a + b + c]], 2)
    assert got == ([0, 0, 0, 3, 3, 3, 6, 6, 6], [0] * 9, 3)
    # a root that lives one level more wins: 36 >= 30
    got = select(9, [low, low, low, [a + b, c]] + [[a + b + c]] * 4, 2)
    assert got == ([0] * 9, [4] * 9, 1)


def test_a_small_component_is_noise_and_splits_nothing():
    """S = 3: the pair (4, 5) is no cluster, so the set of four CONTINUES through the merge with it (kids = 1) and the pair's rows
    join it at level 1; the pair (6, 7) never meets anything and stays noise"""
    four = (0, 1, 2, 3)
    got = select(8, [[four, (4, 5), (6, 7)], [four + (4, 5), (6, 7)]], 3)
    assert got == ([0, 0, 0, 0, 0, 0, X, X], [0, 0, 0, 0, 1, 1, X, X], 1)
    # at S = 2 the pair is a cluster and the merge starts a parent: 4 + 2 against 6, the tie goes to the parent; (6, 7) is a cluster
    got = select(8, [[four, (4, 5), (6, 7)], [four + (4, 5), (6, 7)]], 2)
    assert got == ([0, 0, 0, 0, 0, 0, 6, 6], [1, 1, 1, 1, 1, 1, 0, 0], 2)


def test_rows_that_are_not_in_do_not_count():
    """a set of three whose third row has core 2: size 2 at levels 0 and 1, below S = 3, so the cluster starts at level 2"""
    got = select(4, [[(0, 1, 2)]] * 4, 3, cores=[0, 0, 2, 0])
    assert got == ([0, 0, 0, X], [2, 2, 2, X], 1)
    got = select(3, [[(0, 1, 2)]] * 2, 1, cores=[0, X, 1])  # a sparse row is in no cluster
    assert got == ([0, X, 0], [0, X, 1], 1)


def test_single_rows_are_clusters_at_size_one():
    """S = 1 with M = 1: every row is a cluster at level 0"""
    assert select(3, [[], [], []], 1) == ([0, 1, 2], [0, 0, 0], 3)
    # rows 0 and 1 merge at the last level: 2 + 2 against 2
    assert select(3, [[], [], [(0, 1)]], 1) == ([0, 1, 2], [0, 0, 0], 3)
    # ... and at the first: one cluster of two from level 0 on
    assert select(3, [[(0, 1)]] * 3, 1) == ([0, 0, 2], [0, 0, 0], 2)


def test_bounds_above_the_sequence_length_lengthen_the_root():
    """two pairs of copies that differ in both of their two columns: the levels from L = 2 on hold one set, so the root's
    stability is 4 x (D - 1) against the pairs' 2 + 2 levels of 2"""
    codes = np.array([[0, 0], [0, 0], [1, 1], [1, 1]], dtype=np.uint8)
    for D, want in ((1, ([0, 0, 2, 2], [0, 0, 0, 0], 2)), (2, ([0, 0, 2, 2], [0, 0, 0, 0], 2)), (3, ([0, 0, 0, 0], [2, 2, 2, 2], 1)),
                    (5, ([0, 0, 0, 0], [2, 2, 2, 2], 1))):
        labels, joined, count, cores = expected_stable(codes, D, 1, 2)
        assert (labels.tolist(), joined.tolist(), count) == want, D
        assert cores.tolist() == [0] * 4
    # min_pts 3: a row's second other row is 2 away; every row is in from level 2 on only, where there is one set
    labels, joined, count, cores = expected_stable(codes, 4, 3, 0)
    assert (labels.tolist(), joined.tolist(), count, cores.tolist()) == ([0] * 4, [2] * 4, 1, [2] * 4)


def test_fewer_rows_than_min_pts_is_all_noise():
    codes = np.array([[0, 0], [0, 0], [1, 1]], dtype=np.uint8)
    for D in (1, 2, 4):
        labels, joined, count, cores = expected_stable(codes, D, 4, 1)
        assert (labels.tolist(), joined.tolist(), count, cores.tolist()) == ([X] * 3, [X] * 3, 0, [X] * 3)


def test_defaults():
    assert sizes(0, 0) == (1, 1) and sizes(4, 0) == (4, 4) and sizes(4, 2) == (4, 2) and sizes(0, 7) == (1, 7)


def test_gpu_fixtures_are_not_trivial():
    """conditions on the INPUTS of tests/test_gpu_stable.py::test_fixture_stores, checked before any GPU run"""
    found, counts = set(), []
    for _, make, D, M, S in FIXTURES:
        codes = make()
        M, S = sizes(M, S)
        cores, labels, _ = expected_reach(codes, D, M)
        found |= traits(cores, labels, S)
        counts.append(expected_stable(codes, D, M, S)[2])
    for needed in ("chosen non-leaf", "chosen leaf under a parent that is not", "noise", "joined later"):
        assert needed in found, (needed, sorted(found))
    assert len([w for w in found if w.startswith("t_hi ")]) >= 2, sorted(found)
    assert max(counts) > 100 and min(counts) >= 1, counts

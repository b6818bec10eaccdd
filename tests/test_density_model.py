"""The model the density tests are held against (tests/density_cases.py), itself held against stores small enough to work
by hand: the expected arrays below are literals."""
import numpy as np

from components_cases import labels_from_pairs
from density_cases import NONE, bridged_store, brute_density, kinds
from self_join_cases import brute_pairs, planted_store

N = NONE


def rows(*strings):
    return np.array([[int(c) for c in s] for s in strings], dtype=np.uint8)


def check(codes, D, min_pts, labels, degrees, counts):
    got = brute_density(codes, D, min_pts)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert got[0].tolist() == labels and got[1].tolist() == degrees and got[2] == counts, got


def test_a_border_row_between_two_clusters_takes_the_smaller_core_number():
    """P = 000000 three times (rows 0, 2, 7), P' = 100000 (row 5), b = 110000 (row 6), Q' = 111000 (row 3), Q = 111100 twice
    (rows 1, 4); bound 1, min_pts 4 (core: 3 neighbours).  Core: the P rows (each other and P'), P' (the P rows and b) and Q'
    (the Q rows and b).  Cluster {0, 2, 5, 7} has label 0, cluster {3} label 3.  b has two neighbours, is not core, and lies
    within 1 of core rows 5 (label 0) and 3 (label 3): the smaller core NUMBER is 3, so b's label is 3, not the smaller
    label 0.  The Q rows have two neighbours each and are border rows of 3."""
    codes = rows("000000", "111100", "000000", "111000", "111100", "100000", "110000", "000000")
    check(codes, 1, 4, [0, 3, 0, 3, 3, 0, 3, 0], [3, 2, 3, 3, 2, 4, 2, 3], {"clusters": 2, "core": 5, "noise": 0})
    # min_pts 5: only P' (4 neighbours) is core; the P rows and b are its border rows, the Q side is noise
    check(codes, 1, 5, [5, N, 5, N, N, 5, 5, 5], [3, 2, 3, 3, 2, 4, 2, 3], {"clusters": 1, "core": 1, "noise": 3})


def test_a_border_row_numbered_below_its_label_and_noise_that_single_linkage_would_group():
    """row 0 = 110000 is within 1 of row 4 = 100000 alone; rows 2, 3 = 000000; row 1 far from everything; rows 5, 6 a pair at
    distance 1 far from the rest.  Bound 1, min_pts 3: core are 2, 3 (each other and 4) and 4; row 0 is a border row whose
    label 2 is LARGER than its own number; rows 5 and 6 have one neighbour each, no core row near: noise, though single
    linkage makes them a component."""
    codes = rows("110000", "333333", "000000", "000000", "100000", "222222", "222223")
    degrees = [1, 0, 2, 2, 3, 1, 1]
    check(codes, 1, 3, [2, N, 2, 2, 2, N, N], degrees, {"clusters": 1, "core": 3, "noise": 3})
    # min_pts 2: the clusters are the components of size >= 2, the singleton is noise
    check(codes, 1, 2, [0, N, 0, 0, 0, 5, 5], degrees, {"clusters": 2, "core": 6, "noise": 1})
    # min_pts 1 and 0: every row is core, the labels are the components
    for min_pts in (1, 0):
        check(codes, 1, min_pts, [0, 1, 0, 0, 0, 5, 5], degrees, {"clusters": 3, "core": 7, "noise": 0})
    check(codes, 1, 8, [N] * 7, degrees, {"clusters": 0, "core": 0, "noise": 7})  # min_pts > n


def test_copies_alone_and_a_bound_no_two_rows_exceed():
    codes = rows("01", "23", "01", "30", "01", "23")
    check(codes, 0, 3, [0, N, 0, N, 0, N], [2, 1, 2, 0, 2, 1], {"clusters": 1, "core": 3, "noise": 3})
    check(codes, 0, 2, [0, 1, 0, N, 0, 1], [2, 1, 2, 0, 2, 1], {"clusters": 2, "core": 5, "noise": 1})
    # bound 2 = the length: every degree is n - 1; all one cluster if n >= min_pts, else all noise
    check(codes, 2, 6, [0] * 6, [5] * 6, {"clusters": 1, "core": 6, "noise": 0})
    check(codes, 2, 7, [N] * 6, [5] * 6, {"clusters": 0, "core": 0, "noise": 6})


def test_min_pts_one_is_the_components():
    for kind, D in (("nt", 5), ("aa", 2)):
        codes = planted_store(3, kind, 60, 40)
        pairs = brute_pairs(codes, D)
        labels, degrees, counts = brute_density(codes, D, 1)
        want = labels_from_pairs(len(codes), pairs)
        assert labels.tobytes() == want.tobytes()
        assert counts == {"clusters": int((want == np.arange(len(codes))).sum()), "core": len(codes), "noise": 0}
        assert int(degrees.sum()) == 2 * len(pairs)


def test_bridged_store_facts():
    for seed in (1, 2, 3):
        codes, role = bridged_store(seed)  # (asserts its facts itself)
        assert len(codes) == 2 * 32 + 11 and sorted(role.tolist()) == sorted([0] * 32 + [1] * 32 + list(range(2, 13)))
        labels, degrees, counts = brute_density(codes, 1, 4)
        core, border, noise = kinds(labels, degrees, 4)
        assert counts["clusters"] == 2 and int(border.sum()) == 2 and int(noise.sum()) == 7
        assert set(np.flatnonzero(border).tolist()) == {int(np.flatnonzero(role == 3)[0]), int(np.flatnonzero(role == 11)[0])}
        # every non-noise label is a core row; a core row's label is a representative
        assert core[labels[~noise]].all() and (labels[labels[core]] == labels[core]).all()

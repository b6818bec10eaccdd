"""The mutual-reachability forest without a GPU: what the expected answers of tests/reach_cases.py mean, and a host model of the
call (smafa_amd/csrc/reach.hip.h), CPU only.

  * The brute-force partitions at every t, restricted to the rows that are core at t, are the core-row labels of the density
    call's brute force at bound t (density_cases.density_from_pairs) — the claim the header makes — and at min_pts 1 they are
    the single-linkage levels (levels_cases.brute_levels).
  * The model: tallies per row and distance from every pair once (tally_keep_kernel), the running sum from 1 (core_dist_kernel),
    and the union of tests/test_forest_model.py — lanes that yield in front of every access to parent[] under a scheduler — over
    rows weighed max(dist, core[a], core[b]) (span_reach_kernel).  Class by class the winners pass reach_cases.check_reach_forest
    whatever the interleaving; all classes in ONE launch can be driven to a forest that is not minimum, so the level counts
    fail.  It checks the argument, not the kernel."""
import random

import numpy as np
import pytest

from density_cases import density_from_pairs
from levels_cases import brute_levels
from neighbours_cases import tie_family
from reach_cases import NONE, brute_cores, check_reach_forest, expected_reach, weighted_pairs
from self_join_cases import brute_pairs, planted_store
from test_forest_model import span, two_cliques, with_mirrors


def small_store(seed):
    return planted_store(300 + seed, "nt", 8, 5, members=8, max_subs=2, copies=6)  # 46 rows in 5 families


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("M", [2, 3, 5])
def test_partitions_on_core_rows_are_the_density_labels(seed, M):
    codes, D = small_store(seed), 4
    n = len(codes)
    cores, labels, counts = expected_reach(codes, D, M)
    assert (cores != NONE).any() and len(set(cores.tolist())) >= 3, cores  # the store has rows of several core distances
    pairs = brute_pairs(codes, D)
    for t in range(D + 1):
        want, degrees, _ = density_from_pairs(n, pairs[pairs["dist"] <= t], M)
        core = cores.astype(np.int64) <= t
        assert (core == (degrees.astype(np.int64) + 1 >= M)).all(), t  # core[i] <= t iff the row is a core row at bound t
        assert labels[t][core].tobytes() == want[core].tobytes(), t
        assert (labels[t][~core] == np.flatnonzero(~core)).all(), t  # rows with core > t are singletons
        assert counts[t] == int((~core).sum()) + len(set(want[core].tolist())), t


@pytest.mark.parametrize("M", [0, 1])
def test_min_pts_one_is_single_linkage(M):
    codes, D = small_store(9), 4
    cores, labels, counts = expected_reach(codes, D, M)
    want, want_counts, _ = brute_levels(codes, D)
    assert not cores.any() and labels.tobytes() == want.tobytes() and counts == want_counts


def test_cores_are_the_kth_neighbour_distance():
    """40 copies and 40 variants at one column each: a copy's 39th other row is at 0 and its 40th at 1 (a tie of 40); a variant's
    40th is at 1 and its 41st at 2; past the 79th there is none"""
    codes, copies = tie_family()
    for M, of_copy, of_variant in ((2, 0, 1), (40, 0, 1), (41, 1, 1), (42, 1, 2), (80, 1, 2), (81, NONE, NONE)):
        cores = brute_cores(codes, 2, M)
        assert (cores[copies] == of_copy).all() and (cores[~copies] == of_variant).all(), (M, cores)
    assert (brute_cores(codes, 1, 42)[~copies] == NONE).all()  # the bound cuts the list


def model(codes, D, M, seed, by_class=True, first=(), mirrors=True):
    """-> (edges, level_ends, cores) of the host model of join_reach_forest"""
    n, L = codes.shape
    E = min(D, L - 1) + 1
    pairs = brute_pairs(codes, E - 1)  # the one join: every pair once, as the exactly-once rule keeps them
    hist = np.zeros((n, E), dtype=np.int64)
    for r in pairs:  # tally_keep_kernel
        hist[int(r["query"]), int(r["dist"])] += 1
        hist[int(r["subject"]), int(r["dist"])] += 1
    cores = np.full(n, NONE, dtype=np.uint32)
    for i in range(n):  # core_dist_kernel
        ball = 1
        for t in range(E):
            ball += hist[i, t]
            if ball >= max(M, 1):
                cores[i] = t
                break
    rows = with_mirrors(pairs, random.Random(seed)) if mirrors else [(int(r["query"]), int(r["subject"]), int(r["dist"])) for r in pairs]
    big = cores.astype(np.int64)
    weighed = [(a, b, max(d, int(big[a]), int(big[b]))) for a, b, d in rows]
    weighed = [r for r in weighed if r[2] <= D]  # (NONE matches no class)
    edges, ends = span(n, weighed, D, seed, by_class=by_class, first=first)
    return edges, ends, cores


@pytest.mark.parametrize("seed", range(8))
def test_class_by_class_is_a_minimum_forest(seed):
    codes, D, M = small_store(seed), 4, 2 + seed % 3
    edges, ends, cores = model(codes, D, M, seed)
    counts = check_reach_forest(codes, edges, ends, cores, D, M)
    assert len(set(counts)) >= 3, counts  # the levels differ


def test_all_classes_in_one_launch_fails_the_level_counts():
    """two cliques of six equal rows at distance 3, min_pts 4: every row has five copies, so every core is 0 and a pair weighs its
    distance.  The heavy rows (0, 1) and (2, 3) run first and win; the light row (0, 2) then joins the two pairs, and one light
    row fewer can win: level_ends[0] comes out too small."""
    codes, pairs = two_cliques()
    n, M = len(codes), 4
    assert not brute_cores(codes, 3, M).any()
    edges, ends, cores = model(codes, 3, M, 0, by_class=False, first=[(0, 1, 3), (2, 3, 3)], mirrors=False)
    assert int(ends[3]) == n - 1 and int(ends[0]) < n - 2  # it spans, but it is not minimum
    with pytest.raises(AssertionError):
        check_reach_forest(codes, edges, ends, cores, 3, M)
    edges, ends, cores = model(codes, 3, M, 0, by_class=True, mirrors=False)
    assert ends.tolist() == [n - 2, n - 2, n - 2, n - 1]
    check_reach_forest(codes, edges, ends, cores, 3, M)


def test_a_core_lifts_a_light_pair_into_a_heavy_class():
    """the weight is not the distance: a row with one copy and min_pts 3 has its copy at 0 but its core at the next row's
    distance, so the pair of copies joins at that level and not at 0"""
    a = np.zeros(8, dtype=np.uint8)
    b = a.copy()
    b[[0, 1]] = 1  # two columns from a
    codes = np.array([a, a, b, b, b], dtype=np.uint8)
    cores, pairs, w = weighted_pairs(codes, 3, 3)
    assert cores.tolist() == [2, 2, 0, 0, 0]
    assert sorted(zip(pairs["query"].tolist(), pairs["subject"].tolist(), w.tolist()))[0] == (0, 1, 2)
    edges, ends, got = model(codes, 3, 3, 1)
    assert ends.tolist() == [2, 2, 4, 4]
    check_reach_forest(codes, edges, ends, got, 3, 3)

"""Expected labels of the levels tests (tests/test_gpu_levels.py, tests/levels_worker.py).

Nothing here comes from the code under test: the edges are self_join_cases.brute_pairs at the largest bound — brute force
on the code bytes, every pair with its distance — and level t is components_cases.labels_from_pairs over the edges with
dist <= t, a plain union-find."""
import numpy as np

from components_cases import labels_from_pairs
from self_join_cases import brute_pairs


def brute_levels(codes, D):
    """-> (labels, counts, pairs) of a store at the bounds 0 .. D: labels uint32 (D + 1, n), level-major; counts[t] = the
    representatives of level t; pairs = the brute-force pairs within min(D, L) (a pair cannot be farther apart than L)"""
    n, L = codes.shape
    pairs = brute_pairs(codes, min(D, L))
    labels = np.zeros((D + 1, n), dtype=np.uint32)
    for t in range(D + 1):
        labels[t] = labels_from_pairs(n, pairs[pairs["dist"] <= t])
    counts = [int((labels[t] == np.arange(n)).sum()) for t in range(D + 1)]
    return labels, counts, pairs


def check_nesting(labels, counts):
    """the rows of a levels answer nest (include/smafa_amd.h): asserted on any answer, expected or computed"""
    n = labels.shape[1]
    idx = np.arange(n)
    for t in range(labels.shape[0]):
        row = labels[t]
        assert (row <= idx).all() and (row[row] == row).all(), t
        assert counts[t] == int((row == idx).sum()), t
        if t:
            assert (row <= labels[t - 1]).all() and (row[labels[t - 1]] == row).all(), t
            assert counts[t] <= counts[t - 1], t

"""The model of tests/peaks_weighted_cases.py on hand-worked stores, and the lifted-peaks identity in the model alone: the peaks of
a raw store are the peaks of its distinct rows under weights_in = sizes, lifted through old_of_new and unique_of."""
import numpy as np
import pytest

from peaks_cases import brute_peaks, valley_store
from peaks_weighted_cases import brute_weighted_peaks, expected_derep, identity_store, lifted, random_weights


def rows(*texts):
    return np.array([[ord(c) - ord("a") for c in t] for t in texts], dtype=np.uint8)


def test_hand_worked_dereplication():
    unique_of, old_of_new, sizes = expected_derep(rows("abc", "abd", "abc", "bbc", "abd", "abc"))
    assert unique_of.tolist() == [0, 1, 0, 2, 1, 0] and old_of_new.tolist() == [0, 1, 3] and sizes.tolist() == [3, 2, 1]
    # the numbering follows the first occurrences, not the order of the sequences
    unique_of, old_of_new, sizes = expected_derep(rows("zz", "aa", "zz", "mm", "aa"))
    assert unique_of.tolist() == [0, 1, 0, 2, 1] and old_of_new.tolist() == [0, 1, 3] and sizes.tolist() == [2, 2, 1]
    unique_of, old_of_new, sizes = expected_derep(rows("ab", "ab", "cd", "ab", "ef"), [5, 0, 7, 2, 0])
    assert unique_of.tolist() == [0, 0, 1, 0, 2] and old_of_new.tolist() == [0, 2, 4] and sizes.tolist() == [7, 7, 0]
    assert [len(a) for a in expected_derep(np.zeros((0, 60), dtype=np.uint8))] == [0, 0, 0]


def test_hand_worked_weighted_peaks():
    """four rows in a chain a - b - c - d, one substitution apart each (a and c, b and d two apart), D = 1"""
    codes = rows("aaaa", "baaa", "bbaa", "bbba")
    # r = 0: the weights are the given ones; every row climbs to its heaviest neighbour, ties to the smaller number
    labels, parents, weights, n_peaks = brute_weighted_peaks(codes, 1, 0, [1, 5, 5, 2])
    assert weights.tolist() == [1, 5, 5, 2] and parents.tolist() == [1, 1, 1, 2] and labels.tolist() == [1, 1, 1, 1] and n_peaks == 1
    # r = 1: a row's weight is its own plus its neighbours' — not its neighbours' count
    labels, parents, weights, n_peaks = brute_weighted_peaks(codes, 1, 1, [1, 5, 5, 2])
    assert weights.tolist() == [6, 11, 12, 7] and parents.tolist() == [1, 2, 2, 2] and labels.tolist() == [2, 2, 2, 2] and n_peaks == 1
    # a weight of 0 is the lightest, and still a row
    labels, parents, weights, n_peaks = brute_weighted_peaks(codes, 1, 0, [0, 0, 3, 0])
    assert weights.tolist() == [0, 0, 3, 0] and parents.tolist() == [0, 2, 2, 2] and n_peaks == 2


@pytest.mark.parametrize("radius", (0, None))
@pytest.mark.parametrize("kind", ("nt", "aa"))
def test_the_identity_in_the_model(kind, radius):
    codes, D = identity_store(kind), 3
    derep = expected_derep(codes)
    raw = brute_peaks(codes, D, radius)
    uniques = brute_weighted_peaks(codes[derep[1]], D, radius, derep[2])
    assert not lifted(raw, derep, uniques)
    assert 10 < raw[3] < len(derep[1]) < len(codes)  # something climbed, something was copied
    # and it is the SIZES that make it hold: with every weight 1 the distinct rows have other peaks
    ones = brute_weighted_peaks(codes[derep[1]], D, radius, np.ones(len(derep[1]), dtype=np.uint32))
    assert lifted(raw, derep, ones)


def test_weighted_peaks_with_ones_are_the_peaks():
    codes, _ = valley_store(3)
    for radius in (0, 1):
        want = brute_peaks(codes, 1, radius)
        got = brute_weighted_peaks(codes, 1, radius, np.ones(len(codes), dtype=np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
    w = random_weights(len(codes), 1)
    labels, parents, weights, n_peaks = brute_weighted_peaks(codes, 1, 0, w)
    assert (w == 0).any() and n_peaks >= 1 and (labels[labels] == labels).all()

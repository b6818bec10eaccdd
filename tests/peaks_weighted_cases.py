"""The numpy model of the peaks with given weights (tests/test_peaks_weighted_model.py, tests/test_gpu_peaks_weighted.py,
tests/peaks_weighted_worker.py).

The weighted peaks are tests/peaks_cases.py's with one line changed — the weights a weighted bincount.  Where the weights come
from in practice is a dereplication, done here on the host: np.unique over the rows gives every row its sequence, the first
occurrence of every sequence orders them, np.add.at sums the sizes; the lifted identity says what the peaks of a raw store and the
weighted peaks of its distinct rows owe each other.  Nothing here comes from the code under test."""
import functools

import numpy as np

from peaks_cases import NONE, flatten, keys_of
from self_join_cases import brute_pairs


# ---- the model
def expected_derep(codes, weights=None):
    """-> (unique_of[n], old_of_new[U], sizes[U]) uint32: the uniques numbered by their first occurrence"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n = len(codes)
    if n == 0:
        return (np.zeros(0, dtype=np.uint32),) * 3
    _, first, inverse = np.unique(codes, axis=0, return_index=True, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))  # sorted-unique number -> first-occurrence number
    unique_of = rank[inverse]
    old_of_new = np.sort(first)
    w = np.ones(n, dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    sizes = np.zeros(len(first), dtype=np.int64)
    np.add.at(sizes, unique_of, w)
    # what the contract says, literally
    assert (codes[old_of_new[unique_of]] == codes).all() and (old_of_new[unique_of] <= np.arange(n)).all()
    assert (unique_of[old_of_new] == np.arange(len(first))).all() and sizes.sum() == w.sum()
    return unique_of.astype(np.uint32), old_of_new.astype(np.uint32), sizes.astype(np.uint32)


def weighted_peaks_from_pairs(n, pairs, radius, w_in):
    """peaks_cases.peaks_from_pairs with weight[i] = w_in[i] + the sum of w_in[j] over the other rows within the radius"""
    q, s, d = pairs["query"].astype(np.int64), pairs["subject"].astype(np.int64), pairs["dist"].astype(np.int64)
    w_in = np.asarray(w_in, dtype=np.int64)
    near = d <= int(radius)
    weights = w_in + np.bincount(q[near], weights=w_in[s[near]], minlength=n).astype(np.int64) + \
        np.bincount(s[near], weights=w_in[q[near]], minlength=n).astype(np.int64)
    assert weights.max(initial=0) <= NONE
    keys = keys_of(weights)
    best = keys.copy()
    np.maximum.at(best, q, keys[s])
    np.maximum.at(best, s, keys[q])
    parents = (np.uint64(NONE) - (best & np.uint64(NONE))).astype(np.uint32)
    labels, _ = flatten(parents)
    return labels, parents, weights.astype(np.uint32), int((parents == np.arange(n)).sum())


def brute_weighted_peaks(codes, D, radius, w_in):
    radius = D if radius is None else radius
    return weighted_peaks_from_pairs(len(codes), brute_pairs(codes, D), radius, w_in)


def lifted(raw, derep, uniques):
    """the identity: raw = (labels, parents, weights, n_peaks) of the raw store, uniques = the same of its dereplication under
    weights_in = sizes, derep = (unique_of, old_of_new, sizes) -> the list of what does not hold (empty: it holds)"""
    unique_of, old_of_new, _ = derep
    bad = []
    if raw[0].tobytes() != old_of_new[uniques[0][unique_of]].tobytes():
        bad.append("labels")
    if raw[2].tobytes() != uniques[2][unique_of].tobytes():
        bad.append("weights")
    if raw[3] != uniques[3]:
        bad.append("n_peaks")
    return bad


@functools.lru_cache(maxsize=None)
def identity_store(kind, seed=0):
    """about 60 seeds x 1 .. 30 copies, plus variants 1 .. 3 substitutions away with few copies each: about 3 000 raw rows"""
    rng = np.random.default_rng(60 + seed + (1 if kind == "aa" else 0))
    lc = np.arange(28 if kind == "aa" else 4, dtype=np.uint8)
    L = 60
    rows = []
    for _ in range(60):
        seed_row = lc[rng.integers(0, len(lc), size=L)]
        rows += [seed_row] * int(rng.integers(1, 31))
        for _ in range(int(rng.integers(8, 16))):
            v = seed_row.copy()
            cols = rng.choice(L, size=int(rng.integers(1, 4)), replace=False)
            v[cols] = (v[cols] + rng.integers(1, len(lc), size=len(cols))) % len(lc)
            rows += [v] * int(rng.integers(1, 5))
    codes = np.ascontiguousarray(np.array(rows, dtype=np.uint8)[rng.permutation(len(rows))])
    assert 2000 <= len(codes) <= 4000, len(codes)
    codes.setflags(write=False)
    return codes


def random_weights(n, seed=0, top=1000):
    """uint32 weights with zeros among them"""
    rng = np.random.default_rng(n + seed)
    w = rng.integers(0, top, size=n).astype(np.uint32)
    w[rng.random(n) < 0.2] = 0
    return w

"""Expected answers of the peaks tests (tests/test_peaks_model.py, tests/test_gpu_peaks.py, tests/peaks_worker.py).

Nothing here comes from the code under test: the pairs are self_join_cases.brute_pairs — brute force on the code bytes —
the weights a bincount over both columns of the pairs within the radius, best[] an np.maximum.at on 64-bit keys
(weight << 32 | 0xFFFFFFFF - number: the heavier row wins, ties go to the smaller number), and the labels repeated lab[lab].

Two stores assert their own facts on the brute-force answer, so that a change of generator cannot hollow the tests out."""
import numpy as np

from components_cases import labels_from_pairs
from density_cases import density_from_pairs
from self_join_cases import brute_pairs

NONE = 0xFFFFFFFF


def keys_of(weights):
    """uint64 keys: (weight, -number) in lexicographic order as one integer"""
    n = len(weights)
    return (weights.astype(np.uint64) << np.uint64(32)) | (np.uint64(NONE) - np.arange(n, dtype=np.uint64))


def flatten(parents):
    """-> (labels, rounds): lab = lab[lab] until nothing changes; rounds = the doublings that changed something"""
    lab = parents.astype(np.int64)
    rounds = 0
    while True:
        nxt = lab[lab]
        if (nxt == lab).all():
            return lab.astype(np.uint32), rounds
        lab = nxt
        rounds += 1


def peaks_from_pairs(n, pairs, radius):
    """pairs (HIT_DTYPE, each unordered pair once, all within the bound) -> (labels, parents, weights uint32[n], n_peaks)"""
    q, s, d = pairs["query"].astype(np.int64), pairs["subject"].astype(np.int64), pairs["dist"].astype(np.int64)
    near = d <= int(radius)
    weights = 1 + np.bincount(q[near], minlength=n) + np.bincount(s[near], minlength=n)
    keys = keys_of(weights)
    best = keys.copy()
    np.maximum.at(best, q, keys[s])
    np.maximum.at(best, s, keys[q])
    parents = (np.uint64(NONE) - (best & np.uint64(NONE))).astype(np.uint32)
    labels, _ = flatten(parents)
    return labels, parents, weights.astype(np.uint32), int((parents == np.arange(n)).sum())


def brute_peaks(codes, D, radius):
    """-> (labels, parents, weights, n_peaks) of a store at bound D and radius r <= D (None: r = D)"""
    radius = D if radius is None else radius
    assert radius <= D
    return peaks_from_pairs(len(codes), brute_pairs(codes, D), radius)


def moved_and_multi_step(answer):
    """-> (rows that are no peak, rows more than one step from their peak)"""
    labels, parents = answer[0], answer[1]
    idx = np.arange(len(labels))
    return int((parents != idx).sum()), int((labels != parents).sum())


VALLEY = (40, 12, 6, 3, 6, 12, 30)


def valley_store(seed, L=60):
    """Seven groups of exact copies with abundances 40, 12, 6, 3, 6, 12, 30; consecutive groups are one substitution apart,
    in distinct columns; shuffled.  -> (codes, group of every row).

    At D = 1 the store is ONE single-linkage component and ONE density cluster at min_pts 1, 2, 3, 4 and 7 (the thinnest
    group has 3 + 6 + 6 = 15 rows within the bound: every row is core).  The peaks call gives exactly two clusters, split at
    the valley's bottom:
      r = 0  the weights are the abundances; the peaks are the smallest-numbered copies of the 40- and the 30-copy group;
             the 3-copy group at the bottom has a 6-copy group on either side, and the tie goes to the side that holds
             the smallest subject number: cluster sizes {61, 48} or {58, 51}.
      r = 1  the weights are the ball counts 52, 58, 21, 15, 21, 48, 42: the 12-copy group next to each abundant end
             sees more rows than that end does (40 + 12 + 6 against 40 + 12, 6 + 12 + 30 against 12 + 30), so the two peaks
             are the smallest-numbered copies of the two 12-copy groups; the bottom's tie (21 = 21) falls as at r = 0, and the
             sizes are the same two.
    These facts are asserted here on the brute-force answer."""
    rng = np.random.default_rng(seed)
    row = rng.integers(0, 4, size=L).astype(np.uint8)
    cols = rng.choice(L, size=len(VALLEY) - 1, replace=False)
    rows, group = [], []
    for g, copies in enumerate(VALLEY):
        if g:
            row = row.copy()
            row[cols[g - 1]] = (row[cols[g - 1]] + 1 + rng.integers(0, 3)) % 4
        rows += [row] * copies
        group += [g] * copies
    perm = rng.permutation(len(rows))
    codes = np.ascontiguousarray(np.array(rows, dtype=np.uint8)[perm])
    group = np.array(group)[perm]
    # the facts, from brute force
    n = len(codes)
    assert n == 109
    pairs = brute_pairs(codes, 1)
    assert len(set(labels_from_pairs(n, pairs).tolist())) == 1
    for min_pts in (1, 2, 3, 4, 7):
        labels, _, counts = density_from_pairs(n, pairs, min_pts)
        assert counts == {"clusters": 1, "core": n, "noise": 0} and len(set(labels.tolist())) == 1
    first = [int(np.flatnonzero(group == g)[0]) for g in range(len(VALLEY))]
    labels, parents, weights, n_peaks = peaks_from_pairs(n, pairs, 0)
    assert weights.tolist() == [VALLEY[g] for g in group]
    assert n_peaks == 2 and sorted(set(labels.tolist())) == sorted([first[0], first[6]])
    sizes = sorted(np.bincount(labels, minlength=n)[[first[0], first[6]]].tolist())
    assert sizes in ([48, 61], [51, 58]), sizes
    bottom = first[2] if first[2] < first[4] else first[4]
    assert (parents[group == 3] == bottom).all()
    labels, parents, weights, n_peaks = peaks_from_pairs(n, pairs, 1)
    assert weights.tolist() == [(52, 58, 21, 15, 21, 48, 42)[g] for g in group]
    assert n_peaks == 2 and sorted(set(labels.tolist())) == sorted([first[1], first[5]])
    assert sorted(np.bincount(labels, minlength=n)[[first[1], first[5]]].tolist()) == sizes
    assert (parents[group == 3] == bottom).all()
    return codes, group


def climb_chain(L=300):
    """3L - 1 rows, numbered along the walk: row k is row k - 1 with column (k - 1) mod L advanced by one letter (mod 4).
    A column is advanced at most three times, so it never returns to a letter it had: rows k and k + m differ in min(m, L)
    columns — consecutive rows are at distance 1, every other pair at >= 2.  At D = 1, r = 0 every weight is 1, the ties go
    to the smaller number, parent[k] == k - 1, row 0 is the one peak, and flattening the chain takes 10 doublings (asserted
    here on the brute-force answer)."""
    rng = np.random.default_rng(L)
    row = rng.integers(0, 4, size=L).astype(np.uint8)
    rows = [row.copy()]
    for k in range(1, 3 * L - 1):
        row[(k - 1) % L] = (row[(k - 1) % L] + 1) % 4
        rows.append(row.copy())
    codes = np.ascontiguousarray(np.array(rows, dtype=np.uint8))
    n = len(codes)
    pairs = brute_pairs(codes, 1)
    assert len(pairs) == n - 1 and (pairs["subject"] == pairs["query"] + 1).all() and (pairs["dist"] == 1).all()
    labels, parents, weights, n_peaks = peaks_from_pairs(n, pairs, 0)
    assert (weights == 1).all() and parents.tolist() == [0] + list(range(n - 1)) and n_peaks == 1 and not labels.any()
    if L == 300:
        assert n == 899 and flatten(parents)[1] == 10
    return codes

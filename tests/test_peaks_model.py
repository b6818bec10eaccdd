"""The model the peaks tests are held against (tests/peaks_cases.py), itself held against stores small enough to work by
hand — the expected arrays below are literals — and against the facts its two stores assert.  The last test is a host model
of jump_kernel's in-place pointer doubling under a random visiting order, held against the plain walk: it checks the
argument (any value a racing thread reads is an ancestor), not the kernel."""
import numpy as np

from density_cases import bridged_store
from peaks_cases import VALLEY, brute_peaks, climb_chain, flatten, keys_of, moved_and_multi_step, valley_store
from self_join_cases import planted_store


def rows(*strings):
    return np.array([[int(c) for c in s] for s in strings], dtype=np.uint8)


def check(codes, D, r, labels, parents, weights, n_peaks):
    got = brute_peaks(codes, D, r)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3]) == (labels, parents, weights, n_peaks), got


def test_copies_climb_to_their_smallest_number_and_a_label_may_exceed_its_row():
    """row 0 = 100000 once, rows 1, 3, 4 = 000000, row 2 = 110000 once, row 5 far away.  D = 1, r = 0: the weights are the
    abundances 1, 3, 1, 3, 3, 1.  Row 0 is within 1 of the copies: its parent is the smallest copy, row 1 — a label LARGER than
    the row.  The copies see each other and row 0: parent 1.  Row 2 sees only row 0 (weight 1, smaller number): parent 0, two
    steps from its peak.  Row 5 is a peak of weight 1."""
    codes = rows("100000", "000000", "110000", "000000", "000000", "333333")
    check(codes, 1, 0, [1, 1, 1, 1, 1, 5], [1, 1, 0, 1, 1, 5], [1, 3, 1, 3, 3, 1], 2)
    # r = D = 1: ball counts — row 0 sees the three copies and row 2 (5), the copies see each other and row 0 (4), row 2 sees
    # row 0 (2): row 0 is now the peak of everything near it
    check(codes, 1, 1, [0, 0, 0, 0, 0, 5], [0, 0, 0, 0, 0, 5], [5, 4, 2, 4, 4, 1], 2)
    check(codes, 1, None, [0, 0, 0, 0, 0, 5], [0, 0, 0, 0, 0, 5], [5, 4, 2, 4, 4, 1], 2)
    # D = 0: only copies are neighbours
    check(codes, 0, 0, [0, 1, 2, 1, 1, 5], [0, 1, 2, 1, 1, 5], [1, 3, 1, 3, 3, 1], 4)


def test_ties_go_to_the_smaller_number_and_chain():
    """four single rows in a walk, numbered 2, 0, 3, 1 along it: all weights 1 at r = 0, every row's parent is the smallest
    number among itself and its neighbours"""
    codes = rows("100000", "111000", "000000", "110000")  # walk: 2 - 0 - 3 - 1
    check(codes, 1, 0, [0, 1, 0, 0], [0, 1, 0, 0], [1, 1, 1, 1], 2)
    # at r = 1 the inner rows of the walk weigh 3, the ends 2: 0 and 3 tie, 0 wins; 1 climbs to 3 and on to 0
    check(codes, 1, 1, [0, 0, 0, 0], [0, 3, 0, 0], [3, 2, 2, 3], 1)


def test_a_bound_no_two_rows_exceed():
    codes = rows("01", "23", "01", "30", "23", "23")
    # D = 2 = the length: every row is every row's neighbour; r = 0: abundances 2, 3, 2, 1, 3, 3: the peak is row 1
    check(codes, 2, 0, [1] * 6, [1] * 6, [2, 3, 2, 1, 3, 3], 1)
    check(codes, 2, 2, [0] * 6, [0] * 6, [6] * 6, 1)  # r = 2 too: every weight is n, the peak row 0
    check(codes, 5, 5, [0] * 6, [0] * 6, [6] * 6, 1)


def test_properties_on_planted_stores():
    for kind, D in (("nt", 5), ("aa", 2)):
        codes = planted_store(3, kind, 60, 40)
        n = len(codes)
        for r in (0, D):
            labels, parents, weights, n_peaks = brute_peaks(codes, D, r)
            idx = np.arange(n)
            keys = keys_of(weights)
            moved = parents != idx
            assert (keys[parents[moved]] > keys[moved]).all() and n_peaks == int((~moved).sum())
            assert (labels[labels] == labels).all() and (parents[labels] == labels).all()
            assert ((codes != codes[parents]).sum(axis=1) <= D).all()
            assert moved_and_multi_step((labels, parents))[0] > 0


def test_valley_store_facts():
    for seed in range(5):
        codes, group = valley_store(seed)  # (asserts its facts itself)
        assert np.bincount(group).tolist() == list(VALLEY)
        for r in (0, 1):
            labels, parents, weights, n_peaks = brute_peaks(codes, 1, r)
            assert n_peaks == 2 and len(set(labels.tolist())) == 2
            # the split is at the valley's bottom: groups 0..2 on one side, 4..6 on the other
            assert len(set(labels[group <= 2].tolist())) == 1 and len(set(labels[group >= 4].tolist())) == 1
            assert labels[group == 0][0] != labels[group == 6][0]


def test_climb_chain_facts():
    codes = climb_chain()  # (asserts its facts itself)
    assert codes.shape == (899, 300)
    labels, parents, weights, n_peaks = brute_peaks(codes, 1, 0)
    flat, rounds = flatten(parents)
    assert flat.tolist() == labels.tolist() and rounds == 10
    assert climb_chain(7).shape == (20, 7)


def test_bridged_store_has_five_peaks():
    codes, role = bridged_store(5)
    labels, parents, weights, n_peaks = brute_peaks(codes, 1, 0)
    assert n_peaks == 5
    first = [int(np.flatnonzero(role == f)[0]) for f in (0, 1)]
    assert (labels[role == 0] == first[0]).all() and (labels[role == 1] == first[1]).all() and first[0] != first[1]
    peaks = np.flatnonzero(parents == np.arange(len(codes)))
    assert all(role[p] >= 2 for p in peaks if weights[p] == 1) and sorted(weights[peaks].tolist()) == [1, 1, 1, 32, 32]


def jump_in_place(parents, rng):
    """jump_kernel on the host, at its least orderly: per round the slots are visited one by one in a random order, each
    reading whatever the slots hold at that moment (old or new), until a round changes nothing -> (labels, rounds)"""
    lab = parents.astype(np.int64).copy()
    rounds = 0
    while True:
        rounds += 1
        changed = False
        for i in rng.permutation(len(lab)):
            u = lab[i]
            uu = lab[u]
            if uu != u:
                lab[i] = uu
                changed = True
        if not changed:
            return lab, rounds


def test_in_place_jumping_equals_the_plain_walk():
    rng = np.random.default_rng(12)
    forests = [np.array([0] + list(range(898)), dtype=np.uint32)]  # the chain
    for n in (1, 2, 50, 700):  # random forests: parent[i] = a row of greater "key" (here: a smaller number), or i
        p = np.array([i if i == 0 or rng.random() < 0.1 else int(rng.integers(0, i)) for i in range(n)], dtype=np.uint32)
        perm = rng.permutation(n)  # renumbered, so that parents are not simply smaller
        q = np.empty(n, dtype=np.uint32)
        q[perm] = perm[p]
        forests.append(q)
    for parents in forests:
        walk = np.empty(len(parents), dtype=np.int64)
        for i in range(len(parents)):
            x = i
            while parents[x] != x:
                x = int(parents[x])
            walk[i] = x
        for _ in range(3):
            lab, rounds = jump_in_place(parents, rng)
            assert lab.tolist() == walk.tolist()
            # never slower than plain doubling, and one more round to see that nothing changes
            assert rounds <= flatten(parents)[1] + 1 <= 33
        assert flatten(parents)[0].tolist() == walk.tolist()

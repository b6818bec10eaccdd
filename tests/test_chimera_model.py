"""The chimera check's model (CPU): tests/chimera_cases.py::brute_chimeras held to hand-worked values on a store of eight rows,
and every planted store that tests/test_gpu_chimeras.py, tests/test_chimera_abi.py and tests/chimera_worker.py use held to its
classes — at least one row of each with the intended verdict.  This is a condition on the INPUTS: a store that misses a class
gets another seed here, never a weaker test there."""
import numpy as np
import pytest

from chimera_cases import (BIMERA, FAR, HAND, LOW_FOLD, NEAR_MISS, NONE, STORES, TIE, brute_chimeras, check_classes, chimera_store,
                           planted, rebuilt)


def test_hand_worked_store():
    # D = 3, r = 0, F = 2: weights 3 3 3 2 2 1 1 1.  Row 5 is 3 from A (columns 3 4 5) and 3 from B (columns 0 1 2): from A
    # pre 3, suf 0; from B pre 0, suf 3.  left = (3, row 0), right = (3, row 3): 3 + 3 >= 6, flagged.  Row 6 is 4 from A (out of
    # reach) and 3 from B: pre 0, suf 3 from row 3 alone, not flagged.  B (weight 2) is 6 from A.  Row 7 is 6 from all.
    a = brute_chimeras(HAND, 3, 0, 2)
    assert a.weights.tolist() == [3, 3, 3, 2, 2, 1, 1, 1]
    assert a.flags.tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and a.n_chimeras == 1
    assert a.left_parent.tolist() == [NONE] * 5 + [0, 3, NONE] and a.left_len.tolist() == [0, 0, 0, 0, 0, 3, 0, 0]
    assert a.right_parent.tolist() == [NONE] * 5 + [3, 3, NONE] and a.right_len.tolist() == [0, 0, 0, 0, 0, 3, 3, 0]
    assert (rebuilt(HAND, a, 5, 3) == HAND[5]).all()
    # D = 4: row 6 reaches A too (columns 2 3 4 5): pre 2 from row 0, suf 3 from row 3: 5 = L - 1, a near miss
    a = brute_chimeras(HAND, 4, 0, 2)
    assert a.flags.tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert (a.left_parent[6], a.left_len[6], a.right_parent[6], a.right_len[6]) == (0, 2, 3, 3)
    # F = 3: B (2) is not three times as heavy as row 5 (1); A (3 >= 3) is: one parent on both sides, no flag
    a = brute_chimeras(HAND, 3, 0, 3)
    assert a.flags.tolist() == [0] * 8 and (a.left_parent[5], a.left_len[5], a.right_parent[5], a.right_len[5]) == (0, 3, 0, 0)
    assert a.left_parent[6] == NONE and a.right_parent[6] == NONE
    # D = 6 = L: every other row is a candidate parent.  B (2) now has A (3) at distance 6 as a parent of last resort at F = 1:
    # pre = suf = 0, the smaller number, row 0.  Row 7 (1): A and B both at length 0, row 0 on both sides.  At F = 2 B has none.
    a = brute_chimeras(HAND, 6, 0, 1)
    assert (a.left_parent[3], a.left_len[3], a.right_parent[3], a.right_len[3]) == (0, 0, 0, 0) and not a.flags[3]
    assert (a.left_parent[7], a.left_len[7], a.right_parent[7], a.right_len[7]) == (0, 0, 0, 0) and not a.flags[7]
    assert a.flags.tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert brute_chimeras(HAND, 6, 0, 2).left_parent[3] == NONE and brute_chimeras(HAND, 9, 0, 1).left_parent.tolist() == a.left_parent.tolist()
    # r = 3 = D: ball counts.  A: 3 + row 5 = 4; B: 2 + rows 5, 6 = 4; row 5: 1 + 3 + 2 + row 6 = 7; row 6: 1 + 2 + row 5 = 4; row
    # 7: 1.  Row 5 is the heaviest row now, and 7 < 2 x 4: at F = 2 nobody has a parent.  At F = 1 row 5 is the one parent of
    # every row within 3 of it: from A's rows pre 3, suf 0; from B's pre 0, suf 3; from row 6 (column 2) pre 2, suf 3
    a = brute_chimeras(HAND, 3, None, 2)
    assert a.weights.tolist() == [4, 4, 4, 4, 4, 7, 4, 1] and (a.left_parent == NONE).all() and a.n_chimeras == 0
    a = brute_chimeras(HAND, 3, None, 1)
    assert a.flags.tolist() == [0] * 8 and (a.left_parent[6], a.left_len[6], a.right_parent[6], a.right_len[6]) == (5, 2, 5, 3)
    assert (a.left_parent[0], a.left_len[0], a.right_parent[0], a.right_len[0]) == (5, 3, 5, 0)
    assert (a.left_parent[3], a.left_len[3], a.right_parent[3], a.right_len[3]) == (5, 0, 5, 3) and a.left_parent[7] == NONE
    # r >= L with counted weights: every weight is n, nobody has a parent
    a = brute_chimeras(HAND, 6, 6, 1)
    assert a.weights.tolist() == [8] * 8 and a.n_chimeras == 0 and (a.left_parent == NONE).all() and not a.left_len.any()


def test_weights_in():
    counted = brute_chimeras(HAND, 3, 0, 2)
    same = brute_chimeras(HAND, 3, 0, 2, counted.weights)
    assert all(np.array_equal(x, y) for x, y in zip(same, counted))
    # A's rows 0 and 1 out (weight 0): row 2 is the left parent; B out altogether: no right parent but row 2 itself (suf 0)
    a = brute_chimeras(HAND, 3, 0, 2, np.array([0, 0, 3, 2, 2, 1, 1, 1], dtype=np.uint32))
    assert (a.left_parent[5], a.right_parent[5]) == (2, 3) and a.flags[5]
    a = brute_chimeras(HAND, 3, 0, 2, np.array([0, 0, 3, 0, 0, 1, 1, 1], dtype=np.uint32))
    assert (a.left_parent[5], a.left_len[5], a.right_parent[5], a.right_len[5]) == (2, 3, 2, 0) and not a.flags[5]
    assert a.left_parent[6] == NONE and a.weights.tolist() == [0, 0, 3, 0, 0, 1, 1, 1]
    # a candidate of weight 0 takes no part either
    a = brute_chimeras(HAND, 3, 0, 2, np.array([3, 3, 3, 2, 2, 0, 1, 1], dtype=np.uint32))
    assert a.left_parent[5] == NONE and not a.flags.any()
    # copies with unequal weights are never each other's parents
    a = brute_chimeras(HAND, 3, 0, 1, np.array([9, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint32))
    assert a.left_parent[1] == NONE and a.left_parent[2] == NONE and a.left_parent[5] == 0
    # the fold in 64 bits: 2^31 x 2 does not wrap
    a = brute_chimeras(HAND, 3, 0, 2, np.array([0xFFFFFFFF, 0, 0, 0, 0, 0x80000000, 0, 0], dtype=np.uint32))
    assert a.left_parent[5] == NONE
    a = brute_chimeras(HAND, 3, 0, 1, np.array([0xFFFFFFFF, 0, 0, 0, 0, 0x80000000, 0, 0], dtype=np.uint32))
    assert a.left_parent[5] == 0


def test_empty_and_one_row():
    a = brute_chimeras(np.zeros((0, 6), dtype=np.uint8), 3, 0, 2)
    assert a.n_chimeras == 0 and a.flags.shape == (0,)
    a = brute_chimeras(HAND[:1], 3, 0, 2)
    assert a.flags.tolist() == [0] and a.left_parent.tolist() == [NONE] and a.weights.tolist() == [1]


@pytest.mark.parametrize("key", sorted(STORES))
def test_every_planted_store_holds_its_classes(key):
    codes, role, info = planted(key)
    kind, L, _ = STORES[key][1:]
    at, wide = check_classes(codes, role, info, L)
    counts = {name: int((role == r).sum()) for r, name in ((BIMERA, "bimera"), (TIE, "tie"), (NEAR_MISS, "near"), (LOW_FOLD, "low"), (FAR, "far"))}
    print("%s: %d rows, %s; flagged at D = 3: F1 %d, F2 %d, F3 %d; at D = 6, F2: %d" % (
        key, len(codes), counts, at[1].n_chimeras, at[2].n_chimeras, at[3].n_chimeras, wide.n_chimeras))
    assert codes.shape[1] == L and ((codes == 4).any() == (kind == "ntn") or kind == "aa")


def test_the_generator_is_deterministic():
    a, b = chimera_store(3, "nt", 60), chimera_store(3, "nt", 60)
    assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all()

"""The consensus model (tests/consensus_cases.py: expected_consensus) against hand-worked values, and what the GPU tests'
fixtures contain (CPU).  The GPU tests hold smafa_db_consensus to this model byte for byte, so the model is held to the
definition of include/smafa_amd.h here."""
import numpy as np
import pytest

from consensus_cases import NONE, chunk_case, edge_codes, edge_labels, expected_consensus, random_grouping, tied_columns
from self_join_cases import SHAPE_STORES, SHAPE_TABLE, shape_case

A, C_, G, T, N = 0, 1, 2, 3, 4


def run(rows, labels):
    return expected_consensus(np.array(rows, dtype=np.uint8), np.array(labels, dtype=np.uint32))


def test_two_rows_that_differ_everywhere():
    """every column is a 1-1 tie: the consensus is the per-column minimum, each row differs from it exactly where it holds the
    larger code (the two divs add up to L), and at equal div the nearest member is the smaller number"""
    a, b = [A, T, G, C_], [C_, G, T, A]
    ids, sizes, cons, nearest, div = run([a, b], [0, 0])
    assert ids.tolist() == [0] and sizes.tolist() == [2]
    assert cons.tolist() == [[A, G, G, A]]  # min per column
    assert div.tolist() == [2, 2] and nearest.tolist() == [0]  # equal div: the smaller number
    # rows that hold the larger code in EVERY column against one that holds the smaller: div = L and 0
    ids, sizes, cons, nearest, div = run([[T, T, T], [A, A, A]], [1, 1])
    assert cons.tolist() == [[A, A, A]] and div.tolist() == [3, 0] and nearest.tolist() == [1] and ids.tolist() == [1]


def test_a_two_two_tie_goes_to_the_smaller_code():
    ids, sizes, cons, nearest, div = run([[G], [C_], [G], [C_]], [2, 2, 2, 2])
    assert cons.tolist() == [[C_]] and div.tolist() == [1, 0, 1, 0] and nearest.tolist() == [1] and sizes.tolist() == [4]


def test_n_is_a_code_like_any_other():
    assert run([[N], [A]], [0, 0])[2].tolist() == [[A]]        # 1-1: A wins
    assert run([[N], [A], [N]], [0, 0, 0])[2].tolist() == [[N]]  # 2-1: N wins
    assert run([[N], [T], [N], [T]], [0, 0, 0, 0])[2].tolist() == [[T]]  # 2-2: the smaller code


def test_an_unlabelled_row_is_left_out():
    ids, sizes, cons, nearest, div = run([[A, A], [T, T], [T, T], [A, C_]], [0, NONE, NONE, 0])
    assert ids.tolist() == [0] and sizes.tolist() == [2] and cons.tolist() == [[A, A]]
    assert div.tolist() == [0, NONE, NONE, 1] and nearest.tolist() == [0]
    ids, sizes, cons, nearest, div = run([[A], [T]], [NONE, NONE])
    assert len(ids) == len(sizes) == len(nearest) == 0 and cons.shape == (0, 1) and div.tolist() == [NONE, NONE]


def test_a_label_need_not_be_a_member():
    ids, sizes, cons, nearest, div = run([[A], [C_], [C_], [G]], [3, 0, 0, 3])  # row 3 is in group 3, row 0 is not in group 0
    assert ids.tolist() == [0, 3] and sizes.tolist() == [2, 2]
    assert cons.tolist() == [[C_], [A]] and nearest.tolist() == [1, 0] and div.tolist() == [0, 0, 0, 1]


def nontrivial(codes, labels, multi):
    """a tied column, a group of more than `multi` rows (several windows at that chunk), a singleton, an unlabelled row and a
    label that is no member's own number"""
    values, counts = np.unique(labels[labels != NONE], return_counts=True)
    assert tied_columns(codes, labels) >= 1
    assert counts.max() > multi and (counts == 1).any() and (labels == NONE).any()
    assert any(labels[v] != v for v in values.tolist())


def test_gpu_fixtures_are_not_trivial():
    codes, labellings = chunk_case()
    nontrivial(codes, labellings["random"], 64)
    counts = np.unique(labellings["random"], return_counts=True)[1]
    assert {1, 64, 65, 600} <= set(counts.tolist())
    assert (labellings["one"] == 7).all() and tied_columns(codes, labellings["one"]) >= 0
    for name, families, D, max_subs in SHAPE_STORES:
        n = families * 10 + 20
        labels = random_grouping(n, 100 + n)
        counts = np.unique(labels[labels != NONE], return_counts=True)[1]
        assert {1, 2, 3, 63, 64, 65, 600} <= set(counts.tolist()) and (labels == NONE).sum() == n // 10, name
    for name in ("aa60", "nt330n"):  # (two of them in full: the model is slow on 25 stores)
        key = next(k for k in SHAPE_STORES if k[0] == name)
        codes, _ = shape_case(*key)
        nontrivial(codes, random_grouping(len(codes), 100 + len(codes)), 64)


@pytest.mark.parametrize("kind", ["nt", "aa"])
def test_edge_stores_cover_the_alphabet(kind):
    codes = edge_codes(kind, 513, 65, 3)
    assert set(np.unique(codes).tolist()) == set(range(28 if kind == "aa" else 5))
    labels = edge_labels(513, 3)
    assert tied_columns(codes, labels) >= 0 and len(np.unique(labels)) == 4 and (labels == NONE).any()
    assert edge_labels(1, 3).tolist() == [0]

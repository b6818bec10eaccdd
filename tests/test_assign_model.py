"""The model of the abundance table (tests/assign_cases.py: expected_assign) held to values worked by hand (CPU), and the
fixtures of tests/test_gpu_assign.py held to what those tests claim of them."""
import numpy as np
import pytest

from assign_cases import NONE, SHAPE_READS, check_against_oracle, expected_assign, planted_reads, random_samples, shape_reads
from components_cases import labels_from_pairs_numpy
from self_join_cases import SHAPE_STORES, shape_case

# four subjects of eight columns: 1 and 2 are both one column from the read "00000000"
SUBJECTS = np.array([[1, 1, 1, 1, 0, 0, 0, 0],
                     [1, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 1],
                     [3, 3, 3, 3, 3, 3, 3, 3]], dtype=np.uint8)
ZERO = np.zeros(8, dtype=np.uint8)


def rows(entries):
    return [(int(e["label"]), int(e["sample"]), int(e["count"])) for e in entries]


def test_a_tie_goes_to_the_smaller_subject_and_its_label():
    entries, subject, dist, counts, totals = expected_assign(SUBJECTS, ZERO[None], 2, labels=[7, 9, 5, 5])
    assert (subject.tolist(), dist.tolist()) == ([1], [1])  # subjects 1 and 2 tie at distance 1
    assert rows(entries) == [(9, 0, 1)]                     # ... and the label is subject 1's, not subject 2's smaller one
    assert counts.tolist() == [0, 1, 0, 0] and totals.tolist() == [1, 1, 0, 0]


def test_the_bound_is_inclusive():
    read = np.array([1, 1, 1, 0, 0, 0, 0, 0], dtype=np.uint8)  # 1 from subject 0, 2 from subject 1
    far = np.array([3, 3, 3, 3, 3, 0, 0, 0], dtype=np.uint8)   # 3 from subject 3, 5 and more from the others
    for D, want in ((3, [3]), (2, [NONE])):
        _, subject, dist, _, totals = expected_assign(SUBJECTS, far[None], D)
        assert subject.tolist() == want and dist.tolist() == ([3] if D == 3 else [NONE])
        assert totals.tolist() == ([1, 1, 0, 0] if D == 3 else [1, 0, 1, 0])
    assert expected_assign(SUBJECTS, read[None], 0)[1].tolist() == [NONE]
    assert expected_assign(SUBJECTS, read[None], 1)[1].tolist() == [0]


def test_a_read_of_weight_zero_has_a_subject_and_no_entry():
    reads = np.stack([ZERO, SUBJECTS[3]])
    entries, subject, dist, counts, totals = expected_assign(SUBJECTS, reads, 1, weights=[0, 4])
    assert subject.tolist() == [1, 3] and dist.tolist() == [1, 0]
    assert rows(entries) == [(3, 0, 4)] and counts.tolist() == [0, 0, 0, 4] and totals.tolist() == [1, 4, 0, 0]


def test_no_labels_means_identity_and_the_order_is_label_then_sample():
    reads = np.stack([SUBJECTS[3], SUBJECTS[0], SUBJECTS[3], SUBJECTS[0], SUBJECTS[2]])
    entries, _, _, counts, totals = expected_assign(SUBJECTS, reads, 0, samples=[2, 1, 0, 1, 2], n_samples=3, weights=[1, 2, 3, 4, 5])
    assert rows(entries) == [(0, 1, 6), (2, 2, 5), (3, 0, 3), (3, 2, 1)]
    assert counts.tolist() == [6, 0, 5, 4] and totals.tolist() == [4, 15, 0, 0]


def test_none_labels_and_unassigned_reads_share_one_entry_per_sample_and_come_last():
    stranger = np.full(8, 2, dtype=np.uint8)
    reads = np.stack([stranger, SUBJECTS[3], SUBJECTS[0], stranger])
    entries, subject, _, counts, totals = expected_assign(SUBJECTS, reads, 1, labels=[4, 4, 4, NONE], samples=[0, 0, 1, 1], n_samples=2)
    assert subject.tolist() == [NONE, 3, 0, NONE]
    assert rows(entries) == [(4, 1, 1), (NONE, 0, 2), (NONE, 1, 1)]  # the noise subject's read and the unassigned one: one entry
    assert totals.tolist() == [3, 2, 2, 0] and int(totals[1] + totals[2]) == 4 and counts.tolist() == [1, 0, 0, 1]


def test_a_sample_number_out_of_range_counts_in_totals_3_alone():
    reads = np.stack([SUBJECTS[0], SUBJECTS[0]])
    entries, subject, _, counts, totals = expected_assign(SUBJECTS, reads, 0, samples=[0, 5], n_samples=2, weights=[3, 7])
    assert rows(entries) == [(0, 0, 3)] and counts.tolist() == [3, 0, 0, 0] and totals.tolist() == [1, 3, 0, 1]
    assert subject.tolist() == [0, 0]


def test_an_empty_store_and_no_reads():
    entries, subject, dist, counts, totals = expected_assign(np.zeros((0, 8), np.uint8), np.stack([ZERO, ZERO]), 3, samples=[1, 1])
    assert subject.tolist() == [NONE, NONE] and dist.tolist() == [NONE, NONE] and len(counts) == 0
    assert rows(entries) == [(NONE, 1, 2)] and totals.tolist() == [1, 0, 2, 0]
    entries, subject, _, counts, totals = expected_assign(SUBJECTS, np.zeros((0, 8), np.uint8), 3)
    assert len(entries) == 0 and len(subject) == 0 and counts.tolist() == [0, 0, 0, 0] and totals.tolist() == [0, 0, 0, 0]


def test_the_totals_add_up():
    codes, reads, subject, _ = shape_reads("aa60", 150, 5)
    weights = np.arange(len(reads), dtype=np.uint32) % 6
    entries, _, _, counts, totals = expected_assign(codes, reads, 5, samples=random_samples(len(reads), 3, 1), weights=weights)
    assert int(totals[1] + totals[2]) == int(weights.sum()) == int(entries["count"].sum()) and int(counts.sum()) == int(totals[1])


@pytest.mark.parametrize("name,families,D,max_subs", SHAPE_STORES)
def test_the_fixtures_hold_what_the_gpu_tests_claim(name, families, D, max_subs):
    codes, reads, subject, dist = shape_reads(name, families, D, max_subs)
    assert len(reads) == SHAPE_READS
    found = subject != NONE
    assert found.any() and (~found).any()                             # assigned and unassigned reads
    assert set(np.unique(dist[found])) == set(range(D + 1))           # every distance up to the bound
    assert set(np.unique(random_samples(len(reads), 3, 1))) == {0, 1, 2}  # every sample is used


def test_ties_across_labels_exist_and_the_model_agrees_with_the_oracle():
    codes, reads, subject, dist = shape_reads("aa60", 150, 5)
    check_against_oracle(codes, reads, 5, subject, dist)
    labels = labels_from_pairs_numpy(len(codes), shape_case("aa60", 150, 5)[1])
    # a read at the same smallest distance from two subjects: exact copies in the store make those; with identity labels the two
    # carry different labels, so the smaller number's label has to win
    d = (reads[:, None, :] != codes[None, :, :]).sum(-1)
    tied = (d == d.min(axis=1)[:, None]).sum(axis=1) > 1
    assert (tied & (subject != NONE)).any()
    assert len(np.unique(labels)) > 1


def test_planted_reads_are_seeded():
    codes = shape_case("nt60", 150, 5)[0]
    assert planted_reads(codes, 5, 100, 3).tobytes() == planted_reads(codes, 5, 100, 3).tobytes()

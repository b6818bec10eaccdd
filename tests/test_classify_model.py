"""The model of the classification (tests/classify_cases.py: expected_classify) held to values worked by hand (CPU), and the
fixtures of tests/test_gpu_classify.py held to the coverage that test claims of them."""
import numpy as np
import pytest

from classify_cases import (NONE, ROOT, coverage, expected_classify, intern_taxonomy, lineage_text, tie_case, tie_lineage)
from self_join_cases import SHAPE_STORES

# five subjects of eight columns: 1 and 2 are both one column from the read "00000000", 0 is two from it, 4 equals subject 3
SUBJECTS = np.array([[1, 1, 0, 0, 0, 0, 0, 0],
                     [1, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 1],
                     [3, 3, 3, 3, 3, 3, 3, 3],
                     [3, 3, 3, 3, 3, 3, 3, 3]], dtype=np.uint8)
ZERO = np.zeros(8, dtype=np.uint8)
# ranks: domain, phylum, genus.  1 and 2 share the domain and the phylum; 0 shares the domain only; 3 ends behind its phylum and 4
# goes on below the same phylum
LINEAGE = np.array([[10, 21, 31],
                    [10, 20, 30],
                    [10, 20, 32],
                    [11, 22, NONE],
                    [11, 22, 33]], dtype=np.uint32)


def rows(entries):
    return [(int(e["label"]), int(e["sample"]), int(e["count"])) for e in entries]


def test_two_best_hits_of_two_genera_give_their_phylum():
    entries, subject, dist, taxon, depth, ties, totals = expected_classify(SUBJECTS, ZERO[None], 3, LINEAGE)
    assert (subject.tolist(), dist.tolist()) == ([1], [1])            # the table's anchor: the smaller number of the tie
    assert (taxon.tolist(), depth.tolist(), ties.tolist()) == ([20], [2], [2])
    assert rows(entries) == [(20, 0, 1)] and totals.tolist() == [1, 1, 0, 0, 0, 1]


def test_slack_takes_the_next_distance_in_and_the_bound_cuts_it():
    _, _, _, taxon, depth, ties, _ = expected_classify(SUBJECTS, ZERO[None], 3, LINEAGE, slack=1)
    assert (taxon.tolist(), depth.tolist(), ties.tolist()) == ([10], [1], [3])  # subject 0 at distance 2 shares the domain alone
    _, _, _, taxon, depth, ties, _ = expected_classify(SUBJECTS, ZERO[None], 1, LINEAGE, slack=1)
    assert (taxon.tolist(), depth.tolist(), ties.tolist()) == ([20], [2], [2])  # min(d + E, N) = 1: subject 0 stays out
    _, _, _, taxon, depth, ties, totals = expected_classify(SUBJECTS, ZERO[None], 8, LINEAGE, slack=NONE)
    assert (taxon.tolist(), depth.tolist(), ties.tolist()) == ([ROOT], [0], [5]) and totals.tolist() == [1, 1, 0, 0, 1, 1]


def test_a_short_anchor_caps_the_depth_and_a_short_member_does_too():
    three = SUBJECTS[3][None]
    _, subject, _, taxon, depth, ties, _ = expected_classify(SUBJECTS, three, 0, LINEAGE)
    assert (subject.tolist(), taxon.tolist(), depth.tolist(), ties.tolist()) == ([3], [22], [2], [2])  # the anchor ends at rank 2
    swapped = LINEAGE[[0, 1, 2, 4, 3]]
    _, subject, _, taxon, depth, _, _ = expected_classify(SUBJECTS, three, 0, swapped)
    assert (subject.tolist(), taxon.tolist(), depth.tolist()) == ([3], [22], [2])                       # ... and so does the other member
    alone = expected_classify(SUBJECTS[:4], three, 0, LINEAGE[:4])
    assert (alone[3].tolist(), alone[4].tolist(), alone[5].tolist()) == ([22], [2], [1])               # s = anchor is included
    empty = LINEAGE.copy()
    empty[4] = NONE
    _, _, _, taxon, depth, _, totals = expected_classify(SUBJECTS, three, 0, empty)
    assert (taxon.tolist(), depth.tolist()) == ([ROOT], [0]) and int(totals[4]) == 1


def test_no_subject_within_the_bound():
    entries, subject, dist, taxon, depth, ties, totals = expected_classify(SUBJECTS, np.full((1, 8), 2, np.uint8), 3, LINEAGE)
    assert subject.tolist() == dist.tolist() == taxon.tolist() == depth.tolist() == [NONE] and ties.tolist() == [0]
    assert rows(entries) == [(NONE, 0, 1)] and totals.tolist() == [1, 0, 1, 0, 0, 0]


def test_the_order_is_taxon_then_sample_root_behind_every_taxon_unassigned_last():
    reads = np.stack([np.full(8, 2, np.uint8), SUBJECTS[3], ZERO, SUBJECTS[3], ZERO])
    lineage = LINEAGE.copy()
    lineage[4] = [12, 23, 33]  # the twins 3 and 4 share nothing: the root
    entries, _, _, taxon, _, _, totals = expected_classify(SUBJECTS, reads, 3, lineage, samples=[1, 1, 0, 0, 5], n_samples=2, weights=[2, 3, 4, 0, 7])
    assert taxon.tolist() == [NONE, ROOT, 20, ROOT, 20]
    assert rows(entries) == [(20, 0, 4), (ROOT, 1, 3), (NONE, 1, 2)]  # weight 0 and the stray sample are in no entry
    assert totals.tolist() == [3, 7, 2, 1, 3, 3]                      # ties > 1: reads 1, 2 and 3 (weight 0 counts, the stray does not)


def test_an_empty_store_and_no_reads():
    entries, subject, _, taxon, depth, ties, totals = expected_classify(np.zeros((0, 8), np.uint8), np.stack([ZERO, ZERO]), 3, np.zeros((0, 3), np.uint32))
    assert subject.tolist() == taxon.tolist() == depth.tolist() == [NONE, NONE] and ties.tolist() == [0, 0]
    assert rows(entries) == [(NONE, 0, 2)] and totals.tolist() == [1, 0, 2, 0, 0, 0]
    entries, subject, *_, totals = expected_classify(SUBJECTS, np.zeros((0, 8), np.uint8), 3, LINEAGE)
    assert len(entries) == 0 and len(subject) == 0 and totals.tolist() == [0] * 6


def test_interning_gives_every_node_an_id_of_its_own():
    lineage, names, parents = intern_taxonomy(4, [(2, ["Root", "d__B", "g__X"]), (0, ["Root", "d__A", "g__X"]), (3, ["Root", "d__B"])])
    assert lineage.tolist() == [[0, 3, 4], [NONE] * 3, [0, 1, 2], [0, 1, NONE]]  # first appearance in the file; g__X twice
    assert lineage_text(4, names, parents) == "Root;d__A;g__X" and lineage_text(2, names, parents) == "Root;d__B;g__X"
    assert lineage_text(ROOT, names, parents) == "root" and lineage_text(NONE, names, parents) == "unassigned"


@pytest.mark.parametrize("name,families,D,max_subs", SHAPE_STORES)
def test_the_fixtures_hold_what_the_gpu_test_claims(name, families, D, max_subs):
    """ties are the rule, every depth occurs, both NONE-tail cases and an unassigned read occur — at every R and slack the GPU test
    runs"""
    store, reads, dmat = tie_case(name, families, D, max_subs)
    for R in (1, 7, 16):
        lineage = tie_lineage(name, families, D, max_subs, R)
        for row in lineage:  # what the host form would refuse
            assert ROOT not in row and not (row[1:][row[:-1] == NONE] != NONE).any()
        for slack in (0, 1, D):
            share, depths, anchor_shortest, other_shortest, unassigned = coverage(store, dmat, D, lineage, slack)
            assert share >= 0.25 and depths == set(range(R + 1)) and anchor_shortest and other_shortest and unassigned, (R, slack, share, depths)

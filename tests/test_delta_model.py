"""The delta join's two rules on the CPU (numpy), against brute force: the exactly-once rule of smafa_dl::delta_filter_kernel on
raw lists — a scan of the new rows against the WHOLE store, self-pairs and mirror images included — and the seed-and-link
update of the components (seed_parents_kernel, link_rows_kernel, flatten_labels_kernel)."""
import numpy as np
import pytest

from components_cases import brute_labels, n_components
from delta_cases import delta_filter, has_both_kinds, marks, pair_keys, seed_and_link, since, store_case
from self_join_cases import SHAPES
from smafa_amd import HIT_DTYPE


def raw_list(want, first_row, n):
    """what the scans of records r = 0 .. n - first_row - 1 (subject first_row + r) leave: both directions of every pair that
    a new row is in, seen from the new row, and the new rows' self-pairs; shuffled"""
    lo, hi = want[want["subject"] >= first_row], want[want["query"] >= first_row]
    rows = np.zeros(len(lo) + len(hi) + (n - first_row), dtype=HIT_DTYPE)
    rows["query"][:len(lo)], rows["subject"][:len(lo)], rows["dist"][:len(lo)] = lo["subject"] - first_row, lo["query"], lo["dist"]
    k = len(lo)
    rows["query"][k:k + len(hi)], rows["subject"][k:k + len(hi)], rows["dist"][k:k + len(hi)] = hi["query"] - first_row, hi["subject"], hi["dist"]
    k += len(hi)
    rows["query"][k:], rows["subject"][k:] = np.arange(n - first_row), np.arange(first_row, n)
    np.random.default_rng(first_row).shuffle(rows)
    return rows


@pytest.mark.parametrize("name", ["aa60", "nt60n", "aa60d0"])
def test_filter_rule_partitions_the_pairs(name):
    codes, want, D = store_case(name)
    n = len(codes)
    rng = np.random.default_rng(4)
    for n0 in marks(n) + [int(x) for x in rng.integers(2, n - 1, size=6)]:
        got = delta_filter(raw_list(want, n0, n), np.arange(n0, n, dtype=np.uint32))
        got = got[np.lexsort((got["subject"], got["dist"], got["query"]))]
        assert got.tobytes() == since(want, n0).tobytes(), n0
        assert len(np.unique(pair_keys(got))) == len(got)
        old = want[want["subject"] < n0]  # the pairs of the store's first n0 rows
        assert len(np.intersect1d(pair_keys(old), pair_keys(got))) == 0
        assert np.array_equal(np.sort(np.concatenate([pair_keys(old), pair_keys(got)])), np.sort(pair_keys(want)))


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_fixture_has_both_pair_kinds(name):
    """what tests/test_gpu_delta_join.py asserts again on the GPU machine: at first_row = n / 2 and n - 300 every shape has
    old-new and new-new pairs at every distance 0..D"""
    codes, want, D = store_case(name)
    n = len(codes)
    for n0 in (n // 2, n - 300):
        assert has_both_kinds(since(want, n0), n0, D), (name, n0)


@pytest.mark.parametrize("name", ["aa60", "nt60n"])
@pytest.mark.parametrize("D", [0, 2, 5])
def test_seed_and_link_gives_the_labels_of_the_whole_store(name, D):
    codes, want5, _ = store_case(name)
    want = want5[want5["dist"] <= D]
    labels = np.zeros(0, dtype=np.uint32)
    before = 0
    for n_now in (1000, 2000, 3020):
        delta = since(want[want["subject"] < n_now], before)
        labels, bad = seed_and_link(labels, before, n_now, zip(delta["query"], delta["subject"]))
        full, _ = brute_labels(codes[:n_now], D)
        assert bad == 0 and labels.tobytes() == full.tobytes(), (n_now, D)
        assert n_components(labels) == n_components(full)
        before = n_now


def test_seed_counts_what_cannot_be_a_label():
    codes, want, D = store_case("aa60")
    full, _ = brute_labels(codes[:1000], D)
    above = full.copy()
    above[10] = 11  # larger than its index
    assert seed_and_link(above, 1000, 1000, [])[1] >= 1
    member = int(np.nonzero(full != np.arange(1000))[0][0])  # a row that is no representative
    later = int(np.nonzero((full != np.arange(1000)) & (np.arange(1000) > member))[0][0])  # another one: nobody points at it
    chained = full.copy()
    chained[later] = member  # points at a non-root
    assert seed_and_link(chained, 1000, 1000, [])[1] == 1
    assert seed_and_link(full, 1000, 1000, [])[1] == 0

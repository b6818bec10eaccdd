"""Every resident-store call on stores of 69 740 rows, under the DEFAULT knobs: the first stores of the suite that the default
join geometry cuts (one span dealt into two blocks of 34 870 records; SMAFA_JOIN_BLOCK is 65 536), whose row numbers, positions
and tile numbers need 17 bits, whose last tile of 256 is ragged, and whose consensus call votes over 18 windows of 4 096 entries.

Nothing is expected from the code under test: tests/big_store_cases.py builds the stores from families that cannot be within the
bound of each other and scatters the existing brute-force models' answers for each family's template;
tests/test_big_store_model.py holds that scatter to the whole-store models on the CPU.  Every call is held byte for byte, the
two forests to their documented contract.

The two default blocks hold the span's even and its odd positions (self_join.hip.h: join_pass deals a span round-robin), and
each is scanned once against the whole span: two scans a join, which the pairs test observes, and no "position 65 536" divides
the blocks.  That pairs cross the blocks needs no position: of 590 840 pairs inside families of up to 40 rows not every one
can join two positions of one parity, and a call that lost those would not give the expected bytes.
The file takes 2.7 s on an MI355X (expectations included)."""
import time

import numpy as np
import pytest

import smafa_amd
from big_store_cases import D, DEFAULT_BLOCK, DEFAULT_STRIDE, STORES, WINDOW, big_store, consensus_of
from self_join_cases import join_spans

pytestmark = pytest.mark.gpu
LATE = 3000  # the rows of the second push
KNOBS = ("SMAFA_DENSITY_KEEP_MAX", "SMAFA_JOIN_BLOCK", "SMAFA_JOIN_STRIDE", "SMAFA_JOIN_SCRATCH_MAX", "SMAFA_CONSENSUS_CHUNK",
         "SMAFA_NEIGHBOUR_SORT")


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for var in KNOBS:
        monkeypatch.delenv(var, raising=False)


def make_store(case, pieces=None):
    store = smafa_amd.SubjectStore(case.L, smafa_amd.ALPHABET_AA if case.kind == "aa" else smafa_amd.ALPHABET_NT)
    for p in pieces or [case.codes]:
        store.push(p)
    assert len(store) == case.n and store.info().planes == {"nt120": 2, "aa60": 5, "nt120n": 3}[case.name]
    return store


def eq(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, getattr(got, "dtype", None),
                                                                                                  getattr(got, "shape", None), want.shape)
    assert got.tobytes() == want.tobytes(), "%s differs from the model at %s" % (what, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8])


def blocks_of(n, block=DEFAULT_BLOCK, stride=DEFAULT_STRIDE):
    return sum(S for _, _, S, _ in join_spans(n, block, stride))


def check_pairs(store, case, what=""):
    got = store.self_pairs(D, first_cap=1 << 20)
    stats = store.last_call_stats()
    blocks = blocks_of(case.n)
    print("%s%s: %d rows, %d pairs, %d scans, %d blocks" % (case.name, what, case.n, len(case.pairs()), stats["scans"], blocks))
    eq(got, case.pairs(), "pairs")
    # one scan per block (>=: a block whose list outgrew the scratch list is scanned again); see the module docstring
    assert blocks >= 2 and stats["scans"] >= blocks, (stats, blocks)
    kernels = store.last_call_kernels()
    assert "smafa_join::store_records_kernel" in kernels and "smafa_join::join_filter_kernel" in kernels
    return got


def check_components(answer, case):
    eq(answer[0], case.components()[0], "labels")
    assert answer[1] == case.components()[1]


def check_levels(answer, case):
    eq(answer[0], case.levels()[0], "level labels")
    assert list(answer[1]) == case.levels()[1]


def check_density(answer, case, M):
    want = case.density(M)
    eq(answer[1], want[1], "degrees")
    eq(answer[0], want[0], "density labels")
    assert answer[2] == want[2], (answer[2], want[2])


def check_peaks(answer, case, radius):
    want = case.peaks(radius)
    eq(answer[2], want[2], "weights")
    eq(answer[1], want[1], "parents")
    eq(answer[0], want[0], "peak labels")
    assert answer[3] == want[3], (answer[3], want[3])


def check_neighbours(answer, case, k):
    for got, want, what in zip(answer, case.neighbours(k), ("offsets", "neighbours", "dists")):
        eq(got, want, what)


def check_stable(answer, case):
    labels, count, joined, cores = answer
    want = case.stable()
    eq(cores, want[3], "cores")
    eq(labels, want[0], "stable labels")
    eq(joined, want[1], "joined")
    assert count == want[2], (count, want[2])


def check_forest(answer, case):
    case.check_forest(answer[0], answer[1], *case.levels())


def check_reach(answer, case):
    cores, labels, counts = case.reach()
    eq(answer[2], cores, "cores")
    case.check_forest(answer[0], answer[1], labels, counts, cores=cores)


def check_consensus(answer, case, labels):
    for got, want, what in zip(answer, consensus_of(case.codes, labels), ("ids", "sizes", "codes", "nearest", "div")):
        eq(got, want, what)


def update_of(store, case, mark):
    seed = np.zeros(case.n, dtype=np.uint32)
    seed[:mark] = case.labels_before(mark)
    return store.self_components_update(mark, D, seed)


@pytest.mark.parametrize("name", list(STORES))
def test_pairs(name):
    case = big_store(name)
    store = make_store(case)
    check_pairs(store, case)
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_delta_calls_behind_a_second_push(name):
    """the last 3 000 rows pushed on their own: the mark, 66 740, lies above 65 536"""
    case = big_store(name)
    mark = case.n - LATE
    assert mark > DEFAULT_BLOCK
    store = make_store(case, [case.codes[:mark], case.codes[mark:]])
    want = case.since(mark)
    assert (want["query"] < mark).any() and (want["query"] >= mark).any()  # old-new and new-new pairs
    eq(store.self_pairs_since(mark, D), want, "delta pairs")
    check_components(update_of(store, case, mark), case)
    print("%s: mark %d, %d delta pairs" % (name, mark, len(want)))
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_components_and_levels(name):
    case = big_store(name)
    store = make_store(case)
    check_components(store.self_components(D), case)
    check_levels(store.self_component_levels(D), case)
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_density_and_peaks(name):
    case = big_store(name)
    store = make_store(case)
    for M in (2, 4):
        check_density(store.self_density(D, M), case, M)
    check_peaks(store.self_peaks(D), case, 0)
    check_peaks(store.self_peaks(D, radius=2), case, 2)
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_neighbours(name):
    case = big_store(name)
    store = make_store(case)
    check_neighbours(store.self_neighbours(D, first_cap=1 << 21), case, None)
    check_neighbours(store.self_neighbours(D, 3, first_cap=1 << 21), case, 3)
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_stable_clusters(name):
    case = big_store(name)
    store = make_store(case)
    check_stable(store.self_stable_clusters(D, 3, 0, joined=True, cores=True), case)
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_forests(name):
    case = big_store(name)
    store = make_store(case)
    check_forest(store.self_forest(D), case)
    check_reach(store.self_reach_forest(D, 3), case)
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_consensus(name):
    """under the components, under all singletons, and under one label over 20 000 scattered rows: 18 windows of 4 096 entries,
    a group that crosses at least four of their edges"""
    case = big_store(name)
    n = case.n
    store = make_store(case)
    planes = store.info().planes
    components = case.components()[0]
    check_consensus(store.cluster_consensus(components), case, components)
    ids, sizes, cons, nearest, div = store.cluster_consensus(np.arange(n, dtype=np.uint32))
    assert cons.tobytes() == case.codes.tobytes() and not div.any() and (sizes == 1).all()
    assert ids.tobytes() == nearest.tobytes() == np.arange(n, dtype=np.uint32).tobytes()
    window = case.window_labels()
    big = int(np.bincount(window).max())  # (no row of these labellings is unlabelled)
    assert big >= 20000 and big // WINDOW >= 4 and -(-n // WINDOW) == 18
    answer = store.cluster_consensus(window)
    kernels = store.last_call_kernels()
    print("%s: consensus of a group of %d rows among %d groups, %d windows, kernels %s" % (name, big, len(answer[0]), -(-n // WINDOW), kernels))
    check_consensus(answer, case, window)
    assert "consensus::vote_tables_kernel<%d>" % planes in kernels and "consensus::tally_vote_kernel<%d>" % planes in kernels
    assert int(answer[1].max()) == big
    store.close()


@pytest.mark.parametrize("knob,value", [("SMAFA_JOIN_BLOCK", 16384), ("SMAFA_NEIGHBOUR_SORT", 2)])
def test_same_bytes_under_knobs(knob, value, monkeypatch):
    """nt120 in five blocks of 16 384, and under the other neighbour sort: the bytes of the default knobs, which are the model's"""
    case = big_store("nt120")
    monkeypatch.setenv(knob, str(value))  # (read when the handle is made)
    store = make_store(case)
    monkeypatch.delenv(knob)
    eq(store.self_pairs(D, first_cap=1 << 20), case.pairs(), "pairs")
    scans = store.last_call_stats()["scans"]
    check_neighbours(store.self_neighbours(D, first_cap=1 << 21), case, None)
    print("nt120, %s=%d: %d scans of the pairs call" % (knob, value, scans))
    if knob == "SMAFA_JOIN_BLOCK":
        assert blocks_of(case.n, value) == 5 and scans >= 5, scans
    store.close()


@pytest.mark.parametrize("name", list(STORES))
def test_every_call_on_one_handle(name):
    """all calls in sequence on one handle, the second push included, then the first call again: the same bytes from buffers
    grown for 69 740 rows"""
    case = big_store(name)
    mark = case.n - LATE
    t0 = time.time()
    store = make_store(case, [case.codes[:mark], case.codes[mark:]])
    first = check_pairs(store, case, ", one handle")
    eq(store.self_pairs_since(mark, D), case.since(mark), "delta pairs")
    check_components(update_of(store, case, mark), case)
    check_components(store.self_components(D), case)
    check_levels(store.self_component_levels(D), case)
    for M in (2, 4):
        check_density(store.self_density(D, M), case, M)
    check_peaks(store.self_peaks(D), case, 0)
    check_peaks(store.self_peaks(D, radius=2), case, 2)
    check_neighbours(store.self_neighbours(D, first_cap=1 << 21), case, None)
    check_neighbours(store.self_neighbours(D, 3, first_cap=1 << 21), case, 3)
    check_stable(store.self_stable_clusters(D, 3, 0, joined=True, cores=True), case)
    check_forest(store.self_forest(D), case)
    check_reach(store.self_reach_forest(D, 3), case)
    check_consensus(store.cluster_consensus(case.window_labels()), case, case.window_labels())
    again = check_pairs(store, case, ", one handle, again")
    assert again.tobytes() == first.tobytes()
    print("%s: every call on one handle in %.1f s" % (name, time.time() - t0))
    store.close()

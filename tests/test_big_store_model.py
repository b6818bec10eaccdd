"""The construction of tests/big_store_cases.py, on the CPU: the distance bound between families, the distances inside them,
the interleaving, and — on a 3 000-row instance of the same generator — that the scattered answers of the templates ARE the
answers of the existing whole-store brute-force models, for every call tests/test_gpu_big_store.py makes, tie rules included."""
import numpy as np
import pytest

from big_store_cases import (D, DEFAULT_BLOCK, NAMES, NONE, S_MAX, SIZES, STORES, TEMPLATES, WINDOW, big_store, bound_of, consensus_of,
                             greatest_in_family_distance, in_family_distances, local)
from components_cases import labels_from_pairs, n_components
from consensus_cases import expected_consensus, random_grouping
from density_cases import density_from_pairs
from forest_cases import expected_levels
from neighbours_cases import brute_neighbours, cut_lists
from peaks_cases import peaks_from_pairs
from reach_cases import expected_reach
from self_join_cases import brute_pairs, join_spans
from stable_cases import expected_stable

SMALL = 23  # every template's family count divided by 23: about 3 000 rows


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), "%s: the scatter differs from brute force at %s" % (what, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8])


def test_templates_and_bound():
    assert bound_of("nt120") == 16 - 2 * S_MAX == 10 and bound_of("aa60") == bound_of("nt120n") + 4 == 14
    assert in_family_distances() == list(range(D + 1))
    assert greatest_in_family_distance() == 2 * S_MAX  # (two members that change disjoint triples: no pair at D = 5)
    assert 10 <= len(NAMES) <= 16 and SIZES.min() == 1 and SIZES.max() == 40
    for matrix, _ in TEMPLATES.values():
        assert matrix.max() <= 3  # offsets 1 .. 3: two offsets differ mod 4 and mod 20 alike


def test_templates_differ_from_single_linkage():
    """what the module docstring of big_store_cases says of bridge, late, spokes and pair5, on the models' own answers"""
    by_name = {name: local(t) for t, name in enumerate(NAMES)}
    bridge, late, spokes, pair5 = (by_name[k] for k in ("bridge", "late", "spokes", "pair5"))
    assert bridge["levels"][1][D] == 1 and bridge["peaks", 0][3] == 2           # one component, two peaks
    assert bridge["levels"][1][:3] == [5, 3, 1]                                 # the chain closes at 2; below it the groups stand apart
    assert late["levels"][1][D] == 1 and late["stable"][2] == 2                 # one component, two stable clusters
    assert (late["stable"][1] == 0).all() and (late["reach"][0] == 0).all()
    labels, degrees, counts = spokes["density", 4]
    assert spokes["levels"][1][D] == 1 and counts == {"clusters": 1, "core": 1, "noise": 0} and degrees.tolist() == [1, 3, 1, 1]  # borders
    assert pair5["levels"][1][D] == 1 and pair5["density", 4][2]["noise"] == 2 and pair5["density", 2][2]["clusters"] == 1
    assert by_name["pair6"]["levels"][1][D] == 2 and len(by_name["pair6"]["pairs"]) == 0


@pytest.mark.parametrize("name", list(STORES))
def test_full_size_store(name):
    """n, the interleaving, the pair count by templates, and the bound on a sample the reference can afford: 300 random rows
    against all rows"""
    store = big_store(name)
    n, codes = store.n, store.codes
    assert DEFAULT_BLOCK < n < 2 * DEFAULT_BLOCK and n % 256 and n == 69740
    assert [(S, R) for _, _, S, R in join_spans(n, DEFAULT_BLOCK, 16)] == [(2, 34870)]  # one span dealt into two blocks
    assert -(-n // WINDOW) == 18
    assert codes.shape == (n, STORES[name][1])
    if store.kind == "nt":  # (4 is N there, and a letter like any other among the amino acids)
        assert (codes == 4).any() == (name == "nt120n") and codes.max() == (4 if name == "nt120n" else 3)
    # increasing maps, members in template order
    for f in (0, 1, store.F // 2, store.F - 1):
        rows = store.row_of[store.start[f]:store.start[f] + SIZES[store.tmpl[f]]]
        assert (np.diff(rows) > 0).all() and (store.fam[rows] == f).all() and store.member[rows].tolist() == list(range(len(rows)))
    order = np.lexsort((store.member, store.fam))
    assert (np.diff(order)[np.diff(store.fam[order]) == 0] > 0).all()  # every family, at once
    want = store.pairs()
    assert len(want) == store.pair_count_by_templates() == sum(int((store.tmpl == t).sum()) * len(local(t)["pairs"]) for t in range(len(NAMES)))
    assert set(np.unique(want["dist"])) == set(range(D + 1))
    # the sample
    rng = np.random.default_rng(300)
    pick = np.sort(rng.choice(n, size=300, replace=False))
    nearest_stranger = 1 << 30
    found = []
    for a in range(0, 300, 20):
        who = pick[a:a + 20]
        dist = (codes[who][:, None, :] != codes[None, :, :]).sum(axis=2)
        stranger = store.fam[who][:, None] != store.fam[None, :]
        nearest_stranger = min(nearest_stranger, int(dist[stranger].min()))
        i, j = np.nonzero(dist <= D)
        keep = who[i] != j
        found.append(np.stack([np.minimum(who[i], j), np.maximum(who[i], j), dist[i, j]], axis=1)[keep])
    assert nearest_stranger >= store.bound > D, (nearest_stranger, store.bound)
    found = np.unique(np.concatenate(found), axis=0)
    touching = want[np.isin(want["query"], pick) | np.isin(want["subject"], pick)]
    expected = np.unique(np.stack([touching[k].astype(np.int64) for k in ("query", "subject", "dist")], axis=1), axis=0)
    assert len(found) > 1000 and found.tolist() == expected.tolist()


@pytest.mark.parametrize("name", list(STORES))
def test_scatter_equals_whole_store_brute_force(name):
    """a 3 000-row store of the same generator: every scattered expectation against the existing model on the whole store"""
    store = big_store(name, SMALL)
    n, codes = store.n, store.codes
    assert 2500 < n < 3500 and len(set(store.tmpl.tolist())) == len(NAMES)
    pairs = brute_pairs(codes, D)
    same(store.pairs(), pairs, "pairs")
    labels, counts, _ = expected_levels(codes, D)
    same(store.levels()[0], labels, "levels")
    assert store.levels()[1] == counts
    same(store.components()[0], labels_from_pairs(n, pairs), "components")
    assert store.components()[1] == n_components(labels[D])
    for M in (2, 4):
        want = density_from_pairs(n, pairs, M)
        same(store.density(M)[0], want[0], "density labels")
        same(store.density(M)[1], want[1], "degrees")
        assert store.density(M)[2] == want[2]
    for radius in (0, 2):
        want = peaks_from_pairs(n, pairs, radius)
        for k, what in enumerate(("peak labels", "parents", "weights")):
            same(store.peaks(radius)[k], want[k], what)
        assert store.peaks(radius)[3] == want[3]
    whole = brute_neighbours(codes, D)
    for k in (None, 3):
        for got, want, what in zip(store.neighbours(k), cut_lists(whole, k), ("offsets", "neighbours", "dists")):
            same(got, want, what)
    cores, labels, counts = expected_reach(codes, D, 3)
    same(store.reach()[0], cores, "cores")
    same(store.reach()[1], labels, "reach levels")
    assert store.reach()[2] == counts
    want = expected_stable(codes, D, 3, 0)
    same(store.stable()[0], want[0], "stable labels")
    same(store.stable()[1], want[1], "joined")
    same(store.stable()[3], want[3], "stable cores")
    assert store.stable()[2] == want[2] and (want[0] == NONE).any()
    # the delta calls
    mark = n - 300
    same(store.since(mark), np.ascontiguousarray(pairs[pairs["subject"] >= mark]), "delta pairs")
    assert (store.since(mark)["query"] < mark).any() and (store.since(mark)["query"] >= mark).any()
    same(store.labels_before(mark), labels_from_pairs(mark, pairs[pairs["subject"] < mark]), "labels before the mark")
    # the consensus: under the components, under the window labelling (a group of a third of the rows) and under a grouping
    # that ignores the families, unlabelled rows and ties included
    for labelling in (store.components()[0], store.window_labels(), random_grouping(n, 5)):
        for got, want, what in zip(consensus_of(codes, labelling), expected_consensus(codes, labelling), ("ids", "sizes", "codes", "nearest", "div")):
            same(got, want, what)
    # the forest checker takes a true forest and refuses a wrong one
    edges = pairs[np.argsort(pairs["dist"], kind="stable")]
    keep, seen = [], np.arange(n)
    for k, (a, b) in enumerate(zip(edges["query"].tolist(), edges["subject"].tolist())):  # Kruskal, plainly
        ra, rb = seen[a], seen[b]
        if ra != rb:
            seen[seen == max(ra, rb)] = min(ra, rb)
            keep.append(k)
    forest = np.ascontiguousarray(edges[keep])
    ends = np.array([(forest["dist"] <= t).sum() for t in range(D + 1)], dtype=np.uint64)
    store.check_forest(forest, ends, *store.levels())
    wrong = forest.copy()
    stranger = np.flatnonzero((store.fam != store.fam[wrong["query"][0]]) & (np.arange(n) > wrong["query"][0]))[0]
    wrong["subject"][0] = stranger  # an edge into another family
    with pytest.raises(AssertionError, match="two families"):
        store.check_forest(wrong, ends, *store.levels())
    with pytest.raises(AssertionError):
        store.check_forest(forest[1:], ends, *store.levels())

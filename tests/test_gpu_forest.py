"""Minimum spanning forest of a resident store (smafa_db_self_forest / smafa_db_self_forest_launch / `smafa forest`): the
edges {a, b, dist}, ordered by dist, whose prefixes [0, level_ends[t]) are acyclic and connect exactly the components at
bound t, for every t = 0 .. D, from one join.

Expected values never come from the code under test (tests/forest_cases.py): the partitions are brute force on the code
bytes (levels_cases.brute_levels), the distance of every edge is recomputed from the code bytes, and the edges are walked
through a plain union-find.  Which of several pairs of equal distance is chosen is free, so no test compares edge lists
byte for byte.  At 1M rows, where brute force is out of reach, the partitions are held against the levels call, which
tests/test_gpu_levels.py holds against brute force."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import chain_store, dense_store
from forest_cases import as_edges, check_forest, check_shape, expected_levels, sorted_inside_levels, walk_forest
from self_join_cases import SHAPES, planted_store

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = ["smafa_sf::init_forest_kernel", "smafa_sf::keep_pairs_kernel", "smafa_sf::span_edges_kernel"]
STAR = "smafa_sf::star_roots_kernel"


@functools.lru_cache(maxsize=None)
def case(name, families):
    """-> (codes, D) of a shape of SHAPES at `families` x 10 + 20 rows, the stores of tests/test_gpu_levels.py (same seeds)"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    return planted_store(11 + families + len(name), kind, L, families, n_frac), D


def kind_of(name):
    return next(s for s in SHAPES if s[0] == name)[1]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def no_foreign_kernels(kernels):
    assert not [k for k in kernels if k.startswith(("smafa_cc::", "smafa_lv::", "smafa_dn::"))], kernels


@pytest.mark.parametrize("name,families", [(s[0], 300) for s in SHAPES] + [("aa60", 2000)])
def test_forest_equals_brute_force(name, families):
    codes, D = case(name, families)
    store = make_store(codes, kind_of(name))
    edges, ends = store.self_forest(D)
    print("%s x %d rows, D = %d: level ends %s, kernels %s" % (name, len(codes), D, ends.tolist(), store.last_call_kernels()))
    counts = check_forest(codes, edges, ends, D)
    if D >= 2:  # every level a different answer
        assert len(set(counts)) >= 3, (name, counts)
    assert sorted_inside_levels(edges)
    no_foreign_kernels(store.last_call_kernels())
    assert store.last_call_stats()["scans"] >= 1
    store.close()


@pytest.mark.parametrize("ceiling", [None, "1000000"])
def test_dense_store(ceiling, monkeypatch):
    """2 000 copies of one row + 2 000 of a second row at distance 3: 16M rows in the one block's list, every pair of the store
    kept.  Exactly 3 998 edges of weight 0 and ONE of weight 3 — a build that unites all classes in one launch lets heavy rows
    win hooks that the light rows make redundant, and fails here.  The kernels that ran are smafa_sf::init_forest_kernel,
    smafa_sf::keep_pairs_kernel and smafa_sf::span_edges_kernel, in this order, after the scans and the join's two kernels —
    and none of smafa_cc::, smafa_lv:: or smafa_dn::."""
    codes, group = dense_store()
    first = [int(np.flatnonzero(group == g)[0]) for g in (0, 1)]
    assert min(first) == 0
    two = np.array(first, dtype=np.uint32)[group]
    if ceiling:
        monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", ceiling)
    store = make_store(codes, "nt")
    edges, ends = store.self_forest(3)
    assert ends.tolist() == [3998, 3998, 3998, 3999], ends.tolist()
    check_shape(codes, edges, ends, 3)
    assert (edges["dist"][:3998] == 0).all() and edges["dist"][3998] == 3
    for t, labels in walk_forest(len(codes), edges, ends):
        assert labels.tobytes() == (two if t < 3 else np.zeros(4000, dtype=np.uint32)).tobytes(), t
    kernels = store.last_call_kernels()
    no_foreign_kernels(kernels)
    assert "smafa_join::join_filter_kernel" not in kernels, kernels
    assert kernels[-3:] == SF and [k for k in kernels if k.startswith("smafa_sf::")] == SF, kernels
    assert kernels[-5:-3] == ["smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel"], kernels
    assert kernels[0].startswith("smafa::"), kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 8 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    if ceiling:  # 16M rows over a list of 1M: the piece was cut more than once; the kept list holds 1M of 8M pairs: the slow path
        assert stats["scans"] > 4, stats
    store.close()


def test_chains():
    """three shuffled chains of 2 048 rows whose neighbours are at distance exactly 1: long paths, deep trees"""
    codes = chain_store(1)[0]
    store = make_store(codes, "nt")
    edges, ends = store.self_forest(3)
    counts = check_forest(codes, edges, ends, 3)
    assert counts[1:] == [3, 3, 3] and counts[0] > 3, counts
    store.close()


def test_slow_path(monkeypatch):
    """the kept list may hold no pair, or fewer than there are: the store is joined once more per class and the raw piece lists —
    mirror images, repeats and self-pairs included — are spanned.  The same contract, more scans."""
    codes, D = case("aa60", 2000)
    n_pairs = expected_levels(codes, D)[2]
    store = make_store(codes, "aa")
    check_forest(codes, *store.self_forest(D), D)
    normal = store.last_call_stats()["scans"]
    store.close()
    for room in ("0", str(n_pairs // 2)):
        assert int(room) < n_pairs
        monkeypatch.setenv("SMAFA_DENSITY_KEEP_MAX", room)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv("SMAFA_DENSITY_KEEP_MAX")
        edges, ends = store.self_forest(D)
        check_forest(codes, edges, ends, D)
        assert sorted_inside_levels(edges)
        assert store.last_call_stats()["scans"] > normal, (room, store.last_call_stats(), normal)  # 1 + (D + 1) joins
        kernels = store.last_call_kernels()
        assert [k for k in kernels if k.startswith("smafa_sf::")] == SF, kernels
        no_foreign_kernels(kernels)
        store.close()


def test_every_engine_one_contract(monkeypatch):
    name = "aa60"
    codes, D = case(name, 2000)

    def check(store):
        return check_forest(codes, *store.self_forest(D), D)

    store = make_store(codes, "aa")
    check(store)
    assert store.last_call_kernels()[0].startswith("smafa::scan_"), store.last_call_kernels()
    for on in (False, True):
        store.set_prefilter(on)
        check(store)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        check(store)
        if level == 2:
            assert any("scan_zone_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()
    store.close()
    # a current block index answers the blocks (limits lifted as tests/test_gpu_self_join.py lifts them)
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = make_store(codes, "aa")
    info = store.build_index(D)
    store.set_index(1)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    before = store.index_info()["probe_launches"]
    check(store)
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    for var, value in (("SMAFA_JOIN_STRIDE", "1"), ("SMAFA_JOIN_BLOCK", "128")):
        monkeypatch.setenv(var, value)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv(var)
        check(store)
        if var == "SMAFA_JOIN_BLOCK":  # 20 020 rows in blocks of 128
            assert store.last_call_stats()["scans"] >= 20020 // 128, store.last_call_stats()
        store.close()


def test_edges_and_errors():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    edges, ends = store.self_forest(5)
    assert len(edges) == 0 and edges.dtype == smafa_amd.HIT_DTYPE and ends.tolist() == [0] * 6
    rng = np.random.default_rng(4)
    first = rng.integers(0, 4, size=(1, L)).astype(np.uint8)
    store.push(first)
    edges, ends = store.self_forest(5)
    assert len(edges) == 0 and ends.tolist() == [0] * 6
    assert not [k for k in store.last_call_kernels() if k.startswith("smafa::")], store.last_call_kernels()  # no scan
    edges, ends = store.self_forest(L + 2)  # one row is a spanning tree of itself
    assert len(edges) == 0 and ends.tolist() == [0] * (L + 3)
    rest = rng.integers(0, 4, size=(299, L)).astype(np.uint8)
    rest[100] = rest[7]  # one pair of equal rows among unrelated ones
    rest[200] = rest[7]
    rest[200, 5] = (rest[200, 5] + 1) % 4  # and a third row at distance 1 of them
    store.push(rest)
    codes = np.concatenate([first, rest])
    edges, ends = store.self_forest(5)
    check_forest(codes, edges, ends, 5)
    assert ends.tolist() == [1, 2, 2, 2, 2, 2] and edges[0].tolist() == (8, 101, 0) and edges[1]["subject"] == 201 and edges[1]["dist"] == 1
    check_forest(codes, *store.self_forest(0), 0)
    store.close()
    # bounds no two rows can exceed: a spanning tree; the edges below L are still held against brute force, the ones at L hang
    # every remaining root under row 0 (smafa_sf::star_roots_kernel)
    L = 9
    codes = planted_store(5, "nt", L, 40)  # 420 rows
    n = len(codes)
    store = make_store(codes, "nt")
    want_counts = expected_levels(codes, L + 3)[1]
    assert want_counts[0] > want_counts[1] > want_counts[2] > 1 and want_counts[L - 1] >= 1 and want_counts[L] == 1, want_counts
    for bound in (L - 1, L, L + 3):
        edges, ends = store.self_forest(bound)
        check_forest(codes, edges, ends, bound)
        kernels = store.last_call_kernels()
        assert any(k.startswith("smafa::") for k in kernels)  # the classes below L are scanned for
        assert (STAR in kernels) == (bound >= L) and kernels[-1] == (STAR if bound >= L else SF[-1]), kernels
        if bound >= L:
            assert (ends[L:] == n - 1).all() and len(edges) == n - 1
            heavy = edges[edges["dist"] == L]
            assert len(heavy) == want_counts[L - 1] - 1 and (heavy["query"] == 0).all()
            assert ((codes[0][None, :] != codes[heavy["subject"]]).sum(axis=1) == L).all()
        else:
            assert len(edges) == n - want_counts[L - 1]
    # the same with components that DO survive bound L - 1: four groups of rows over two letters each, no letter shared between
    # two groups, so rows of different groups differ in every column; row 0's group apart, three roots are left to hang
    lc = synth.letter_codes(1)
    rng = np.random.default_rng(12)
    apart = np.concatenate([lc[2 * g + rng.integers(0, 2, size=(30, L))] for g in range(4)]).astype(np.uint8)
    rng.shuffle(apart, axis=0)
    apart_counts = expected_levels(apart, L)[1]
    assert apart_counts[L - 1] == 4 and apart_counts[L] == 1 and apart_counts[0] > apart_counts[2] > 4, apart_counts
    other = make_store(apart, "aa")
    edges, ends = other.self_forest(L)
    check_forest(apart, edges, ends, L)
    assert STAR in other.last_call_kernels()
    heavy = edges[edges["dist"] == L]
    assert len(heavy) == 3 and (heavy["query"] == 0).all() and int(ends[L]) == len(apart) - 1 and int(ends[L - 1]) == len(apart) - 4
    assert sorted(heavy["subject"].tolist()) == sorted(set(expected_levels(apart, L)[0][L - 1].tolist()) - {0})
    other.close()
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_forest(None)
    assert e.value.code == _lib.ERR_INVALID
    out = np.zeros(n, dtype=smafa_amd.HIT_DTYPE)
    out["dist"] = 7
    ends = (C.c_uint64 * 3)(9, 9, 9)
    l = _lib.lib()
    assert l.smafa_db_self_forest(store._h, 2, out.ctypes.data, n - 2, ends) == _lib.ERR_INVALID
    assert (" %d rows" % (n - 2)).encode() in l.smafa_last_error() and (out["dist"] == 7).all() and list(ends) == [9, 9, 9]
    assert l.smafa_db_self_forest(store._h, 2, None, n - 1, ends) == _lib.ERR_INVALID
    assert b"NULL edges" in l.smafa_last_error()
    assert l.smafa_db_self_forest(store._h, 2, out.ctypes.data, n - 1, None) == _lib.ERR_INVALID
    assert b"NULL level_ends" in l.smafa_last_error()
    assert l.smafa_db_self_forest(store._h, _lib.NONE, out.ctypes.data, n - 1, ends) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert l.smafa_db_self_forest_launch(store._h, 2, None, None) == _lib.ERR_INVALID
    assert b"NULL edges" in l.smafa_last_error()
    assert l.smafa_db_self_forest_launch(store._h, _lib.NONE, out.ctypes.data, out.ctypes.data) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert (out["dist"] == 7).all() and list(ends) == [9, 9, 9]
    assert l.smafa_db_self_forest(store._h, 2, out.ctypes.data, n - 1, ends) == _lib.OK
    got_ends = np.array(list(ends), dtype=np.uint64)
    check_forest(codes, out[: int(got_ends[-1])], got_ends, 2)
    assert (out["dist"][int(got_ends[-1]):] == 7).all()  # nothing past the edges
    store.close()


def test_a_chunk_that_cannot_fit_fails_as_the_join_does(monkeypatch):
    """the join's own SMAFA_ERR_NOMEM case, 70 000 equal rows: raised from the forest call too (no partial list is spanned),
    and the handle then answers the components call at a bound that needs no list"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    store = make_store(np.zeros((70_000, 60), dtype=np.uint8), "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_forest(2)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    labels, count = store.self_components(60)
    assert count == 1 and not labels.any()
    store.close()


def test_device_form():
    """smafa_db_self_forest_launch on torch buffers — tests/forest_worker.py, a process of its own: torch has to initialise
    HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forest_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "forest device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_against_the_levels_call_at_scale():
    """1M x 60 aa in 10 000 families of 100, D = 5 (the store of tests/test_gpu_levels.py): no brute force here — the prefixes
    connect exactly the rows of the levels call, acyclically, and every edge is at its recomputed distance"""
    D = 5
    codes = synth.related_subjects(10_000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    edges, ends = store.self_forest(D)
    kernels = store.last_call_kernels()
    assert [k for k in kernels if k.startswith("smafa_sf::")] == SF, kernels
    no_foreign_kernels(kernels)
    assert store.last_call_stats()["scans"] >= 1
    labels, counts = store.self_component_levels(D)
    assert ends.tolist() == [n - c for c in counts] and len(set(counts)) >= 3, (ends.tolist(), counts)
    check_shape(codes, edges, ends, D)
    assert sorted_inside_levels(edges)
    for t, row in walk_forest(n, edges, ends):
        assert row.tobytes() == labels[t].tobytes(), t
    print("%d rows: level ends %s" % (n, ends.tolist()))
    store.close()


def parse(text):
    rows = [[int(v) for v in line.split(b"\t")] for line in text.splitlines()]
    assert all(len(r) == 3 for r in rows) and text.endswith(b"\n")
    return as_edges(np.array(rows, dtype=np.uint32).reshape(-1, 3))


def ends_of(edges, D):
    return np.array([(edges["dist"] <= t).sum() for t in range(D + 1)], dtype=np.uint64)


@pytest.mark.parametrize("kind,L,D", [("nt", 60, 5), ("aa", 60, 3)])
def test_cli_forest(tmp_path, kind, L, D):
    codes = planted_store(21, kind, L, 300)
    counts = expected_levels(codes, D)[1]
    assert len(set(counts)) >= 3
    fa, db, packed = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    texts = []
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, "forest", "-d", path, "--max-divergence", str(D)], capture_output=True)
        assert r.returncode == 0, r.stderr
        texts.append(r.stdout)
    out = str(tmp_path / "forest.tsv")
    with open(out, "wb") as f:
        smafa_amd.forest(db, D, out_fd=f.fileno())
    texts.append(open(out, "rb").read())
    for text in texts:  # (two runs need not choose the same edges: each is held to the contract)
        edges = parse(text)
        check_forest(codes, edges, ends_of(edges, D), D)
        assert len(edges) == len(codes) - counts[D] and sorted_inside_levels(edges)
    # an empty DB prints nothing
    empty_db = str(tmp_path / "e.db")
    # (a version-3 file, amino acids: a version-2 file without rows is three bytes, which `smafa` refuses as the reference does)
    smafa_amd.write_db(empty_db, np.zeros((0, L), dtype=np.uint8), smafa_amd.ALPHABET_AA)
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", empty_db, "--max-divergence", "2"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr

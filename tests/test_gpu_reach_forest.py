"""Mutual-reachability forest of a resident store (smafa_db_self_reach_forest / smafa_db_self_reach_forest_launch / `smafa forest
--min-pts`): the edges {a, b, w = max(distance, core[a], core[b])}, ordered by w, whose prefixes [0, level_ends[t]) are acyclic
and connect exactly the graph cut at weight t, for every t = 0 .. D, from one join — and the core distances beside them.

Expected values never come from the code under test (tests/reach_cases.py): cores, weights and partitions are brute force on the
code bytes, and the edges are walked through a plain union-find.  Which of several pairs of equal weight is chosen is free, so no
test compares edge lists byte for byte."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import dense_store
from density_cases import bridged_store
from forest_cases import as_edges, check_forest, sorted_inside_levels
from neighbours_cases import tie_family
from reach_cases import NONE, check_reach_forest, expected_reach
from self_join_cases import SHAPE_STORES, SHAPE_TABLE, SHAPES, planted_store, shape_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel", "smafa_sf::init_forest_kernel"]
MR = ["smafa_mr::tally_keep_kernel", "smafa_mr::core_dist_kernel", "smafa_mr::span_reach_kernel"]
STAR = "smafa_sf::star_roots_kernel"


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


@functools.lru_cache(maxsize=None)
def aa_case():
    """the 20 020-row aa store of tests/test_gpu_forest.py (same seed), D = 5"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == "aa60")
    return planted_store(11 + 2000 + len("aa60"), kind, L, 2000, n_frac), D


def own_kernels(kernels):
    """the call's kernels behind the scans; nothing of another call's namespace among them"""
    own = [k for k in kernels if not k.startswith("smafa::")]
    assert kernels[: len(kernels) - len(own)] and all(k.startswith("smafa::") for k in kernels[: len(kernels) - len(own)]), kernels
    assert not [k for k in own if k.startswith(("smafa_cc::", "smafa_lv::", "smafa_dn::", "smafa_pk::", "smafa_nb::", "smafa_dl::"))], kernels
    assert "smafa_sf::keep_pairs_kernel" not in own and "smafa_sf::span_edges_kernel" not in own, kernels
    return own


@pytest.mark.parametrize("name,families,D,max_subs", SHAPE_STORES)
def test_every_shape_equals_brute_force(name, families, D, max_subs):
    codes, _ = shape_case(name, families, D, max_subs)
    store = make_store(codes, SHAPE_TABLE[name][0])
    for M in (1, 2, 4):
        edges, ends, cores = store.self_reach_forest(D, M)
        print("%s x %d rows, D = %d, M = %d: level ends %s" % (name, len(codes), D, M, ends.tolist()))
        check_reach_forest(codes, edges, ends, cores, D, M)
        assert sorted_inside_levels(edges)
        if M == 1:
            check_forest(codes, edges, ends, D)
        own_kernels(store.last_call_kernels())
    store.close()


def merge_level(labels, rows_a, rows_b):
    return next((t for t in range(len(labels)) if labels[t][rows_a[0]] == labels[t][rows_b[0]]), None)


def test_bridged_families():
    """two families of copies bridged by a chain of single rows: single linkage joins them at level 1, mutual reachability at
    min_pts 4 only where the chain's rows have become core"""
    codes, role = bridged_store(5)
    D, M = 3, 4
    fam = [np.flatnonzero(role == r) for r in (0, 1)]
    single = merge_level(expected_reach(codes, D, 1)[1], *fam)
    reach = merge_level(expected_reach(codes, D, M)[1], *fam)
    assert single == 1 and reach is not None and reach > single, (single, reach)
    store = make_store(codes, "nt")
    edges, ends, cores = store.self_reach_forest(D, M)
    check_reach_forest(codes, edges, ends, cores, D, M)
    # a copy has 31 copies; an outermost chain row a whole family at 1; the rows between them two rows at 1 and two more at 2
    assert (cores[role < 2] == 0).all() and (cores[(role == 2) | (role == 12)] == 1).all() and (cores[(role >= 3) & (role <= 11)] == 2).all()
    assert reach == 2 and int(ends[1]) < int(ends[2]) == len(codes) - 1
    store.close()


@pytest.mark.parametrize("M", [40, 41, 42, 80, 81])
def test_tied_core_distances(M):
    """40 copies and 40 one-column variants: the (M - 1)-th distance lies inside a tie of 40 rows"""
    codes, copies = tie_family()
    store = make_store(codes, "nt")
    edges, ends, cores = store.self_reach_forest(2, M)
    check_reach_forest(codes, edges, ends, cores, 2, M)
    assert (cores[copies] == {40: 0, 41: 1, 42: 1, 80: 1, 81: NONE}[M]).all()
    assert (cores[~copies] == {40: 1, 41: 1, 42: 2, 80: 2, 81: NONE}[M]).all()
    store.close()


@pytest.mark.parametrize("M,keep_max", [(1, None), (1, "0"), (1, "1000000"), (4000, None), (4000, "0"), (4001, None)])
def test_dense_store(M, keep_max, monkeypatch):
    """2 000 copies of one row + 2 000 of a second row at distance 3, bound 3: 8M pairs, every one kept.  M = 1: 3 998 edges of
    weight 0 and one of weight 3.  M = 4 000: a row's 3 999th other row is at 3, so every core and every weight is 3: 3 999 edges in
    the last class.  M = 4 001: every row is sparse, no edge.  The kept list on the normal path, none (SMAFA_DENSITY_KEEP_MAX=0) and
    one below the pair total: one join against E + 1.  The kernels that ran are smafa_sf::init_forest_kernel,
    smafa_mr::tally_keep_kernel, smafa_mr::core_dist_kernel and smafa_mr::span_reach_kernel, in this order, behind the scans and the
    join's two kernels."""
    codes, group = dense_store()
    if keep_max is not None:
        monkeypatch.setenv("SMAFA_DENSITY_KEEP_MAX", keep_max)  # (read when the handle is made)
    store = make_store(codes, "nt")
    edges, ends, cores = store.self_reach_forest(3, M)
    check_reach_forest(codes, edges, ends, cores, 3, M)
    assert ends.tolist() == {1: [3998, 3998, 3998, 3999], 4000: [0, 0, 0, 3999], 4001: [0, 0, 0, 0]}[M]
    assert (cores == {1: 0, 4000: 3, 4001: NONE}[M]).all()
    kernels = store.last_call_kernels()
    own = own_kernels(kernels)
    assert own == HEAD + (MR if M <= 4000 else MR[:2]), kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    assert stats["launches"] >= (8 if M <= 4000 else 5)
    store.close()
    if keep_max is not None:  # the slow path: the first join and one more per class, E = 4
        monkeypatch.delenv("SMAFA_DENSITY_KEEP_MAX")
        normal = make_store(codes, "nt")
        normal.self_reach_forest(3, M)
        assert stats["scans"] >= normal.last_call_stats()["scans"] + 4, (stats, normal.last_call_stats())
        normal.close()


def test_against_the_neighbours_and_density_calls(monkeypatch):
    """20 020 aa rows in blocks of 128 at stride 2: the cores are entry M - 2 of each row's list of self_neighbours(max_num_hits =
    M - 1) where the list is full, NONE where it is short; the partition of every level on its core rows is self_density(t, M)"""
    codes, D = aa_case()
    M, n = 4, len(codes)
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    monkeypatch.setenv("SMAFA_JOIN_STRIDE", "2")
    store = make_store(codes, "aa")
    monkeypatch.delenv("SMAFA_JOIN_BLOCK")
    monkeypatch.delenv("SMAFA_JOIN_STRIDE")
    edges, ends, cores = store.self_reach_forest(D, M)
    assert store.last_call_stats()["scans"] >= n // 128
    check_reach_forest(codes, edges, ends, cores, D, M)
    offsets, _, dists = store.self_neighbours(D, M - 1)
    offsets = offsets.astype(np.int64)
    full = np.diff(offsets) == M - 1
    assert full.any() and (~full).any()
    assert (cores[full] == dists[offsets[:-1][full] + M - 2]).all() and (cores[~full] == NONE).all()
    parent = np.arange(n)
    for t in range(D + 1):
        labels = expected_reach(codes, D, M)[1][t]  # (check_reach_forest held the walked edges to these, byte for byte)
        got, _, counts = store.self_density(t, M)
        core = cores.astype(np.int64) <= t
        assert counts["core"] == int(core.sum()) and core.any()
        assert got[core].tobytes() == labels[core].tobytes(), t
        assert (labels[~core] == parent[~core]).all()
    assert len(set(edges["dist"].tolist())) >= 3
    store.close()


def test_every_engine_one_contract(monkeypatch):
    codes, D = aa_case()
    M = 3

    def check(store):
        edges, ends, cores = store.self_reach_forest(D, M)
        return check_reach_forest(codes, edges, ends, cores, D, M)

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
    store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    for var, value in (("SMAFA_JOIN_STRIDE", "1"), ("SMAFA_JOIN_BLOCK", "4032")):
        monkeypatch.setenv(var, value)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv(var)
        check(store)
        store.close()


def test_edges_and_errors():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    edges, ends, cores = store.self_reach_forest(5, 3)  # no row
    assert len(edges) == 0 and edges.dtype == smafa_amd.HIT_DTYPE and ends.tolist() == [0] * 6 and cores.shape == (0,)
    rng = np.random.default_rng(4)
    first = rng.integers(0, 4, size=(1, L)).astype(np.uint8)
    store.push(first)
    for M, want in ((0, 0), (1, 0), (2, NONE)):  # one row: core 0 where it alone is enough
        edges, ends, cores = store.self_reach_forest(5, M)
        assert len(edges) == 0 and ends.tolist() == [0] * 6 and cores.tolist() == [want], (M, cores)
        assert not [k for k in store.last_call_kernels() if k.startswith("smafa::")], store.last_call_kernels()  # no scan
    edges, ends, cores = store.self_reach_forest(L + 2, 1)
    assert len(edges) == 0 and ends.tolist() == [0] * (L + 3) and cores.tolist() == [0]
    rest = rng.integers(0, 4, size=(299, L)).astype(np.uint8)
    rest[100] = rest[7]
    rest[200] = rest[7]
    rest[200, 5] = (rest[200, 5] + 1) % 4
    store.push(rest)
    codes = np.concatenate([first, rest])
    for M in (0, 1, 2, 3, 4):  # min_pts 0 is taken as 1; at 3 the two copies join at 1, at 4 every row is sparse
        edges, ends, cores = store.self_reach_forest(5, M)
        check_reach_forest(codes, edges, ends, cores, 5, M)
        assert ends.tolist() == {0: [1, 2, 2, 2, 2, 2], 1: [1, 2, 2, 2, 2, 2], 2: [1, 2, 2, 2, 2, 2], 3: [0, 2, 2, 2, 2, 2], 4: [0] * 6}[M]
    store.close()
    # bounds no two rows can exceed: the classes below L held against brute force, the roots left hung under row 0 at weight L
    L = 9
    codes = planted_store(5, "nt", L, 40)  # 420 rows
    n = len(codes)
    store = make_store(codes, "nt")
    for bound in (L - 1, L, L + 3):
        for M in (1, 3):
            edges, ends, cores = store.self_reach_forest(bound, M)
            check_reach_forest(codes, edges, ends, cores, bound, M)
            kernels = store.last_call_kernels()
            assert (STAR in kernels) == (bound >= L) and kernels[-1] == (STAR if bound >= L else MR[-1]), kernels
            if bound >= L:
                assert (ends[L:] == n - 1).all() and len(edges) == n - 1 and (cores <= L).all()
    edges, ends, cores = store.self_reach_forest(L + 1, n + 1)  # fewer rows than min_pts: every row sparse, no edge, no star
    assert len(edges) == 0 and not ends.any() and (cores == NONE).all() and STAR not in store.last_call_kernels()
    check_reach_forest(codes, edges, ends, cores, L + 1, n + 1)
    edges, ends, cores = store.self_reach_forest(L + 1, n)  # exactly min_pts rows: every core is the farthest row's distance
    check_reach_forest(codes, edges, ends, cores, L + 1, n)
    assert len(edges) == n - 1 and STAR in store.last_call_kernels()
    # four groups of rows over two letters each and one row over a ninth letter: it differs from every row in every column, so its
    # core is L at min_pts 2, and four roots are left to hang
    lc = synth.letter_codes(1)
    rng = np.random.default_rng(12)
    apart = np.concatenate([lc[2 * g + rng.integers(0, 2, size=(30, L))] for g in range(4)] + [np.full((1, L), lc[8])]).astype(np.uint8)
    rng.shuffle(apart, axis=0)
    other = make_store(apart, "aa")
    edges, ends, cores = other.self_reach_forest(L, 2)
    counts = check_reach_forest(apart, edges, ends, cores, L, 2)
    lone = int(np.flatnonzero((apart == lc[8]).all(axis=1))[0])
    assert cores[lone] == L and int((cores == L).sum()) == 1 and counts[L - 1] == 5 and counts[L] == 1
    heavy = edges[edges["dist"] == L]
    assert len(heavy) == 4 and (heavy["query"] == 0).all() and STAR in other.last_call_kernels()
    other.close()
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_reach_forest(None, 3)
    assert e.value.code == _lib.ERR_INVALID
    out = np.zeros(n, dtype=smafa_amd.HIT_DTYPE)
    out["dist"] = 7
    ends = (C.c_uint64 * 3)(9, 9, 9)
    kept = np.full(n, 5, dtype=np.uint32)
    l = _lib.lib()
    untouched = lambda: (out["dist"] == 7).all() and list(ends) == [9, 9, 9] and (kept == 5).all()  # noqa: E731
    assert l.smafa_db_self_reach_forest(store._h, 2, 3, out.ctypes.data, n - 2, ends, kept.ctypes.data) == _lib.ERR_INVALID
    assert (" %d rows" % (n - 2)).encode() in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_reach_forest(store._h, 2, 3, None, n - 1, ends, kept.ctypes.data) == _lib.ERR_INVALID
    assert b"smafa_db_self_reach_forest: NULL edges" in l.smafa_last_error()
    assert l.smafa_db_self_reach_forest(store._h, 2, 3, out.ctypes.data, n - 1, None, kept.ctypes.data) == _lib.ERR_INVALID
    assert b"NULL level_ends" in l.smafa_last_error()
    assert l.smafa_db_self_reach_forest(store._h, _lib.NONE, 3, out.ctypes.data, n - 1, ends, kept.ctypes.data) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert l.smafa_db_self_reach_forest_launch(store._h, 2, 3, None, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_reach_forest_launch: NULL edges" in l.smafa_last_error()
    assert l.smafa_db_self_reach_forest_launch(store._h, _lib.NONE, 3, out.ctypes.data, out.ctypes.data, None) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_reach_forest(store._h, 2, 3, out.ctypes.data, n - 1, ends, None) == _lib.OK  # no cores wanted
    got_ends = np.array(list(ends), dtype=np.uint64)
    assert l.smafa_db_self_reach_forest(store._h, 2, 3, out.ctypes.data, n - 1, ends, kept.ctypes.data) == _lib.OK
    assert list(ends) == got_ends.tolist()
    check_reach_forest(codes, out[: int(got_ends[-1])], got_ends, kept, 2, 3)
    assert (out["dist"][int(got_ends[-1]):] == 7).all()  # nothing past the edges
    store.close()


def test_a_chunk_that_cannot_fit_fails_as_the_join_does(monkeypatch):
    """the join's own SMAFA_ERR_NOMEM case, 70 000 equal rows: raised from this call too (no partial list is spanned), and the
    handle then answers the components call at a bound that needs no list"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    store = make_store(np.zeros((70_000, 60), dtype=np.uint8), "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_reach_forest(2, 3)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    labels, count = store.self_components(60)
    assert count == 1 and not labels.any()
    store.close()


def test_device_form():
    """smafa_db_self_reach_forest_launch on torch buffers, with and without d_cores — tests/reach_worker.py, a process of its own:
    torch has to initialise HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reach_worker.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "reach forest device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def parse(text, columns):
    rows = [line.split(b"\t") for line in text.splitlines()]
    assert all(len(r) == columns for r in rows) and (text.endswith(b"\n") or not text)
    return rows


def ends_of(edges, D):
    return np.array([(edges["dist"] <= t).sum() for t in range(D + 1)], dtype=np.uint64)


@pytest.mark.parametrize("kind,L,D", [("nt", 60, 5), ("aa", 60, 3)])
def test_cli_forest_min_pts(tmp_path, kind, L, D):
    codes = planted_store(21, kind, L, 300)
    M = 4
    want_cores, _, counts = expected_reach(codes, D, M)
    assert len(set(counts)) >= 3 and (want_cores == NONE).any()
    fa, db, packed = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    core_text = b"".join(b"%d\t%d\n" % (i, -1 if c == NONE else c) for i, c in enumerate(want_cores.tolist()))
    texts = []
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, "forest", "-d", path, "--max-divergence", str(D), "--min-pts", str(M)], capture_output=True)
        assert r.returncode == 0, r.stderr
        texts.append(r.stdout)
        r = subprocess.run([_lib.CLI_PATH, "forest", "-d", path, "--max-divergence", str(D), "--min-pts", str(M), "--cores"],
                           capture_output=True)
        assert r.returncode == 0 and r.stdout == core_text, r.stderr
    out = str(tmp_path / "forest.tsv")
    with open(out, "wb") as f:
        smafa_amd.reach_forest(db, D, M, out_fd=f.fileno())
    texts.append(open(out, "rb").read())
    with open(out, "wb") as f:
        smafa_amd.reach_forest(db, D, M, cores=True, out_fd=f.fileno())
    assert open(out, "rb").read() == core_text
    for text in texts:  # (two runs need not choose the same edges: each is held to the contract)
        edges = as_edges(np.array([[int(v) for v in r] for r in parse(text, 3)], dtype=np.uint32).reshape(-1, 3))
        check_reach_forest(codes, edges, ends_of(edges, D), np.array(want_cores), D, M)
        assert len(edges) == len(codes) - counts[D] and sorted_inside_levels(edges)
    # an empty DB prints nothing
    empty_db = str(tmp_path / "e.db")
    smafa_amd.write_db(empty_db, np.zeros((0, L), dtype=np.uint8), smafa_amd.ALPHABET_AA)
    for more in ([], ["--cores"]):
        r = subprocess.run([_lib.CLI_PATH, "forest", "-d", empty_db, "--max-divergence", "2", "--min-pts", "3", *more], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"", r.stderr


def test_cli_forest_without_min_pts_is_unchanged(tmp_path):
    """`smafa forest` without --min-pts prints the host form of self_forest — on a store whose forest is unique (its pairs are
    a copy, a chain of two steps and the pair that closes the chain's triangle at a larger distance), byte for byte"""
    L, D = 60, 3
    rng = np.random.default_rng(33)
    codes = rng.integers(0, 4, size=(200, L)).astype(np.uint8)
    codes[150] = codes[40]
    codes[10] = codes[3]
    codes[10, 5] = (codes[10, 5] + 1) % 4
    codes[20] = codes[10]
    codes[20, 9] = (codes[20, 9] + 1) % 4
    store = make_store(codes, "nt")
    edges, ends = store.self_forest(D)
    store.close()
    assert [tuple(e) for e in edges.tolist()] == [(40, 150, 0), (3, 10, 1), (10, 20, 1)]
    check_forest(codes, edges, ends, D)
    fa, db = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    synth.write_fasta(fa, codes, 0)
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db], capture_output=True).returncode == 0
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", str(D)], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"40\t150\t0\n3\t10\t1\n10\t20\t1\n", (r.stdout, r.stderr)

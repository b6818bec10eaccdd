"""Stable clusters of a resident store (smafa_db_self_stable / smafa_db_self_stable_launch / `smafa stable`): one label per
subject, HDBSCAN's selection over the mutual-reachability hierarchy, counted in levels.

Expected values never come from the code under test (tests/stable_cases.py): the levels are brute force on the code bytes, the
selection is the header's definition in plain loops, and every output — labels, joined, the cluster count, the cores — is held
to it byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import dense_store
from reach_cases import NONE, check_reach_forest
from self_join_cases import SHAPE_STORES, SHAPE_TABLE, shape_case
from stable_cases import FIXTURES, check_stable, expected_stable, planted_codes, short_codes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel", "smafa_sf::init_forest_kernel"]
MR = ["smafa_mr::tally_keep_kernel", "smafa_mr::core_dist_kernel", "smafa_mr::span_reach_kernel"]
STAR = "smafa_sf::star_roots_kernel"
ST = ["smafa_st::unite_class_kernel", "smafa_st::snapshot_kernel", "smafa_st::census_kernel", "smafa_st::adopt_kernel",
      "smafa_st::excess_kernel", "smafa_st::choose_kernel", "smafa_st::assign_kernel"]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    if len(codes):
        store.push(codes)
    return store


def call(store, D, M, S):
    return store.self_stable_clusters(D, M, S, joined=True, cores=True)


def same_bytes(a, b):
    return a[1] == b[1] and all(x.tobytes() == y.tobytes() for x, y in zip((a[0],) + a[2:], (b[0],) + b[2:]))


def own_kernels(kernels):
    """the call's kernels behind the scans"""
    own = [k for k in kernels if not k.startswith("smafa::")]
    assert all(k.startswith("smafa::") for k in kernels[: len(kernels) - len(own)]), kernels
    return own


@pytest.mark.parametrize("name,families,D,max_subs", SHAPE_STORES)
def test_every_shape_equals_the_definition(name, families, D, max_subs):
    codes, _ = shape_case(name, families, D, max_subs)
    store = make_store(codes, SHAPE_TABLE[name][0])
    for M in (1, 2, 4):
        for S in (0, 1, 5):
            count = check_stable(codes, call(store, D, M, S), D, M, S)
            print("%s x %d rows, D = %d, M = %d, S = %d: %d clusters" % (name, len(codes), D, M, S, count))
    assert own_kernels(store.last_call_kernels())[-len(ST):] == ST
    store.close()


@pytest.mark.parametrize("case", range(len(FIXTURES)))
def test_fixture_stores(case):
    """the bridged families of the reach tests, the three-column store, a two-word-per-plane store and a nucleotide store with N —
    tests/test_stable_model.py::test_gpu_fixtures_are_not_trivial says what their answers contain"""
    name, make, D, M, S = FIXTURES[case]
    codes = make()
    store = make_store(codes, "aa" if name == "aa" else "nt")
    if name == "ntn":
        assert (codes == 4).any() and store.info().planes == 3
    if name == "aa":
        assert store.info().words_per_plane == 2
    check_stable(codes, call(store, D, M, S), D, M, S)
    store.close()


@pytest.mark.parametrize("M,S,keep_max", [(1, 0, None), (1, 0, "0"), (4000, 5, None), (4000, 5, "0"), (4001, 1, None)])
def test_dense_store(M, S, keep_max, monkeypatch):
    """2 000 copies of one row + 2 000 of a second row at distance 3, bound 3, the kept list on the normal path and none
    (SMAFA_DENSITY_KEEP_MAX=0).  M = 1: two clusters that live three levels (6 000 each) against their union's one (4 000).
    M = 4 000: every core is 3, one cluster at level 3.  M = 4 001: every row is sparse, all noise.  The kernels that ran are the
    reach forest's, then smafa_st::unite_class_kernel, smafa_st::snapshot_kernel, smafa_st::census_kernel,
    smafa_st::adopt_kernel, smafa_st::excess_kernel, smafa_st::choose_kernel and smafa_st::assign_kernel, in this order."""
    codes, group = dense_store()
    if keep_max is not None:
        monkeypatch.setenv("SMAFA_DENSITY_KEEP_MAX", keep_max)  # (read when the handle is made)
    store = make_store(codes, "nt")
    out = call(store, 3, M, S)
    check_stable(codes, out, 3, M, S)
    labels, count, joined, cores = out
    first = [int(np.flatnonzero(group == g)[0]) for g in (0, 1)]
    if M == 1:
        assert count == 2 and (labels == np.where(group == 0, first[0], first[1])).all() and not joined.any()
    elif M == 4000:
        assert count == 1 and not labels.any() and (joined == 3).all() and (cores == 3).all()
    else:
        assert count == 0 and (labels == NONE).all() and (joined == NONE).all() and (cores == NONE).all()
    kernels = store.last_call_kernels()
    assert own_kernels(kernels) == HEAD + (MR if M <= 4000 else MR[:2]) + ST, kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    assert stats["launches"] >= 5 * 4 + 2
    store.close()


@pytest.mark.parametrize("D", [0, 2, 3, 6])
def test_bounds_around_the_sequence_length(D):
    """L = 3: D = 0, L - 1, L and L + 3; above L - 1 nothing more is scanned and the last plane counts D - L + 1 times"""
    codes = short_codes()
    store = make_store(codes, "nt")
    for M, S in ((1, 0), (1, 5), (3, 0), (3, 5), (len(codes), 1), (len(codes) + 1, 1)):
        check_stable(codes, call(store, D, M, S), D, M, S)
        own = own_kernels(store.last_call_kernels())
        assert (STAR in own) == (D >= 3 and M <= len(codes)) and (ST[2] in own) == (D > 0), own
        assert own[-1] == ST[-1] and [k for k in own if k.startswith("smafa_st::")] == [k for k in ST if D > 0 or k != ST[2]]
    store.close()


def test_a_large_bound_costs_no_more_than_the_sequence_length():
    """D = 40 and D = 1000 on an L = 3 store launch what D = L launches: the levels above L are added arithmetically.  At D = 1000
    the one set of the levels from L on has lived 998 levels of 420 rows, more than everything under it can add up to (at most
    420 rows x 3 levels): one cluster, label 0"""
    codes = short_codes()
    store = make_store(codes, "nt")
    call(store, 3, 2, 0)  # (the handle's first join also inverts the order, once)
    check_stable(codes, call(store, 3, 2, 0), 3, 2, 0)
    launches = store.last_call_stats()["launches"]
    check_stable(codes, call(store, 40, 2, 0), 40, 2, 0)
    assert store.last_call_stats()["launches"] == launches
    labels, count, joined, cores = call(store, 1000, 2, 0)
    assert store.last_call_stats()["launches"] == launches
    assert count == 1 and not labels.any() and (joined <= 3).all() and cores.tobytes() == expected_stable(codes, 3, 2, 0)[3].tobytes()
    store.close()


def test_every_engine_the_same_bytes(monkeypatch):
    codes = planted_codes("aa")
    D, M, S = 5, 3, 4
    store = make_store(codes, "aa")
    first = call(store, D, M, S)
    check_stable(codes, first, D, M, S)
    for on in (False, True):
        store.set_prefilter(on)
        assert same_bytes(call(store, D, M, S), first)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        assert same_bytes(call(store, D, M, S), first)
    store.close()
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = make_store(codes, "aa")
    info = store.build_index(D)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    for mode in (1, 0):
        store.set_index(mode)
        before = store.index_info()["probe_launches"]
        assert same_bytes(call(store, D, M, S), first)
        assert (store.index_info()["probe_launches"] > before) == (mode == 1)
    store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    for var, value in (("SMAFA_JOIN_STRIDE", "1"), ("SMAFA_JOIN_BLOCK", "128")):
        monkeypatch.setenv(var, value)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv(var)
        assert same_bytes(call(store, D, M, S), first)
        store.close()


def test_tiny_stores():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    labels, count, joined, cores = call(store, 5, 3, 0)  # no row
    assert count == 0 and labels.shape == joined.shape == cores.shape == (0,) and labels.dtype == np.uint32
    rng = np.random.default_rng(4)
    codes = rng.integers(0, 4, size=(2, L)).astype(np.uint8)
    codes[1] = codes[0]
    codes[1, 7] = (codes[1, 7] + 1) % 4
    store.push(codes[:1])
    for M, S, one in ((0, 0, True), (1, 1, True), (1, 2, False), (2, 0, False), (2, 1, False)):  # one row
        out = call(store, 5, M, S)
        check_stable(codes[:1], out, 5, M, S)
        assert out[1] == (1 if one else 0) and out[0].tolist() == [0 if one else NONE] and out[2].tolist() == [0 if one else NONE]
        assert out[3].tolist() == [0 if M <= 1 else NONE]
        assert not [k for k in store.last_call_kernels() if k.startswith("smafa::")], store.last_call_kernels()  # no scan
    check_stable(codes[:1], call(store, L + 2, 1, 1), L + 2, 1, 1)
    store.push(codes[1:])
    for D in (0, 1, 5):  # two rows, one column apart
        for M, S in ((1, 1), (1, 2), (2, 0), (2, 1), (3, 0)):
            check_stable(codes, call(store, D, M, S), D, M, S)
    assert call(store, 1, 2, 0)[0].tolist() == [0, 0] and call(store, 0, 2, 0)[0].tolist() == [NONE, NONE]
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_stable_clusters(None, 3)
    assert e.value.code == _lib.ERR_INVALID and "bound" in str(e.value)
    store.close()


def test_the_same_call_twice_and_behind_other_calls():
    """one handle: the call twice, then behind a reach forest and a density call, which use the same handle-owned buffers"""
    codes = planted_codes("ntn")
    D, M, S = 5, 3, 0
    store = make_store(codes, "nt")
    first = call(store, D, M, S)
    check_stable(codes, first, D, M, S)
    assert same_bytes(call(store, D, M, S), first)
    edges, ends, cores = store.self_reach_forest(D, M)
    check_reach_forest(codes, edges, ends, cores, D, M)
    assert same_bytes(call(store, D, M, S), first)
    store.self_density(2, 4)
    assert same_bytes(call(store, D, M, S), first)
    other = call(store, 2, 2, 5)  # other parameters in between
    check_stable(codes, other, 2, 2, 5)
    assert same_bytes(call(store, D, M, S), first)
    labels, count = store.self_stable_clusters(D, M, S)  # the optional outputs left out
    assert count == first[1] and labels.tobytes() == first[0].tobytes()
    store.close()


def test_a_chunk_that_cannot_fit_fails_as_the_join_does(monkeypatch):
    """the join's own SMAFA_ERR_NOMEM case, 70 000 equal rows: raised from this call too, and the handle stays usable"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    store = make_store(np.zeros((70_000, 60), dtype=np.uint8), "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_stable_clusters(2, 3)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    labels, count = store.self_components(60)
    assert count == 1 and not labels.any()
    store.close()


def test_a_refused_call_writes_nothing():
    codes = short_codes()
    n = len(codes)
    store = make_store(codes, "nt")
    l = _lib.lib()
    labels, joined, cores = (np.full(n, 5, dtype=np.uint32) for _ in range(3))
    count = C.c_uint64(9)
    untouched = lambda: (labels == 5).all() and (joined == 5).all() and (cores == 5).all() and count.value == 9  # noqa: E731
    args = (labels.ctypes.data, joined.ctypes.data, cores.ctypes.data)
    assert l.smafa_db_self_stable(store._h, 2, 3, 0, *args, n - 1, C.byref(count)) == _lib.ERR_INVALID
    assert (b"labels holds %d entries" % (n - 1)) in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_stable(store._h, _lib.NONE, 3, 0, *args, n, C.byref(count)) == _lib.ERR_INVALID
    assert b"smafa_db_self_stable: stable clusters need a bound (max_div)" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_stable(store._h, 2, 3, 0, None, args[1], args[2], n, C.byref(count)) == _lib.ERR_INVALID
    assert b"smafa_db_self_stable: NULL labels" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_stable(store._h, 2, 3, 0, *args, n, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_stable: NULL n_clusters" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_stable(store._h, 2, 3, 0, args[0], None, None, n, C.byref(count)) == _lib.OK  # the optional ones left out
    assert (joined == 5).all() and (cores == 5).all() and count.value == expected_stable(codes, 2, 3, 0)[2]
    assert labels.tobytes() == expected_stable(codes, 2, 3, 0)[0].tobytes()
    store.close()


def test_argument_checks_in_order():
    """handle, labels, n_clusters, bound, capacity: with several arguments wrong the first of these is the one named"""
    codes = short_codes()
    n = len(codes)
    store = make_store(codes, "nt")
    l = _lib.lib()
    labels = np.full(n, 5, dtype=np.uint32)
    count = C.c_uint64(9)
    for form, tail in ((l.smafa_db_self_stable, (0,)), (l.smafa_db_self_stable_launch, ())):
        who = b"smafa_db_self_stable" + (b"" if tail else b"_launch")
        assert form(store._h, _lib.NONE, 3, 0, None, None, None, *tail, None) == _lib.ERR_INVALID
        assert who + b": NULL labels" in l.smafa_last_error()
        assert form(store._h, _lib.NONE, 3, 0, labels.ctypes.data, None, None, *tail, None) == _lib.ERR_INVALID
        assert who + b": NULL n_clusters" in l.smafa_last_error()
        assert form(store._h, _lib.NONE, 3, 0, labels.ctypes.data, None, None, *tail, C.byref(count)) == _lib.ERR_INVALID
        assert who + b": stable clusters need a bound (max_div)" in l.smafa_last_error()
    assert l.smafa_db_self_stable(store._h, 2, 3, 0, labels.ctypes.data, None, None, 0, C.byref(count)) == _lib.ERR_INVALID
    assert b"smafa_db_self_stable: labels holds 0 entries, the store has %d subjects" % n in l.smafa_last_error()
    assert (labels == 5).all() and count.value == 9
    store.close()


def test_device_form():
    """smafa_db_self_stable_launch on torch buffers, with and without d_joined and d_cores — tests/stable_worker.py, a process of
    its own: torch has to initialise HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stable_worker.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "stable clusters device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.parametrize("kind,D,M,S", [("ntn", 5, 2, 0), ("aa", 5, 4, 3)])
def test_cli_stable(tmp_path, kind, D, M, S):
    codes = planted_codes(kind)
    want, want_joined, count, _ = expected_stable(codes, D, M, S)
    assert count > 1 and (want == NONE).any()
    fa, db, packed = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", "aa" if kind == "aa" else "nt"]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    show = lambda v: -1 if v == NONE else v  # noqa: E731
    plain = b"".join(b"%d\t%d\n" % (i, show(v)) for i, v in enumerate(want.tolist()))
    with_joined = b"".join(b"%d\t%d\t%d\n" % (i, show(v), show(j)) for i, (v, j) in enumerate(zip(want.tolist(), want_joined.tolist())))
    size = ["--min-cluster-size", str(S)] if S else []
    for path in (db, packed):
        base = [_lib.CLI_PATH, "stable", "-d", path, "--max-divergence", str(D), "--min-pts", str(M), *size]
        r = subprocess.run(base, capture_output=True)
        assert r.returncode == 0 and r.stdout == plain, r.stderr
        assert (b"%d stable clusters among %d sequences" % (count, len(codes))) in r.stderr, r.stderr
        r = subprocess.run(base + ["--joined"], capture_output=True)
        assert r.returncode == 0 and r.stdout == with_joined, r.stderr
    out = str(tmp_path / "stable.tsv")
    with open(out, "wb") as f:
        smafa_amd.stable_clusters(db, D, M, S, joined=True, out_fd=f.fileno())
    assert open(out, "rb").read() == with_joined
    empty_db = str(tmp_path / "e.db")
    smafa_amd.write_db(empty_db, np.zeros((0, 60), dtype=np.uint8), smafa_amd.ALPHABET_AA)
    r = subprocess.run([_lib.CLI_PATH, "stable", "-d", empty_db, "--max-divergence", "2", "--min-pts", "3", "--joined"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr


def test_cli_forest_min_pts_is_unchanged(tmp_path):
    """`smafa forest --min-pts` prints what it printed: three rows with a-b at 1, b-c at 3, a-c at 4; at min_pts 2 the cores are
    1, 1, 3 and the forest is unique"""
    fa, db = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGT\n>b\nACGTACGA\n>c\nTTTTACGA\n")
    smafa_amd.makedb(fa, db)
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "4", "--min-pts", "2"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"0\t1\t1\n1\t2\t3\n", r.stderr
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "2", "--min-pts", "2", "--cores"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"0\t1\n1\t1\n2\t-1\n", r.stderr
    # and `stable` on the same rows: the pair is a cluster from level 1 on, and the third row, core at 3, joins it there (one big
    # child: the cluster continues)
    r = subprocess.run([_lib.CLI_PATH, "stable", "-d", db, "--max-divergence", "4", "--min-pts", "2", "--joined"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"0\t0\t1\n1\t0\t1\n2\t0\t3\n", r.stderr
    r = subprocess.run([_lib.CLI_PATH, "stable", "-d", db, "--max-divergence", "2", "--min-pts", "2", "--joined"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"0\t0\t1\n1\t0\t1\n2\t-1\t-1\n", r.stderr

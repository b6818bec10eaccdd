"""Density clusters of a resident store (smafa_db_self_density / smafa_db_self_density_launch / `smafa density`): DBSCAN
over the store's own rows with eps = the bound — degrees[i] = the number of other subjects within the bound of i, core iff
degrees[i] + 1 >= min_pts, labels = the smallest core number of a core row's cluster, the label of its smallest core
neighbour for a border row, NONE for noise.

Expected answers never come from the code under test: tests/density_cases.py works from brute-force pairs on the code bytes.
At 1M rows, where brute force is out of reach, the answer is held against its properties, the components call and a
sub-sample of whole components that is stored alone and compared with brute force.
The file takes 10.2 s on an MI355X (3.7 s of it the device form's worker process, 2.8 s the two CLI cases, 1.5 s the 1M-row
case, which therefore stays at 10 000 families)."""
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
from density_cases import NONE, bridged_store, brute_density, density_from_pairs, kinds
from self_join_cases import SHAPES, brute_pairs, planted_store

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_PTS = (1, 3, 11, 12)  # (11: the one value at which the wide shape, whose families are all within its bound, has every kind of row)
DN = ["smafa_dn::init_density_kernel", "smafa_dn::count_keep_kernel", "smafa_dn::link_cores_kernel",
      "smafa_dn::flatten_density_kernel"]


@functools.lru_cache(maxsize=None)
def case(name, families):
    """-> (codes, {min_pts: (labels, degrees, counts)}, D, number of pairs) of a shape of SHAPES at `families` x 10 + 20
    rows, the stores of tests/test_gpu_self_join.py (same seeds)"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    codes = planted_store(11 + families + len(name), kind, L, families, n_frac)
    pairs = brute_pairs(codes, D)
    want = {m: density_from_pairs(len(codes), pairs, m) for m in MIN_PTS}
    return codes, want, D, len(pairs)


def kind_of(name):
    return next(s for s in SHAPES if s[0] == name)[1]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def check(got, want, degrees=True):
    labels, degs, counts = got
    assert labels.dtype == np.uint32 and labels.shape == want[0].shape
    assert labels.tobytes() == want[0].tobytes()
    if degrees:
        assert degs.dtype == np.uint32 and degs.tobytes() == want[1].tobytes()
    else:
        assert degs is None
    assert counts == want[2], (counts, want[2])


@pytest.mark.parametrize("name,families", [(s[0], 300) for s in SHAPES] + [("aa60", 2000)])
def test_density_equals_brute_force(name, families):
    codes, want, D, _ = case(name, families)
    # the planted copies separate core from non-core rows: for some min_pts the expected answer has every kind of row.  (At
    # bound 0 a border row cannot exist — equal rows have equal degrees — so the copies-only shape has core and noise rows.
    # A family of 10 has degrees up to 9 and a planted copy adds one: min_pts 11 asks for a copy, 12 for two.)
    present = [tuple(bool(k.any()) for k in kinds(want[m][0], want[m][1], m)) for m in MIN_PTS]
    assert ((True, True, True) in present) if D > 0 else ((True, False, True) in present), (name, present)
    store = make_store(codes, kind_of(name))
    for m in MIN_PTS:
        got = store.self_density(D, m)
        print("%s x %d rows, D = %d, min_pts = %d: %s, kernels %s" % (name, len(codes), D, m, got[2], store.last_call_kernels()))
        check(got, want[m])
    check(store.self_density(D, 3, degrees=False), want[3], degrees=False)
    store.close()


@pytest.mark.parametrize("name", ["nt60", "aa60"])
def test_min_pts_one_is_the_components_call(name):
    """min_pts = 1 (and 0) is, bytes and count, self_components(D) — with degrees (counted, then linked) and without (linked
    directly, no count kernel) — and the degrees add up to twice the join's pair count"""
    codes, want, D, _ = case(name, 300)
    store = make_store(codes, kind_of(name))
    row, count = store.self_components(D)
    for min_pts in (1, 0):
        labels, degrees, counts = store.self_density(D, min_pts)
        assert labels.tobytes() == row.tobytes() and counts == {"clusters": count, "core": len(codes), "noise": 0}
    assert "smafa_dn::count_keep_kernel" in store.last_call_kernels()
    pair_count = (C.c_uint64 * 1)()
    # (the host form with no room counts only: SMAFA_ERR_CAPACITY and the exact number of pairs)
    assert _lib.lib().smafa_db_self_hits(store._h, D, None, 0, pair_count) in (_lib.OK, _lib.ERR_CAPACITY)
    assert int(degrees.astype(np.int64).sum()) == 2 * int(pair_count[0]) and pair_count[0] > 0
    labels, none, counts = store.self_density(D, 1, degrees=False)
    assert none is None and labels.tobytes() == row.tobytes() and counts["clusters"] == count
    kernels = store.last_call_kernels()
    assert "smafa_dn::count_keep_kernel" not in kernels and "smafa_join::inverse_order_kernel" not in kernels, kernels
    assert [k for k in kernels if k.startswith("smafa_dn::")] == [DN[0], DN[2], DN[3]], kernels
    assert not [k for k in kernels if k.startswith(("smafa_cc::", "smafa_lv::"))], kernels
    store.close()


def test_bridged_families():
    """two families bridged by a chain of single rows: ONE component at bound 1, two clusters at min_pts 4"""
    codes, role = bridged_store(5)
    want = brute_density(codes, 1, 4)
    store = make_store(codes, "nt")
    row, count = store.self_components(1)
    assert count == 1 and not row.any()
    got = store.self_density(1, 4)
    check(got, want)
    labels, degrees, counts = got
    core, border, noise = kinds(labels, degrees, 4)
    assert counts == {"clusters": 2, "core": 66, "noise": 7} and int(border.sum()) == 2
    assert set(role[border].tolist()) == {3, 11} and set(role[noise].tolist()) == set(range(4, 11))
    assert len(set(labels[role == 0].tolist())) == 1 and labels[role == 0][0] != labels[role == 1][0]
    store.close()


def test_one_join_against_two_joins(monkeypatch):
    """the kept pair list: unset (every pair kept: one join, smafa_dn::link_cores_kernel once over the list), 0 (nothing
    kept: the store is joined twice) and a capacity below the pair count (the list overflows: degrees still exact, joined
    twice) give the same bytes"""
    codes, want, D, pairs = case("nt60", 300)
    assert pairs > 2000
    scans = {}
    for knob in (None, "0", str(pairs // 2)):
        if knob is None:
            monkeypatch.delenv("SMAFA_DENSITY_KEEP_MAX", raising=False)
        else:
            monkeypatch.setenv("SMAFA_DENSITY_KEEP_MAX", knob)  # (read when the handle is made)
        store = make_store(codes, "nt")
        monkeypatch.delenv("SMAFA_DENSITY_KEEP_MAX", raising=False)
        for m in MIN_PTS:
            check(store.self_density(D, m), want[m])
            kernels = store.last_call_kernels()
            assert "smafa_dn::link_cores_kernel" in kernels and [k for k in kernels if k.startswith("smafa_dn::")] == DN, kernels
            scans.setdefault(knob, []).append(store.last_call_stats()["scans"])
        store.close()
    print("scans per call: %s" % scans)
    assert len(set(scans[None])) == 1 and scans[None][0] >= 1
    assert scans["0"] == [2 * s for s in scans[None]] and scans[str(pairs // 2)] == scans["0"], scans


@pytest.mark.parametrize("ceiling", [None, "1000000"])
def test_dense_store(ceiling, monkeypatch):
    """2 000 copies of one row + 2 000 of a second row at distance 3: two hot degree[] neighbourhoods of 2 000 rows, 16M rows in
    the one block's list at bound 3 (four times the scratch list: scanned again; under the ceiling: cut instead, and the kept list,
    whose default capacity is that ceiling, overflows: joined twice).  Kernels: the scans, smafa_join::store_records_kernel,
    smafa_join::inverse_order_kernel, then smafa_dn::init_density_kernel, smafa_dn::count_keep_kernel,
    smafa_dn::link_cores_kernel, smafa_dn::flatten_density_kernel."""
    codes, group = dense_store()
    first = [int(np.flatnonzero(group == g)[0]) for g in (0, 1)]
    assert min(first) == 0
    two = np.array(first, dtype=np.uint32)[group]
    if ceiling:
        monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", ceiling)
    store = make_store(codes, "nt")
    labels, degrees, counts = store.self_density(2, 100)
    assert (degrees == 1999).all() and counts == {"clusters": 2, "core": 4000, "noise": 0}
    assert labels.tobytes() == two.tobytes()
    kernels = store.last_call_kernels()
    assert not [k for k in kernels if k.startswith(("smafa_cc::", "smafa_lv::"))] and "smafa_join::join_filter_kernel" not in kernels
    assert kernels[-6:] == ["smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel"] + DN, kernels
    assert kernels[0].startswith("smafa::") and all(k.startswith("smafa::") for k in kernels[:-6]), kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 6 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    if ceiling:  # 8M rows in the one block's list, which may not grow: the piece is cut, and the 4M pairs overflow a kept list
        # of 1M: the store is joined twice, piece for piece as the components call on this handle joins it once
        store.self_components(2)
        once = store.last_call_stats()["scans"]
        assert once > 2 and stats["scans"] == 2 * once, (stats, once)
    labels, degrees, counts = store.self_density(3, 4000)
    assert (degrees == 3999).all() and counts == {"clusters": 1, "core": 4000, "noise": 0} and not labels.any()
    kernels = store.last_call_kernels()
    assert kernels[-5:] == ["smafa_join::store_records_kernel"] + DN, kernels  # (the inverse order map is current)
    labels, degrees, counts = store.self_density(3, 4001)
    assert (degrees == 3999).all() and counts == {"clusters": 0, "core": 0, "noise": 4000} and (labels == NONE).all()
    kernels = store.last_call_kernels()
    assert "smafa_dn::link_cores_kernel" not in kernels and kernels[-3:] == [DN[0], DN[1], DN[3]], kernels
    store.close()


def test_every_engine_one_answer(monkeypatch):
    name, m = "aa60", 3
    codes, want, D, _ = case(name, 2000)
    want = want[m]
    store = make_store(codes, "aa")
    check(store.self_density(D, m), want)
    assert store.last_call_kernels()[0].startswith("smafa::scan_"), store.last_call_kernels()
    for on in (False, True):
        store.set_prefilter(on)
        check(store.self_density(D, m), want)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        check(store.self_density(D, m), want)
        if level == 2:
            assert any("scan_zone_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()
    store.close()
    # a current block index answers the blocks (limits lifted as tests/test_gpu_levels.py lifts them); modes 2 and 3 may
    # build one on the way
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = make_store(codes, "aa")
    info = store.build_index(D)
    store.set_index(1)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    before = store.index_info()["probe_launches"]
    check(store.self_density(D, m), want)
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    store.close()
    for mode in (2, 3):
        store = make_store(codes, "aa")
        store.set_index(mode)
        check(store.self_density(D, m), want)
        check(store.self_density(D, m), want)
        store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    # many pieces, with mirror images across pieces (and, with the index, repeats): every pair still counts exactly once
    for var, value in (("SMAFA_JOIN_STRIDE", "1"), ("SMAFA_JOIN_BLOCK", "128")):
        monkeypatch.setenv(var, value)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv(var)
        check(store.self_density(D, m), want)
        if var == "SMAFA_JOIN_BLOCK":  # 20 020 rows in blocks of 128
            assert store.last_call_stats()["scans"] >= 20020 // 128, store.last_call_stats()
        store.close()


def test_edges_and_errors():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    labels, degrees, counts = store.self_density(5, 3)
    assert labels.shape == (0,) and degrees.shape == (0,) and counts == {"clusters": 0, "core": 0, "noise": 0}
    rng = np.random.default_rng(4)
    first = rng.integers(0, 4, size=(1, L)).astype(np.uint8)
    store.push(first)
    labels, degrees, counts = store.self_density(5, 1)
    assert labels.tolist() == [0] and degrees.tolist() == [0] and counts == {"clusters": 1, "core": 1, "noise": 0}
    assert not [k for k in store.last_call_kernels() if k.startswith("smafa::")], store.last_call_kernels()  # no scan
    labels, degrees, counts = store.self_density(5, 2)
    assert labels.tolist() == [NONE] and degrees.tolist() == [0] and counts == {"clusters": 0, "core": 0, "noise": 1}
    store.close()
    # bounds no two rows can exceed: no scan; every degree is n - 1, one cluster if n >= min_pts, else all noise
    L = 9
    codes = planted_store(5, "nt", L, 40)
    n = len(codes)
    store = make_store(codes, "nt")
    for bound in (L, L + 3):
        for min_pts, all_core in ((0, True), (5, True), (n, True), (n + 1, False)):
            labels, degrees, counts = store.self_density(bound, min_pts)
            assert not [k for k in store.last_call_kernels() if k.startswith(("smafa::", "smafa_join::"))], store.last_call_kernels()
            assert (degrees == n - 1).all()
            if all_core:
                assert not labels.any() and counts == {"clusters": 1, "core": n, "noise": 0}
            else:
                assert (labels == NONE).all() and counts == {"clusters": 0, "core": 0, "noise": n}
            check((labels, degrees, counts), brute_density(codes, bound, min_pts))
    check(store.self_density(L - 1, 5), brute_density(codes, L - 1, 5))
    assert any(k.startswith("smafa::") for k in store.last_call_kernels())
    check(store.self_density(2, n + 1), brute_density(codes, 2, n + 1))  # min_pts > n: all noise
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_density(None, 3)
    assert e.value.code == _lib.ERR_INVALID
    want = brute_density(codes, 2, 3)
    out, deg = np.full(n, 7, dtype=np.uint32), np.full(n, 7, dtype=np.uint32)
    counts = (C.c_uint64 * 3)(9, 9, 9)
    l = _lib.lib()
    assert l.smafa_db_self_density(store._h, 2, 3, out.ctypes.data, deg.ctypes.data, n - 1, counts) == _lib.ERR_INVALID
    assert str(n - 1).encode() in l.smafa_last_error() and (out == 7).all() and (deg == 7).all() and list(counts) == [9, 9, 9]
    assert l.smafa_db_self_density(store._h, 2, 3, None, deg.ctypes.data, n, counts) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error()
    assert l.smafa_db_self_density(store._h, 2, 3, out.ctypes.data, deg.ctypes.data, n, None) == _lib.ERR_INVALID
    assert b"NULL counts" in l.smafa_last_error()
    assert l.smafa_db_self_density(store._h, _lib.NONE, 3, out.ctypes.data, deg.ctypes.data, n, counts) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert l.smafa_db_self_density_launch(store._h, 2, 3, None, None, None) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error()
    assert (out == 7).all() and (deg == 7).all() and list(counts) == [9, 9, 9]
    assert l.smafa_db_self_density(store._h, 2, 3, out.ctypes.data, None, n, counts) == _lib.OK  # degrees = NULL is accepted
    assert out.tobytes() == want[0].tobytes() and (deg == 7).all()
    assert list(counts) == [want[2]["clusters"], want[2]["core"], want[2]["noise"]]
    assert l.smafa_db_self_density(store._h, 2, 3, out.ctypes.data, deg.ctypes.data, n, counts) == _lib.OK
    assert deg.tobytes() == want[1].tobytes()
    store.close()


def test_a_chunk_that_cannot_fit_fails_as_the_join_does(monkeypatch):
    """the join's own SMAFA_ERR_NOMEM case, 70 000 equal rows: raised from the density call too (nothing is counted from a
    partial list), and the handle then answers at a bound that needs no list"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    store = make_store(np.zeros((70_000, 60), dtype=np.uint8), "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_density(2, 3)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    labels, degrees, counts = store.self_density(60, 3)
    assert counts == {"clusters": 1, "core": 70_000, "noise": 0} and not labels.any() and (degrees == 69_999).all()
    store.close()


def test_device_form():
    """smafa_db_self_density_launch on torch buffers — tests/density_worker.py, a process of its own: torch has to initialise
    HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "density_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "density device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_properties_at_scale():
    """1M x 60 aa in 10 000 families of 100, D = 5 (the store of tests/test_gpu_levels.py's scale case)"""
    D = 5
    codes = synth.related_subjects(10_000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    row, count = store.self_components(D)
    labels, degrees, counts = store.self_density(D, 1)
    assert labels.tobytes() == row.tobytes() and counts == {"clusters": count, "core": n, "noise": 0}
    assert [k for k in store.last_call_kernels() if k.startswith("smafa_dn::")] == DN
    m = 20
    dense_labels, dense_degrees, dense_counts = store.self_density(D, m)
    print("%d rows, D = %d: %d components; min_pts %d: %s; %s" % (n, D, count, m, dense_counts, store.last_call_stats()))
    assert dense_degrees.tobytes() == degrees.tobytes()
    core, border, noise = kinds(dense_labels, dense_degrees, m)
    assert dense_counts["core"] == int(core.sum()) and dense_counts["noise"] == int(noise.sum())
    assert 0 < dense_counts["clusters"] <= dense_counts["core"] < n and dense_counts["noise"] > 0 and border.any()
    reps = core & (dense_labels == np.arange(n))
    assert dense_counts["clusters"] == int(reps.sum())
    assert (dense_labels[dense_labels[core]] == dense_labels[core]).all() and (dense_labels[core] <= np.flatnonzero(core)).all()
    assert core[dense_labels[~noise]].all()  # every non-noise label is a core row
    assert (row[dense_labels[~noise]] == row[~noise]).all()  # ... of the row's own single-linkage component
    # whole components of about 2 000 rows in all, stored alone: the same degrees, and brute force agrees
    comps, sizes = np.unique(row, return_counts=True)
    pick = np.isin(row, comps[: int(np.searchsorted(np.cumsum(sizes), 2000))])
    sub = np.ascontiguousarray(codes[pick])
    assert 1000 <= len(sub) <= 2000
    small = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    small.push(sub)
    pairs = small.self_pairs(D)
    from_pairs = np.bincount(pairs["query"], minlength=len(sub)) + np.bincount(pairs["subject"], minlength=len(sub))
    want = brute_density(sub, D, m)
    assert from_pairs.tolist() == want[1].tolist() and degrees[pick].tolist() == want[1].tolist()
    check(small.self_density(D, m), want)
    small.close()
    store.close()


@pytest.mark.parametrize("kind,L,D", [("nt", 60, 5), ("aa", 60, 3)])
def test_cli_density(tmp_path, kind, L, D):
    codes = planted_store(21, kind, L, 300)
    n, m = len(codes), 3
    labels, degrees, counts = brute_density(codes, D, m)
    assert counts["noise"] > 0 and counts["clusters"] > 1
    text = "".join("%d\t%d\t%d\n" % (i, -1 if labels[i] == NONE else labels[i], degrees[i]) for i in range(n)).encode()
    assert b"\t-1\t" in text
    fa, db, packed = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, "density", "-d", path, "--max-divergence", str(D), "--min-pts", str(m)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == text, path
    out = str(tmp_path / "density.tsv")
    with open(out, "wb") as f:
        smafa_amd.density(db, D, m, out_fd=f.fileno())
    assert open(out, "rb").read() == text
    # an empty DB prints nothing
    empty_db = str(tmp_path / "e.db")
    # (a version-3 file, amino acids: a version-2 file without rows is three bytes, which `smafa` refuses as the reference does)
    smafa_amd.write_db(empty_db, np.zeros((0, L), dtype=np.uint8), smafa_amd.ALPHABET_AA)
    r = subprocess.run([_lib.CLI_PATH, "density", "-d", empty_db, "--max-divergence", "2", "--min-pts", "3"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr

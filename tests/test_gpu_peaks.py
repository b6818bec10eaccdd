"""Abundance-peak clusters of a resident store (smafa_db_self_peaks / smafa_db_self_peaks_launch / `smafa peaks`): weights[i]
= 1 + the number of other subjects within the radius of i, parents[i] = the subject of greatest (weight, smaller number)
among i and the subjects within the bound of it, labels[i] = the peak (parents[p] == p) reached from i along the parents.

Expected answers never come from the code under test: tests/peaks_cases.py works from brute-force pairs on the code bytes.
At 1M rows, where brute force is out of reach, the answer is held against its properties, the components call and a
sub-sample of whole components that is stored alone and compared with brute force.
The file takes 9.8 s on an MI355X (3.7 s of it the device form's worker process, 2.6 s the two CLI cases, 1.3 s the 1M-row
case, 0.9 s the engines' case)."""
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
from peaks_cases import brute_peaks, climb_chain, keys_of, moved_and_multi_step, peaks_from_pairs, valley_store
from self_join_cases import SHAPES, brute_pairs, planted_store

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PK = ["smafa_pk::init_peaks_kernel", "smafa_pk::weigh_keep_kernel", "smafa_pk::climb_kernel", "smafa_pk::crown_kernel",
      "smafa_pk::settle_kernel", "smafa_pk::jump_kernel"]
CLIMBED = [PK[0], PK[1], PK[2], PK[4], PK[5]]  # a call with pairs: everything but the crown


@functools.lru_cache(maxsize=None)
def case(name, families):
    """-> (codes, {radius: (labels, parents, weights, n_peaks)} for r = 0 and r = D, D, number of pairs) of a shape of SHAPES
    at `families` x 10 + 20 rows, the stores of tests/test_gpu_self_join.py and tests/test_gpu_density.py (same seeds)"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    codes = planted_store(11 + families + len(name), kind, L, families, n_frac)
    pairs = brute_pairs(codes, D)
    want = {r: peaks_from_pairs(len(codes), pairs, r) for r in {0, D}}
    return codes, want, D, len(pairs)


def kind_of(name):
    return next(s for s in SHAPES if s[0] == name)[1]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def check(got, want, parents=True, weights=True):
    labels, par, wts, n_peaks = got
    assert labels.dtype == np.uint32 and labels.shape == want[0].shape
    assert labels.tobytes() == want[0].tobytes()
    if parents:
        assert par.dtype == np.uint32 and par.tobytes() == want[1].tobytes()
    else:
        assert par is None
    if weights:
        assert wts.dtype == np.uint32 and wts.tobytes() == want[2].tobytes()
    else:
        assert wts is None
    assert n_peaks == want[3], (n_peaks, want[3])


def pk_kernels(store):
    return [k for k in store.last_call_kernels() if k.startswith("smafa_pk::")]


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_peaks_equal_brute_force(name):
    codes, want, D, _ = case(name, 300)
    # the expected answer exercises the climb: rows that moved, and (copies alone cannot chain) rows more than one step
    # from their peak, at r = 0 or r = D
    moved = [moved_and_multi_step(want[r]) for r in sorted(want)]
    assert any(m[0] > 0 for m in moved) and (name == "aa60d0" or any(m[1] > 0 for m in moved)), (name, moved)
    store = make_store(codes, kind_of(name))
    for r in sorted(want):
        for parents, weights in ((True, True), (False, False), (True, False), (False, True)):
            got = store.self_peaks(D, r, parents=parents, weights=weights)
            check(got, want[r], parents, weights)
        print("%s x %d rows, D = %d, r = %d: %d peaks, moved / multi-step %s, kernels %s, %s" % (
            name, len(codes), D, r, want[r][3], moved_and_multi_step(want[r]), pk_kernels(store), store.last_call_stats()))
        assert pk_kernels(store) == CLIMBED
    check(store.self_peaks(D, None), want[D])  # radius None (SMAFA_NONE): r = D
    store.close()


@pytest.mark.parametrize("name", ["nt60", "aa60", "nt9"])
def test_weights_are_the_density_degrees(name):
    codes, want, D, _ = case(name, 300)
    store = make_store(codes, kind_of(name))
    _, degrees, _ = store.self_density(D, 1)
    _, _, weights, _ = store.self_peaks(D, D)
    assert weights.tobytes() == (degrees + 1).astype(np.uint32).tobytes() and int(degrees.sum()) > 0
    _, copies, _ = store.self_density(0, 1)
    _, _, weights, _ = store.self_peaks(D, 0)
    assert weights.tobytes() == (copies + 1).astype(np.uint32).tobytes() and int(copies.sum()) > 0
    store.close()


def test_valley_store():
    """one component, one density cluster, two peaks"""
    for seed in (0, 3):
        codes, group = valley_store(seed)
        store = make_store(codes, "nt")
        row, count = store.self_components(1)
        assert count == 1 and not row.any()
        assert store.self_density(1, 4)[2] == {"clusters": 1, "core": len(codes), "noise": 0}
        for r in (0, 1):
            want = brute_peaks(codes, 1, r)
            got = store.self_peaks(1, r)
            check(got, want)
            assert got[3] == 2 and len(set(got[0].tolist())) == 2
            assert len(set(got[0][group <= 2].tolist())) == 1 and len(set(got[0][group >= 4].tolist())) == 1
        store.close()


def test_bridged_families():
    codes, role = bridged_store(5)
    want = brute_peaks(codes, 1, 0)
    assert want[3] == 5
    store = make_store(codes, "nt")
    got = store.self_peaks(1, 0)
    check(got, want)
    labels, parents, weights, n_peaks = got
    first = [int(np.flatnonzero(role == f)[0]) for f in (0, 1)]
    assert (labels[role == 0] == first[0]).all() and (labels[role == 1] == first[1]).all() and first[0] != first[1]
    peaks = np.flatnonzero(parents == np.arange(len(codes)))
    light = [p for p in peaks if weights[p] == 1]
    assert light and all(role[p] >= 2 for p in light)
    store.close()


def test_climb_chain():
    """899 rows, each the parent of the next: smafa_pk::jump_kernel flattens the chain by pointer doubling, in more than one
    round — no thread walks it"""
    codes = climb_chain()
    want = brute_peaks(codes, 1, 0)
    store = make_store(codes, "nt")
    got = store.self_peaks(1, 0)
    check(got, want)
    assert not got[0].any() and got[3] == 1
    assert "smafa_pk::jump_kernel" in store.last_call_kernels() and pk_kernels(store) == CLIMBED
    check(store.self_peaks(1, 0), want)  # once more: the inverse order map is current now and costs no launch
    assert "smafa_join::inverse_order_kernel" not in store.last_call_kernels()
    launches = store.last_call_stats()["launches"]
    store.self_components(1)  # the same join, and three launches of its own: init, link, flatten (+ the records and scans)
    shared = store.last_call_stats()["launches"] - 3
    # init x 2, weigh/keep, climb and settle are 5 launches on top of the shared ones; the rest are jump rounds
    rounds = launches - shared - 5
    print("climb_chain: %d launches, %d of them jump rounds" % (launches, rounds))
    assert 2 <= rounds <= 11, (launches, shared)
    store.close()


def test_one_join_against_two_joins(monkeypatch):
    """the kept pair list: unset (every pair kept: one join, smafa_pk::climb_kernel once over the list), 0 (nothing kept:
    the store is joined twice) and a capacity below the pair count (the list overflows: weights still exact, joined twice)
    give the same bytes"""
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
        for r in sorted(want):
            check(store.self_peaks(D, r), want[r])
            assert "smafa_pk::climb_kernel" in store.last_call_kernels() and pk_kernels(store) == CLIMBED
            scans.setdefault(knob, []).append(store.last_call_stats()["scans"])
        store.close()
    print("scans per call: %s" % scans)
    assert len(set(scans[None])) == 1 and scans[None][0] >= 1
    assert scans["0"] == [2 * s for s in scans[None]] and scans[str(pairs // 2)] == scans["0"], scans


@pytest.mark.parametrize("ceiling", [None, "1000000"])
def test_dense_store(ceiling, monkeypatch):
    """2 000 copies of one row + 2 000 of a second row at distance 3: two hot weight[] and best[] neighbourhoods of 2 000 rows
    (under the ceiling the piece is cut and the kept list, whose default capacity is that ceiling, overflows: joined twice).
    Kernels at bound 2: the scans, smafa_join::store_records_kernel, smafa_join::inverse_order_kernel, then
    smafa_pk::init_peaks_kernel, smafa_pk::weigh_keep_kernel, smafa_pk::climb_kernel, smafa_pk::settle_kernel,
    smafa_pk::jump_kernel; at bound 3 = radius 3, where the two rows are within the bound of each other, the same without
    the inverse order map, which is current."""
    codes, group = dense_store()
    first = [int(np.flatnonzero(group == g)[0]) for g in (0, 1)]
    assert min(first) == 0
    two = np.array(first, dtype=np.uint32)[group]
    if ceiling:
        monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", ceiling)
    store = make_store(codes, "nt")
    labels, parents, weights, n_peaks = store.self_peaks(2, 0)
    assert n_peaks == 2 and (weights == 2000).all()
    assert labels.tobytes() == two.tobytes() and parents.tobytes() == two.tobytes()
    kernels = store.last_call_kernels()
    assert not [k for k in kernels if k.startswith(("smafa_cc::", "smafa_lv::", "smafa_dn::"))] and "smafa_join::join_filter_kernel" not in kernels
    assert kernels[-7:] == ["smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel"] + CLIMBED, kernels
    assert kernels[0].startswith("smafa::") and all(k.startswith("smafa::") for k in kernels[:-7]), kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 7 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    if ceiling:  # the 4M pairs overflow a kept list of 1M: joined twice, piece for piece as the components call joins once
        store.self_components(2)
        once = store.last_call_stats()["scans"]
        assert once > 2 and stats["scans"] == 2 * once, (stats, once)
    labels, parents, weights, n_peaks = store.self_peaks(3, 3)
    assert n_peaks == 1 and (weights == 4000).all() and not labels.any() and not parents.any()
    kernels = store.last_call_kernels()
    assert kernels[-6:] == ["smafa_join::store_records_kernel"] + CLIMBED, kernels
    labels, parents, weights, n_peaks = store.self_peaks(3, 0)  # weights 2 000 again: ties, one peak, row 0
    assert n_peaks == 1 and (weights == 2000).all() and not labels.any() and not parents.any()
    store.close()


def test_every_engine_one_answer(monkeypatch):
    name, r = "aa60", 0
    codes, want, D, _ = case(name, 2000)
    want = want[r]
    store = make_store(codes, "aa")
    check(store.self_peaks(D, r), want)
    assert store.last_call_kernels()[0].startswith("smafa::scan_"), store.last_call_kernels()
    for on in (False, True):
        store.set_prefilter(on)
        check(store.self_peaks(D, r), want)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        check(store.self_peaks(D, r), want)
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
    check(store.self_peaks(D, r), want)
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    store.close()
    for mode in (2, 3):
        store = make_store(codes, "aa")
        store.set_index(mode)
        check(store.self_peaks(D, r), want)
        check(store.self_peaks(D, r), want)
        store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    # many pieces, with mirror images across pieces (and, with the index, repeats): every pair still weighs exactly once
    for var, value in (("SMAFA_JOIN_STRIDE", "1"), ("SMAFA_JOIN_BLOCK", "128")):
        monkeypatch.setenv(var, value)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv(var)
        check(store.self_peaks(D, r), want)
        check(store.self_peaks(D, D), case(name, 2000)[1][D])
        if var == "SMAFA_JOIN_BLOCK":  # 20 020 rows in blocks of 128
            assert store.last_call_stats()["scans"] >= 20020 // 128, store.last_call_stats()
        store.close()


def test_edges_and_errors():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    labels, parents, weights, n_peaks = store.self_peaks(5, 0)
    assert labels.shape == (0,) and parents.shape == (0,) and weights.shape == (0,) and n_peaks == 0
    rng = np.random.default_rng(4)
    store.push(rng.integers(0, 4, size=(1, L)).astype(np.uint8))
    for D, r in ((5, 0), (5, 5), (L, 0), (L + 1, L + 1)):
        labels, parents, weights, n_peaks = store.self_peaks(D, r)
        assert labels.tolist() == [0] and parents.tolist() == [0] and weights.tolist() == [1] and n_peaks == 1
        assert not [k for k in store.last_call_kernels() if k.startswith(("smafa::", "smafa_join::"))], store.last_call_kernels()  # no scan
    store.close()
    # bounds no two rows can exceed: one peak, the row of greatest key; the weights from a count-only join at r, or none
    L = 9
    codes = planted_store(5, "nt", L, 40)
    n = len(codes)
    store = make_store(codes, "nt")
    for bound in (L, L + 3):
        want = brute_peaks(codes, bound, 0)
        assert want[3] == 1 and len(set(want[0].tolist())) == 1 and want[2].max() > 1
        got = store.self_peaks(bound, 0)
        check(got, want)
        kernels = store.last_call_kernels()
        assert any(k.startswith("smafa::") for k in kernels)  # the count-only join at r = 0
        assert pk_kernels(store) == [PK[0], PK[1], PK[3], PK[4]], kernels  # nothing climbed, nothing jumped
        check(store.self_peaks(bound, 2), brute_peaks(codes, bound, 2))
        for r in (L, bound, None):
            got = store.self_peaks(bound, r)
            assert not [k for k in store.last_call_kernels() if k.startswith(("smafa::", "smafa_join::"))], store.last_call_kernels()
            assert pk_kernels(store) == [PK[0], PK[3], PK[4]]
            assert (got[2] == n).all() and not got[0].any() and not got[1].any() and got[3] == 1
            check(got, brute_peaks(codes, bound, bound))
    check(store.self_peaks(L - 1, 0), brute_peaks(codes, L - 1, 0))
    assert any(k.startswith("smafa::") for k in store.last_call_kernels())
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_peaks(None, 0)
    assert e.value.code == _lib.ERR_INVALID
    want = brute_peaks(codes, 2, 0)
    out, par, wts = (np.full(n, 7, dtype=np.uint32) for _ in range(3))
    count = (C.c_uint64 * 1)(9)
    l = _lib.lib()

    def untouched():
        return (out == 7).all() and (par == 7).all() and (wts == 7).all() and count[0] == 9

    assert l.smafa_db_self_peaks(store._h, 2, 0, out.ctypes.data, par.ctypes.data, wts.ctypes.data, n - 1, count) == _lib.ERR_INVALID
    assert str(n - 1).encode() in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_peaks(store._h, 2, 0, None, par.ctypes.data, wts.ctypes.data, n, count) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_peaks(store._h, 2, 0, out.ctypes.data, par.ctypes.data, wts.ctypes.data, n, None) == _lib.ERR_INVALID
    assert b"NULL n_peaks" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_peaks(store._h, _lib.NONE, 0, out.ctypes.data, par.ctypes.data, wts.ctypes.data, n, count) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_peaks(store._h, 2, 3, out.ctypes.data, par.ctypes.data, wts.ctypes.data, n, count) == _lib.ERR_INVALID
    assert b"radius 3" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_peaks_launch(store._h, 2, 0, None, None, None, None) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error() and untouched()
    assert l.smafa_db_self_peaks(store._h, 2, 0, out.ctypes.data, None, None, n, count) == _lib.OK  # NULL parents / weights
    assert out.tobytes() == want[0].tobytes() and (par == 7).all() and (wts == 7).all() and count[0] == want[3]
    assert l.smafa_db_self_peaks(store._h, 2, 0, out.ctypes.data, par.ctypes.data, wts.ctypes.data, n, count) == _lib.OK
    assert par.tobytes() == want[1].tobytes() and wts.tobytes() == want[2].tobytes()
    store.close()


def test_a_chunk_that_cannot_fit_fails_as_the_join_does(monkeypatch):
    """the join's own SMAFA_ERR_NOMEM case, 70 000 equal rows: raised from the peaks call too (nothing is weighed from a
    partial list), and the handle then answers at a bound that needs no list"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    store = make_store(np.zeros((70_000, 60), dtype=np.uint8), "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_peaks(2, 0)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    labels, parents, weights, n_peaks = store.self_peaks(60, 60)
    assert n_peaks == 1 and not labels.any() and not parents.any() and (weights == 70_000).all()
    store.close()


def test_device_form():
    """smafa_db_self_peaks_launch on torch buffers — tests/peaks_worker.py, a process of its own: torch has to initialise
    HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "peaks_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "peaks device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_properties_at_scale():
    """1M x 60 aa in 10 000 families of 100, D = 5, r = 0 (the store of tests/test_gpu_density.py's scale case)"""
    D = 5
    codes = synth.related_subjects(10_000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    idx = np.arange(n)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    row, count = store.self_components(D)
    labels, parents, weights, n_peaks = store.self_peaks(D, 0)
    print("%d rows, D = %d: %d components, %d peaks; %s; %s" % (n, D, count, n_peaks, pk_kernels(store), store.last_call_stats()))
    assert pk_kernels(store) == CLIMBED
    assert (labels[labels] == labels).all() and (parents[labels] == labels).all()
    keys = keys_of(weights)
    moved = parents != idx
    assert moved.any() and (keys[parents[moved]] > keys[moved]).all()
    assert ((codes != codes[parents]).sum(axis=1) <= D).all()
    assert (row[labels] == row).all()  # the peak lies in the row's own single-linkage component
    assert n_peaks == int((~moved).sum()) and count <= n_peaks < n
    # whole components of about 2 000 rows in all, stored alone: the same weights, and brute force agrees
    comps, sizes = np.unique(row, return_counts=True)
    pick = np.isin(row, comps[: int(np.searchsorted(np.cumsum(sizes), 2000))])
    sub = np.ascontiguousarray(codes[pick])
    assert 1000 <= len(sub) <= 2000
    small = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    small.push(sub)
    want = brute_peaks(sub, D, 0)
    check(small.self_peaks(D, 0), want)
    assert weights[pick].tolist() == want[2].tolist()
    # renumbering whole components keeps the order of the numbers: the same forest, in the sub-sample's numbers
    new_number = np.cumsum(pick) - 1
    assert new_number[parents[pick]].tolist() == want[1].tolist() and new_number[labels[pick]].tolist() == want[0].tolist()
    small.close()
    store.close()


@pytest.mark.parametrize("kind,L,D,radius", [("nt", 60, 5, None), ("aa", 60, 3, 2)])
def test_cli_peaks(tmp_path, kind, L, D, radius):
    """the version-2 (nt) / version-3 (aa) file and the packed file; --radius defaulted (0) and given"""
    codes = planted_store(21, kind, L, 300)
    n = len(codes)
    r = 0 if radius is None else radius
    labels, parents, weights, n_peaks = brute_peaks(codes, D, r)
    assert 1 < n_peaks < n and moved_and_multi_step((labels, parents))[0] > 0
    text = "".join("%d\t%d\t%d\t%d\n" % (i, labels[i], parents[i], weights[i]) for i in range(n)).encode()
    fa, db, packed = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    extra = [] if radius is None else ["--radius", str(radius)]
    for path in (db, packed):
        p = subprocess.run([_lib.CLI_PATH, "peaks", "-d", path, "--max-divergence", str(D), *extra], capture_output=True)
        assert p.returncode == 0, p.stderr
        assert p.stdout == text, path
    out = str(tmp_path / "peaks.tsv")
    with open(out, "wb") as f:
        smafa_amd.peaks(db, D, r, out_fd=f.fileno())
    assert open(out, "rb").read() == text
    # an empty DB prints nothing
    empty_db = str(tmp_path / "e.db")
    # (a version-3 file, amino acids: a version-2 file without rows is three bytes, which `smafa` refuses as the reference does)
    smafa_amd.write_db(empty_db, np.zeros((0, L), dtype=np.uint8), smafa_amd.ALPHABET_AA)
    p = subprocess.run([_lib.CLI_PATH, "peaks", "-d", empty_db, "--max-divergence", "2"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b"", p.stderr

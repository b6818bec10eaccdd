"""Single-linkage components of a resident store (smafa_db_self_components / smafa_db_self_components_launch /
`smafa components`): labels[i] = the smallest subject number in i's connected component of the graph whose edges are the
store's pairs within the bound.

Expected labels never come from the code under test: the edges are brute force on the code bytes
(self_join_cases.brute_pairs) and the labels a plain union-find over them (tests/components_cases.py).  At 1M rows, where
brute force is out of reach, the labels are held against `self_pairs` and `scan`, which the suite holds against the oracle.
The file takes 13 s on an MI355X (4 s of it the device form's worker process, 2 s the 1M-row case)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import (brute_labels, chain_store, dense_store, labels_from_pairs_numpy, n_components,
                              widest_chained_component)
from self_join_cases import SHAPES, planted_store

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = ["smafa_cc::init_labels_kernel", "smafa_cc::link_rows_kernel", "smafa_cc::flatten_labels_kernel"]


@functools.lru_cache(maxsize=None)
def case(name, families):
    """-> (codes, expected labels, expected pairs, D) of a shape of SHAPES at `families` x 10 + 20 rows, the stores of
    tests/test_gpu_self_join.py (same seeds)"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    codes = planted_store(11 + families + len(name), kind, L, families, n_frac)
    want, pairs = brute_labels(codes, D)
    return codes, want, pairs, D


def kind_of(name):
    return next(s for s in SHAPES if s[0] == name)[1]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def check(got, want):
    labels, count = got
    assert labels.dtype == np.uint32 and labels.tobytes() == want.tobytes()
    assert count == int((want == np.arange(len(want))).sum())


@pytest.mark.parametrize("families", [300, 2000])
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_labels_equal_brute_force(name, families):
    codes, want, pairs, D = case(name, families)
    assert (want <= np.arange(len(want))).all() and (want[want] == want).all()
    chained = widest_chained_component(codes, want, D)
    if D > 0:
        # real chaining, not stars: a component of >= 3 rows whose farthest two members are more than D apart
        assert chained is not None and chained[0] >= 3 and chained[1] > D, name
    else:
        # At bound 0 an edge means EQUAL rows, and equality is transitive already: every member of a component is at distance
        # 0 from every other, so no store and no seed has a component wider than the bound.  What bound 0 can show is a
        # component of >= 3 rows (copies of copies), and that is asserted.
        assert chained is None and np.bincount(want).max() >= 3, name
    store = make_store(codes, kind_of(name))
    got = store.self_components(D)
    print("%s x %d rows, D = %d: %d pairs, %d components, chained %s, kernels %s" % (
        name, len(codes), D, len(pairs), got[1], chained, store.last_call_kernels()))
    check(got, want)
    store.close()


@pytest.mark.parametrize("seed", [1])
def test_chains(seed):
    """three chains of 2 048 rows, neighbours at distance exactly 1, shuffled together: 3 components at bound 1"""
    codes, which = chain_store(seed)
    assert len(codes) == 3 * 2048
    want1, _ = brute_labels(codes, 1)
    assert n_components(want1) == 3
    for c in range(3):  # and they are the chains: each labelled by its first-appended row
        assert (want1[which == c] == np.flatnonzero(which == c)[0]).all()
    want0, _ = brute_labels(codes, 0)
    assert n_components(want0) > 3
    store = make_store(codes, "nt")
    check(store.self_components(1), want1)
    check(store.self_components(0), want0)
    store.close()


@pytest.mark.parametrize("ceiling", [None, "1000000"])
def test_dense_store(ceiling, monkeypatch):
    """2 000 copies of one row + 2 000 of a second row at distance 3: 16M rows in the one block's list (four times the
    scratch list: scanned again; under the ceiling: halved) and two labels, or one, to show for them"""
    codes, group = dense_store()
    first = [int(np.flatnonzero(group == g)[0]) for g in (0, 1)]
    assert min(first) == 0
    if ceiling:
        monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", ceiling)
    store = make_store(codes, "nt")
    labels, count = store.self_components(3)
    assert count == 1 and not labels.any() and len(labels) == 4000
    kernels = store.last_call_kernels()
    assert "smafa_join::join_filter_kernel" not in kernels and "smafa_join::inverse_order_kernel" not in kernels, kernels
    assert [k for k in kernels if k.startswith("smafa_cc::")] == CC, kernels
    assert kernels.index("smafa_join::store_records_kernel") == len(kernels) - 4 and kernels[0].startswith("smafa::"), kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 5 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    labels, count = store.self_components(2)
    assert count == 2 and labels.tobytes() == np.array(first, dtype=np.uint32)[group].tobytes()
    store.close()


def test_every_engine_one_answer(monkeypatch):
    name = "aa60"
    codes, want, pairs, D = case(name, 2000)
    store = make_store(codes, "aa")
    check(store.self_components(D), want)
    assert store.last_call_kernels()[0].startswith("smafa::scan_"), store.last_call_kernels()
    for on in (False, True):
        store.set_prefilter(on)
        check(store.self_components(D), want)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        check(store.self_components(D), want)
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
    check(store.self_components(D), want)
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    for var, value in (("SMAFA_JOIN_STRIDE", "1"), ("SMAFA_JOIN_BLOCK", "128")):
        monkeypatch.setenv(var, value)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv(var)
        check(store.self_components(D), want)
        if var == "SMAFA_JOIN_BLOCK":  # 20 020 rows in blocks of 128
            assert store.last_call_stats()["scans"] >= 20020 // 128, store.last_call_stats()
        store.close()


def test_state_after_push_and_beside_the_join():
    codes, want, pairs, D = case("aa60", 300)
    more = planted_store(77, "aa", 60, 498)  # 5 000 rows
    store = make_store(codes, "aa")
    assert store.self_pairs(D).tobytes() == pairs.tobytes()
    check(store.self_components(D), want)
    assert store.self_pairs(D).tobytes() == pairs.tobytes()
    store.push(more)
    both = np.concatenate([codes, more])
    want2, pairs2 = brute_labels(both, D)
    assert len(pairs2) > len(pairs)
    check(store.self_components(D), want2)
    assert store.self_pairs(D, first_cap=1 << 20).tobytes() == pairs2.tobytes()
    check(store.self_components(D), want2)
    store.close()


def test_edges_and_errors():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    labels, count = store.self_components(5)
    assert len(labels) == 0 and count == 0
    rng = np.random.default_rng(4)
    first = rng.integers(0, 4, size=(1, L)).astype(np.uint8)
    store.push(first)
    labels, count = store.self_components(5)
    assert labels.tolist() == [0] and count == 1
    rest = rng.integers(0, 4, size=(299, L)).astype(np.uint8)
    rest[100] = rest[7]  # one pair of equal rows among unrelated ones
    store.push(rest)
    want, _ = brute_labels(np.concatenate([first, rest]), 5)
    assert n_components(want) == 299 and want[101] == 8
    check(store.self_components(5), want)
    check(store.self_components(0), want)
    for bound in (L, L + 1000):
        labels, count = store.self_components(bound)
        assert len(labels) == 300 and not labels.any() and count == 1
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_components(None)
    assert e.value.code == _lib.ERR_INVALID
    out = np.full(300, 7, dtype=np.uint32)
    count = C.c_uint64(9)
    l = _lib.lib()
    assert l.smafa_db_self_components(store._h, 5, out.ctypes.data, 299, C.byref(count)) == _lib.ERR_INVALID
    assert b"299" in l.smafa_last_error() and (out == 7).all()
    assert l.smafa_db_self_components(store._h, 5, None, 300, C.byref(count)) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error()
    assert l.smafa_db_self_components(store._h, 5, out.ctypes.data, 300, None) == _lib.ERR_INVALID
    assert b"NULL count" in l.smafa_last_error()
    assert l.smafa_db_self_components_launch(store._h, 5, None, None) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error()
    store.close()


def test_a_chunk_that_cannot_fit_fails_as_the_join_does(monkeypatch):
    """the join's own SMAFA_ERR_NOMEM case, 70 000 equal rows: raised from the components call too (no partial list is
    linked), and a handle made under the same settings then answers a small store"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    store = make_store(np.zeros((70_000, 60), dtype=np.uint8), "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_components(0)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    labels, count = store.self_components(60)  # the handle stays usable (this bound needs no list)
    assert count == 1 and not labels.any()
    store.close()
    codes, want, pairs, _ = case("aa60d0", 300)
    small = make_store(codes, "aa")
    check(small.self_components(0), want)
    small.close()


def test_device_form():
    """smafa_db_self_components_launch on torch buffers — tests/components_worker.py, a process of its own: torch has to
    initialise HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "components_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "components device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_against_the_join_and_the_query_path_at_scale():
    """1M x 60 aa in 10 000 families of 100, D = 5"""
    D = 5
    codes = synth.related_subjects(10_000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    labels, count = store.self_components(D)
    kernels = store.last_call_kernels()
    assert [k for k in kernels if k.startswith("smafa_cc::")] == CC and "smafa_join::join_filter_kernel" not in kernels, kernels
    assert len(labels) == n and (labels[labels] == labels).all() and (labels <= np.arange(n)).all()
    assert count == n_components(labels)
    pairs = store.self_pairs(D, first_cap=1 << 25)
    assert len(pairs) > n
    assert (labels[pairs["query"]] == labels[pairs["subject"]]).all()
    ref = labels_from_pairs_numpy(n, pairs)
    assert count == n_components(ref)
    # (equal counts + every edge inside one label = the same partition; labels are then the minima iff they equal ref's)
    assert labels.tobytes() == ref.tobytes()
    rng = np.random.default_rng(2)
    neighbours = 0
    for i in np.sort(rng.choice(n, size=200, replace=False)):
        near = store.scan(codes[i:i + 1], max_divergence=D)
        assert (labels[near["subject"]] == labels[i]).all(), i
        neighbours += len(near) - 1
    print("%d rows: %d pairs, %d components, %d neighbours over 200 sampled rows" % (n, len(pairs), count, neighbours))
    assert neighbours >= 200
    store.close()


@pytest.mark.parametrize("kind,L,D", [("nt", 60, 5), ("aa", 60, 5)])
def test_cli_components(tmp_path, kind, L, D):
    codes = planted_store(21, kind, L, 300)
    want, _ = brute_labels(codes, D)
    assert n_components(want) < len(want)
    text = "".join("%d\t%d\n" % (i, want[i]) for i in range(len(want))).encode()
    fa, db, packed = (str(tmp_path / n) for n in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, "components", "-d", path, "--max-divergence", str(D)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == text, path
    out = str(tmp_path / "components.tsv")
    with open(out, "wb") as f:
        smafa_amd.components(db, D, out_fd=f.fileno())
    assert open(out, "rb").read() == text

"""Single-linkage levels of a resident store (smafa_db_self_levels / smafa_db_self_levels_launch /
`smafa components --levels`): labels[t][i] = the smallest subject number in i's connected component of the graph whose
edges are the store's pairs at distance <= t, for every t = 0 .. D, from one join.

Expected labels never come from the code under test: the edges are brute force on the code bytes with their distances
(self_join_cases.brute_pairs) and level t a plain union-find over the edges with dist <= t (tests/levels_cases.py).  Row t
is also held against the components call at bound t, which tests/test_gpu_components.py holds against brute force.  At 1M
rows, where brute force is out of reach, the rows are held against their nesting properties, the components call at D and
the grouping of equal rows.
The file takes 15 s on an MI355X (3.5 s of it the device form's worker process, 3.3 s the 1M-row case, 6 s the two CLI cases)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import chain_store, dense_store, n_components
from levels_cases import brute_levels, check_nesting
from self_join_cases import SHAPES, planted_store

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LV = ["smafa_lv::init_levels_kernel", "smafa_lv::hook_levels_kernel", "smafa_lv::flatten_levels_kernel"]


@functools.lru_cache(maxsize=None)
def case(name, families):
    """-> (codes, expected labels (D + 1, n), expected counts, D) of a shape of SHAPES at `families` x 10 + 20 rows, the
    stores of tests/test_gpu_self_join.py (same seeds)"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    codes = planted_store(11 + families + len(name), kind, L, families, n_frac)
    want, counts, _ = brute_levels(codes, D)
    return codes, want, counts, D


def kind_of(name):
    return next(s for s in SHAPES if s[0] == name)[1]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def check(got, want, counts):
    labels, got_counts = got
    assert labels.dtype == np.uint32 and labels.shape == want.shape
    for t in range(len(want)):
        assert labels[t].tobytes() == want[t].tobytes(), "level %d" % t
    assert got_counts == counts


@pytest.mark.parametrize("name,families", [(s[0], 300) for s in SHAPES] + [("aa60", 2000)])
def test_every_level_equals_brute_force(name, families):
    codes, want, counts, D = case(name, families)
    check_nesting(want, counts)
    if D >= 2:  # every level a different answer: a build that returns row D for every level fails here
        assert len(set(counts)) >= 3, (name, counts)
    store = make_store(codes, kind_of(name))
    got = store.self_component_levels(D)
    print("%s x %d rows, D = %d: components %s, kernels %s" % (name, len(codes), D, got[1], store.last_call_kernels()))
    check(got, want, counts)
    store.close()


@pytest.mark.parametrize("which", ["chains", "nt60"])
def test_row_t_is_the_components_call_at_t(which):
    """row t, bytes and count, is what smafa_db_self_components(db, t) gives — on three shuffled chains of 2 048 rows whose
    neighbours are at distance exactly 1 (720 / 3 / 3 / 3 components), and on a planted store"""
    if which == "chains":
        codes, D = chain_store(1)[0], 3
    else:
        codes, D = case("nt60", 300)[0], 5
    store = make_store(codes, "nt")
    labels, counts = store.self_component_levels(D)
    assert labels.shape == (D + 1, len(codes))
    for t in range(D + 1):
        row, count = store.self_components(t)
        assert labels[t].tobytes() == row.tobytes() and counts[t] == count, t
    if which == "chains":
        assert counts[1:] == [3, 3, 3] and counts[0] > 3, counts
    check_nesting(labels, counts)
    store.close()


@pytest.mark.parametrize("ceiling", [None, "1000000"])
def test_dense_store(ceiling, monkeypatch):
    """2 000 copies of one row + 2 000 of a second row at distance 3: 16M rows in the one block's list (four times the
    scratch list: scanned again; under the ceiling: halved); levels 0 - 2 have two labels, level 3 one.  The kernels that
    ran are the smafa_lv:: ones, in order, after the scans and store_records_kernel — and none of smafa_cc::."""
    codes, group = dense_store()
    first = [int(np.flatnonzero(group == g)[0]) for g in (0, 1)]
    assert min(first) == 0
    two = np.array(first, dtype=np.uint32)[group]
    if ceiling:
        monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", ceiling)
    store = make_store(codes, "nt")
    labels, counts = store.self_component_levels(3)
    assert counts == [2, 2, 2, 1] and labels.shape == (4, 4000)
    for t in range(3):
        assert labels[t].tobytes() == two.tobytes(), t
    assert not labels[3].any()
    kernels = store.last_call_kernels()
    assert "smafa_join::join_filter_kernel" not in kernels and "smafa_join::inverse_order_kernel" not in kernels, kernels
    assert not [k for k in kernels if k.startswith("smafa_cc::")], kernels
    assert kernels[-3:] == LV and [k for k in kernels if k.startswith("smafa_lv::")] == LV, kernels
    assert kernels.index("smafa_join::store_records_kernel") == len(kernels) - 4 and kernels[0].startswith("smafa::"), kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 5 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    if ceiling:  # 16M rows over a list of 1M: the piece was cut more than once
        assert stats["scans"] > 4, stats
    store.close()


def test_every_engine_one_answer(monkeypatch):
    name = "aa60"
    codes, want, counts, D = case(name, 2000)
    store = make_store(codes, "aa")
    check(store.self_component_levels(D), want, counts)
    assert store.last_call_kernels()[0].startswith("smafa::scan_"), store.last_call_kernels()
    for on in (False, True):
        store.set_prefilter(on)
        check(store.self_component_levels(D), want, counts)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        check(store.self_component_levels(D), want, counts)
        if level == 2:
            assert any("scan_zone_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()
    store.close()
    # a current block index answers the blocks (limits lifted as tests/test_gpu_self_join.py lifts them); modes 2 and 3 may
    # build one on the way
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = make_store(codes, "aa")
    info = store.build_index(D)
    store.set_index(1)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    before = store.index_info()["probe_launches"]
    check(store.self_component_levels(D), want, counts)
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    store.close()
    for mode in (2, 3):
        store = make_store(codes, "aa")
        store.set_index(mode)
        check(store.self_component_levels(D), want, counts)
        check(store.self_component_levels(D), want, counts)
        store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    for var, value in (("SMAFA_JOIN_STRIDE", "1"), ("SMAFA_JOIN_BLOCK", "128")):
        monkeypatch.setenv(var, value)  # (read when the handle is made)
        store = make_store(codes, "aa")
        monkeypatch.delenv(var)
        check(store.self_component_levels(D), want, counts)
        if var == "SMAFA_JOIN_BLOCK":  # 20 020 rows in blocks of 128
            assert store.last_call_stats()["scans"] >= 20020 // 128, store.last_call_stats()
        store.close()


def test_edges_and_errors():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    labels, counts = store.self_component_levels(5)
    assert labels.shape == (6, 0) and counts == [0] * 6
    rng = np.random.default_rng(4)
    first = rng.integers(0, 4, size=(1, L)).astype(np.uint8)
    store.push(first)
    labels, counts = store.self_component_levels(5)
    assert labels.tolist() == [[0]] * 6 and counts == [1] * 6
    assert not [k for k in store.last_call_kernels() if k.startswith("smafa::")], store.last_call_kernels()  # no scan
    rest = rng.integers(0, 4, size=(299, L)).astype(np.uint8)
    rest[100] = rest[7]  # one pair of equal rows among unrelated ones
    rest[200] = rest[7]
    rest[200, 5] = (rest[200, 5] + 1) % 4  # and a third row at distance 1 of them
    store.push(rest)
    codes = np.concatenate([first, rest])
    want, want_counts, _ = brute_levels(codes, 5)
    assert want_counts[:2] == [299, 298] and want[0][101] == 8 and want[1][201] == 8 and want[0][201] == 201
    check(store.self_component_levels(5), want, want_counts)
    check(store.self_component_levels(0), want[:1], want_counts[:1])
    store.close()
    # bounds no two rows can exceed: levels >= L are zero rows with one component, the rows below are still brute force
    L = 9
    codes = planted_store(5, "nt", L, 40)  # 420 rows: brute force lists nearly every pair at these bounds
    n = len(codes)
    store = make_store(codes, "nt")
    want, want_counts, _ = brute_levels(codes, L + 3)
    assert want_counts[0] > want_counts[1] > want_counts[2] > 1 and want_counts[L - 1] >= 1, want_counts
    for t in range(L, L + 4):
        assert not want[t].any() and want_counts[t] == 1  # (brute force agrees: every pair is within L)
    for bound in (L - 1, L, L + 3):  # (level t does not depend on the largest bound asked for)
        check(store.self_component_levels(bound), want[:bound + 1], want_counts[:bound + 1])
        assert any(k.startswith("smafa::") for k in store.last_call_kernels())  # the levels below L are scanned for
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_component_levels(None)
    assert e.value.code == _lib.ERR_INVALID
    out = np.full(3 * n, 7, dtype=np.uint32)
    count = (C.c_uint64 * 3)(9, 9, 9)
    l = _lib.lib()
    assert l.smafa_db_self_levels(store._h, 2, out.ctypes.data, 3 * n - 1, count) == _lib.ERR_INVALID
    assert str(3 * n - 1).encode() in l.smafa_last_error() and (out == 7).all()
    assert l.smafa_db_self_levels(store._h, 2, out.ctypes.data, n, count) == _lib.ERR_INVALID  # room for one level only
    assert l.smafa_db_self_levels(store._h, 2, None, 3 * n, count) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error()
    assert l.smafa_db_self_levels(store._h, 2, out.ctypes.data, 3 * n, None) == _lib.ERR_INVALID
    assert b"NULL count" in l.smafa_last_error()
    assert l.smafa_db_self_levels(store._h, _lib.NONE, out.ctypes.data, 3 * n, count) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert l.smafa_db_self_levels_launch(store._h, 2, None, None) == _lib.ERR_INVALID
    assert b"NULL labels" in l.smafa_last_error()
    assert l.smafa_db_self_levels(store._h, 2, out.ctypes.data, 3 * n, count) == _lib.OK
    assert out.tobytes() == want[:3].tobytes() and list(count) == want_counts[:3]
    store.close()


def test_a_chunk_that_cannot_fit_fails_as_the_join_does(monkeypatch):
    """the join's own SMAFA_ERR_NOMEM case, 70 000 equal rows: raised from the levels call too (no partial list is linked),
    and the handle then answers the components call at a bound that needs no list"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")
    store = make_store(np.zeros((70_000, 60), dtype=np.uint8), "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_component_levels(2)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    labels, count = store.self_components(60)
    assert count == 1 and not labels.any()
    store.close()


def test_device_form():
    """smafa_db_self_levels_launch on torch buffers — tests/levels_worker.py, a process of its own: torch has to initialise
    HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "levels_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "levels device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_nesting_and_the_components_call_at_scale():
    """1M x 60 aa in 10 000 families of 100, D = 5 (the store of
    tests/test_gpu_components.py::test_against_the_join_and_the_query_path_at_scale)"""
    D = 5
    codes = synth.related_subjects(10_000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    labels, counts = store.self_component_levels(D)
    kernels = store.last_call_kernels()
    assert [k for k in kernels if k.startswith("smafa_lv::")] == LV and not [k for k in kernels if k.startswith("smafa_cc::")], kernels
    assert labels.shape == (D + 1, n)
    check_nesting(labels, counts)
    assert counts == sorted(counts, reverse=True) and [n_components(labels[t]) for t in range(D + 1)] == counts
    assert len(set(counts)) >= 3, counts
    row, count = store.self_components(D)
    assert labels[D].tobytes() == row.tobytes() and counts[D] == count
    # level 0 is the grouping of equal rows: each row labelled by the first row equal to it
    _, first, inverse = np.unique(codes, axis=0, return_index=True, return_inverse=True)
    assert labels[0].tobytes() == first[inverse.reshape(-1)].astype(np.uint32).tobytes()
    print("%d rows: components per level %s" % (n, counts))
    store.close()


@pytest.mark.parametrize("kind,L,D", [("nt", 60, 5), ("aa", 60, 3)])
def test_cli_levels(tmp_path, kind, L, D):
    codes = planted_store(21, kind, L, 300)
    n = len(codes)
    want, counts, _ = brute_levels(codes, D)
    assert len(set(counts)) >= 3
    text = "".join("%d\t%s\n" % (i, "\t".join(str(v) for v in want[:, i])) for i in range(n)).encode()
    fa, db, packed = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, "components", "-d", path, "--max-divergence", str(D), "--levels"], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == text, path
    # column t + 1 is the label column of `smafa components --max-divergence t`, whose bytes the flag leaves as they were
    columns = [line.split(b"\t") for line in text.splitlines()]
    for t in range(D + 1):
        r = subprocess.run([_lib.CLI_PATH, "components", "-d", db, "--max-divergence", str(t)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == b"".join(c[0] + b"\t" + c[t + 1] + b"\n" for c in columns), t
        assert r.stdout == "".join("%d\t%d\n" % (i, want[t, i]) for i in range(n)).encode(), t
    out = str(tmp_path / "levels.tsv")
    with open(out, "wb") as f:
        smafa_amd.component_levels(db, D, out_fd=f.fileno())
    assert open(out, "rb").read() == text
    # an empty DB prints nothing
    empty_db = str(tmp_path / "e.db")
    # (a version-3 file, amino acids: a version-2 file without rows is three bytes, which `smafa` refuses as the reference does)
    smafa_amd.write_db(empty_db, np.zeros((0, L), dtype=np.uint8), smafa_amd.ALPHABET_AA)
    r = subprocess.run([_lib.CLI_PATH, "components", "-d", empty_db, "--max-divergence", "2", "--levels"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr

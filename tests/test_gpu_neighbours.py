"""Neighbour lists of a resident store (smafa_db_self_neighbours / smafa_db_self_neighbours_launch / `smafa neighbours`):
offsets[i] .. offsets[i + 1] bound row i's neighbours within the bound, ordered by (distance, number), cut to the k nearest.

Expected answers never come from the code under test: tests/neighbours_cases.py::brute_neighbours works row by row on the
code bytes, and the comparison is exact equality of the three arrays.  At 200 000 rows, and for all but the first and last
rows of the dense store, the answer is held against its properties and the pairs and density calls."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import dense_store
from neighbours_cases import (brute_neighbours, cut_lists, middle_pair, no_pair, planted_ends, rows_of, same, short_store,
                              tie_family)
from self_join_cases import SHAPES, SPANS_FAMILIES, ONE_SPAN_FAMILIES, planted_store, shape_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = ["smafa_nb::mirror_pack_kernel", "smafa_nb::row_bounds_kernel", "smafa_nb::cut_degrees_kernel", "smafa_nb::emit_kernel"]
UNCUT = [NB[0], NB[1], NB[3]]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def nb_kernels(store):
    return [k for k in store.last_call_kernels() if k.startswith("smafa_nb::")]


@functools.lru_cache(maxsize=None)
def case(name, D):
    """-> (codes, the whole brute-force answer at D) of a shape of SHAPES at 300 x 10 + 20 rows, the stores of
    tests/test_gpu_self_join.py (same seeds)"""
    _, kind, L, _, n_frac = next(s for s in SHAPES if s[0] == name)
    codes = planted_store(11 + 300 + len(name), kind, L, 300, n_frac)
    return codes, brute_neighbours(codes, D)


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_neighbours_equal_brute_force(name):
    _, kind, L, D, _ = next(s for s in SHAPES if s[0] == name)
    store = None
    for bound in ((D, D - 2) if D >= 2 else (0, 1)):
        codes, whole = case(name, bound)
        assert len(whole[1]) > 0 and int(whole[2].max()) == bound
        if store is None:
            store = make_store(codes, kind)
        for k in (None, 1, 3):
            same(store.self_neighbours(bound, k), cut_lists(whole, k))
            assert nb_kernels(store) == (UNCUT if k is None else NB), store.last_call_kernels()
        got = store.self_neighbours(bound, 3, dists=False)
        same(got, cut_lists(whole, 3), dists=False)
    kernels = store.last_call_kernels()
    assert kernels[0].startswith("smafa::") and "smafa_join::store_records_kernel" in kernels
    assert not [k for k in kernels if k.startswith(("smafa_cc::", "smafa_lv::", "smafa_dn::", "smafa_pk::"))]
    store.close()


def sorts_traced(err):
    """the "(N sort[s])" of every level-2 summary line of a neighbours call that had entries to order"""
    return [int(m) for m in re.findall(r"neighbours of \d+ rows.*?\((\d) sorts?\), .*? [1-9]\d* entries", err)]


def run_sort2(which):
    """a child process: the same stores under SMAFA_NEIGHBOUR_SORT=2, their answers as bytes on stdout; every call's summary
    line (level-2 trace, on the child's stderr) must say that two sorts ran"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import smafa_amd, test_gpu_neighbours as t\n"
            "smafa_amd._lib.lib().smafa_set_verbosity(2)\n"
            "sys.stdout.write(t.key_width_answers(%r).hex())\n" % (ROOT, os.path.join(ROOT, "tests"), which))
    env = dict(os.environ, SMAFA_NEIGHBOUR_SORT="2")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-1500:]
    sorts = sorts_traced(r.stderr)
    # two bounds x (no cut, k = 2), and a call more wherever the lists outgrew the first capacity offered
    assert len(sorts) >= 4 and set(sorts) == {2}, (sorts, r.stderr[-1500:])
    return bytes.fromhex(r.stdout)


KEY_WIDTH_STORES = {
    "ends257": (lambda: planted_ends(257), (3, 4)),
    "ends513": (lambda: planted_ends(513), (3, 4)),
    "short": (lambda: short_store(), (4, 9)),
}


def key_width_answers(which, check=False):
    """every answer of one store of KEY_WIDTH_STORES, concatenated; check: each against brute force"""
    build, bounds = KEY_WIDTH_STORES[which]
    codes = build()
    n = len(codes)
    store = make_store(codes, "nt")
    out = b""
    for D in bounds:
        whole = brute_neighbours(codes, D) if check else None
        for k in (None, 2):
            got = store.self_neighbours(D, k)
            if check:
                same(got, cut_lists(whole, k))
                if which == "short":
                    assert k is not None or ((np.diff(got[0].astype(np.int64)) == n - 1).all() and int(got[2].max()) == 4)
                else:
                    lists = {i: got[1][int(got[0][i]):int(got[0][i + 1])].tolist() for i in (0, n - 1)}
                    assert lists == {0: [n - 1], n - 1: [0]}, lists
            out += b"".join(a.tobytes() for a in got)
    store.close()
    return out


@pytest.mark.parametrize("which", list(KEY_WIDTH_STORES))
def test_key_widths_and_the_two_sort_path(which, capfd):
    """n = 257 and 513 (the row field widens) with rows 0 and n - 1 planted as neighbours, D = 3 and 4 (the distance field
    widens); seq_len 4 at D = 4 and 9, every row listing every other; then the same under SMAFA_NEIGHBOUR_SORT=2 in a child
    process: identical bytes"""
    _lib.lib().smafa_set_verbosity(2)
    try:
        one = key_width_answers(which, check=True)
    finally:
        _lib.lib().smafa_set_verbosity(0)
    sorts = sorts_traced(capfd.readouterr().err)
    assert len(sorts) >= 4 and set(sorts) == {1}, sorts  # by the key rule these stores take one sort
    assert run_sort2(which) == one


def test_gaps():
    codes, a, b = middle_pair()
    n = len(codes)
    store = make_store(codes, "nt")
    for k in (None, 1):
        offsets, nb, ds = store.self_neighbours(3, k)
        want = np.zeros(n + 1, dtype=np.uint64)
        want[a + 1:] = 1
        want[b + 1:] = 2
        assert offsets.tobytes() == want.tobytes() and nb.tolist() == [b, a] and ds.tolist() == [1, 1]
    store.close()
    codes = no_pair()
    store = make_store(codes, "nt")
    for k in (None, 2):
        offsets, nb, ds = store.self_neighbours(3, k)
        assert offsets.shape == (len(codes) + 1,) and not offsets.any() and len(nb) == 0 and len(ds) == 0
        kernels = store.last_call_kernels()
        assert nb_kernels(store) == [NB[0]] and "smafa_join::store_records_kernel" in kernels, kernels  # no sort, bounds or emit
    store.close()


def test_ties_at_the_cut():
    codes, is_copy = tie_family()
    whole = brute_neighbours(codes, 2)
    store = make_store(codes, "nt")
    copies = np.flatnonzero(is_copy).tolist()
    for k in (1, 39, 40, 41, 79):
        got = store.self_neighbours(2, k)
        same(got, cut_lists(whole, k))
        for i in range(80):
            mine = got[1][int(got[0][i]):int(got[0][i + 1])].tolist()
            assert len(mine) == k
            nearest = [c for c in copies if c != i]  # distance 0 for a copy, distance 1 for a variant
            assert mine[:min(k, len(nearest))] == nearest[:k], (k, i)
    same(store.self_neighbours(2), whole)
    store.close()


@pytest.mark.parametrize("sorts", [1, 2])
def test_growth_over_many_pieces(sorts, monkeypatch, capfd):
    """blocks of 192 rows in spans of 3: eight pieces, the entry list grows in front of several of them with the live entries
    carried over — and, on the two-sort path, the live rows of the list beside them"""
    codes, _ = shape_case("nt60", SPANS_FAMILIES, 5)
    whole = brute_neighbours(codes, 5)
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "192")
    monkeypatch.setenv("SMAFA_JOIN_STRIDE", "3")
    if sorts == 2:
        monkeypatch.setenv("SMAFA_NEIGHBOUR_SORT", "2")  # (read when the handle is made)
    store = make_store(codes, "nt")
    monkeypatch.delenv("SMAFA_NEIGHBOUR_SORT", raising=False)
    _lib.lib().smafa_set_verbosity(2)
    try:
        got = store.self_neighbours(5, first_cap=1 << 20)
    finally:
        _lib.lib().smafa_set_verbosity(0)
    err = capfd.readouterr().err
    same(got, whole)
    line = [ln for ln in err.splitlines() if "neighbours of 1520 rows" in ln]
    assert len(line) == 1, err
    print(line[0])
    m = re.search(r"(\d+) entries, (\d+) listed, (\d+) growths", line[0])
    assert m and int(m.group(1)) == len(whole[1]) == int(m.group(2)) and int(m.group(3)) >= 2, line[0]
    assert sorts_traced(err) == [sorts], line[0]
    assert store.last_call_stats()["scans"] >= 8
    same(store.self_neighbours(5, 2, first_cap=1 << 20), cut_lists(whole, 2))  # the list is large enough now
    store.close()


def test_dense_store():
    """2 000 copies of one row + 2 000 of a second row at distance 3, bound 3: every row lists the 3 999 others, 16M entries"""
    codes, group = dense_store()
    n = len(codes)
    store = make_store(codes, "nt")
    pairs = len(store.self_pairs(3, first_cap=1 << 23))
    _, degrees, _ = store.self_density(3, 1)
    got = store.self_neighbours(3, first_cap=n * (n - 1))
    offsets, nb, ds = got
    assert len(nb) == 2 * pairs == n * (n - 1) and int(offsets[n]) == len(nb)
    assert np.diff(offsets.astype(np.int64)).tolist() == degrees.tolist()
    rows = list(range(50)) + list(range(n - 50, n))
    same(rows_of(got, rows), brute_neighbours(codes, 3, rows=rows))
    assert nb_kernels(store) == UNCUT
    cut = store.self_neighbours(3, 5)
    same(rows_of(cut, rows), brute_neighbours(codes, 3, 5, rows=rows))
    assert int(cut[0][n]) == 5 * n and (cut[2] == 0).all()
    store.close()


def test_every_engine_one_answer(monkeypatch):
    D = 5
    codes, whole = case("aa60", D)
    want = cut_lists(whole, 4)
    store = make_store(codes, "aa")
    same(store.self_neighbours(D, 4), want)
    for on in (False, True):
        store.set_prefilter(on)
        same(store.self_neighbours(D, 4), want)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        same(store.self_neighbours(D, 4), want)
        if level == 2:
            assert any("scan_zone_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()
    store.close()
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = make_store(codes, "aa")
    info = store.build_index(D)
    store.set_index(1)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    before = store.index_info()["probe_launches"]
    same(store.self_neighbours(D, 4), want)
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    store.close()
    for mode in (2, 3):
        store = make_store(codes, "aa")
        store.set_index(mode)
        same(store.self_neighbours(D, 4), want)
        same(store.self_neighbours(D, 4), want)
        store.close()


def test_capacity_and_errors():
    codes, whole = case("nt60", 5)
    n = len(codes)
    total = len(whole[1])
    store = make_store(codes, "nt")
    l = _lib.lib()
    offsets = np.full(n + 1, 7, dtype=np.uint64)
    nb, ds = (np.full(total + 8, 7, dtype=np.uint32) for _ in range(2))
    n_out = (C.c_uint64 * 1)(9)

    def untouched():
        return (nb == 7).all() and (ds == 7).all()

    # the degrees alone
    assert l.smafa_db_self_neighbours(store._h, 5, _lib.NONE, offsets.ctypes.data, None, None, 0, n_out) == _lib.ERR_CAPACITY
    assert n_out[0] == total and offsets.tobytes() == whole[0].tobytes()
    offsets[:] = 7
    assert l.smafa_db_self_neighbours(store._h, 5, _lib.NONE, offsets.ctypes.data, nb.ctypes.data, ds.ctypes.data, total - 1, n_out) == _lib.ERR_CAPACITY
    assert str(total).encode() in l.smafa_last_error() and n_out[0] == total and offsets.tobytes() == whole[0].tobytes() and untouched()
    assert l.smafa_db_self_neighbours(store._h, 5, _lib.NONE, offsets.ctypes.data, nb.ctypes.data, ds.ctypes.data, total, n_out) == _lib.OK
    assert nb[:total].tobytes() == whole[1].tobytes() and ds[:total].tobytes() == whole[2].tobytes() and (nb[total:] == 7).all()
    nb[:] = 7
    ds[:] = 7
    assert l.smafa_db_self_neighbours(store._h, 5, _lib.NONE, offsets.ctypes.data, nb.ctypes.data, None, total, n_out) == _lib.OK  # dists = NULL
    assert nb[:total].tobytes() == whole[1].tobytes() and (ds == 7).all()
    # invalid arguments: named, and nothing written
    nb[:] = 7
    offsets[:] = 7
    n_out[0] = 9
    for args, word in (((5, 0, offsets.ctypes.data, nb.ctypes.data, ds.ctypes.data, total, n_out), b"max_num_hits"),
                       ((_lib.NONE, 3, offsets.ctypes.data, nb.ctypes.data, ds.ctypes.data, total, n_out), b"bound"),
                       ((5, 3, None, nb.ctypes.data, ds.ctypes.data, total, n_out), b"NULL offsets"),
                       ((5, 3, offsets.ctypes.data, nb.ctypes.data, ds.ctypes.data, total, None), b"NULL n_out"),
                       ((5, 3, offsets.ctypes.data, None, ds.ctypes.data, total, n_out), b"NULL neighbours")):
        assert l.smafa_db_self_neighbours(store._h, *args) == _lib.ERR_INVALID
        assert word in l.smafa_last_error(), l.smafa_last_error()
        assert untouched() and (offsets == 7).all() and n_out[0] == 9
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_neighbours(None)
    assert e.value.code == _lib.ERR_INVALID
    store.close()
    # an empty store and a single row
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    offsets, nb, ds = store.self_neighbours(5)
    assert offsets.tolist() == [0] and len(nb) == 0 and len(ds) == 0
    store.push(codes[:1])
    offsets, nb, ds = store.self_neighbours(5, 2)
    assert offsets.tolist() == [0, 0] and len(nb) == 0
    store.close()


def test_device_form():
    """smafa_db_self_neighbours_launch on torch buffers — tests/neighbours_worker.py, a process of its own: torch has to
    initialise HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "neighbours_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "neighbours device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.parametrize("name,families,D", [("aa250", ONE_SPAN_FAMILIES, 5), ("nt330", SPANS_FAMILIES, 5)])
def test_wide_records_and_off_grid_spans(name, families, D, monkeypatch):
    """two stores of the join's second case table: aa 250 columns (records of two LDS windows) and nt 330 on two planes, the
    latter in spans of 3 x 192 positions that begin inside a wave tile"""
    codes, _ = shape_case(name, families, D)
    if families == SPANS_FAMILIES:
        monkeypatch.setenv("SMAFA_JOIN_BLOCK", "192")
        monkeypatch.setenv("SMAFA_JOIN_STRIDE", "3")
    store = make_store(codes, name[:2])
    whole = brute_neighbours(codes, D)
    same(store.self_neighbours(D), whole)
    same(store.self_neighbours(D, 2), cut_lists(whole, 2))
    if families == SPANS_FAMILIES:
        assert store.last_call_stats()["scans"] >= 8
    store.close()


def test_properties_at_scale():
    """200 000 x 60 aa in 2 000 families of 100, D = 5"""
    D = 5
    codes = synth.related_subjects(2_000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    _, degrees, _ = store.self_density(D, 1)
    offsets, nb, ds = store.self_neighbours(D, first_cap=1 << 24)
    print("%d rows, D = %d: %d entries; %s; %s" % (n, D, len(nb), nb_kernels(store), store.last_call_stats()))
    assert nb_kernels(store) == UNCUT
    deg = np.diff(offsets.astype(np.int64))
    assert deg.tolist() == degrees.tolist() and int(offsets[n]) == len(nb) == len(ds) and len(nb) > n
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    nbi = nb.astype(np.int64)
    assert (nbi != row).all() and int(ds.max()) == D  # no self entry
    # sorted by (dist, neighbour) within a row: the triple (row, dist, neighbour) strictly increases along the arrays
    key = (row << 40) | (ds.astype(np.int64) << 32) | nbi
    assert (np.diff(key) > 0).all()
    # symmetry: the mirrored triples are the same set
    mirror = np.sort((nbi << 40) | (ds.astype(np.int64) << 32) | row)
    assert (mirror == key).all()
    # distances are the real ones, on a sample
    pick = np.random.default_rng(1).choice(len(nb), size=20000, replace=False)
    assert ((codes[row[pick]] != codes[nbi[pick]]).sum(axis=1) == ds[pick]).all()
    # the cut output is the prefix of the uncut one, row by row
    want = cut_lists((offsets, nb, ds), 5)
    got = store.self_neighbours(D, 5, first_cap=1 << 21)
    same(got, want)
    assert nb_kernels(store) == NB
    store.close()


@pytest.mark.parametrize("fixture", ["random_3_2.fna.smafadb", "random_3_2_one_repeated.fna.smafadb"])
def test_cli_neighbours(fixture, tmp_path):
    path = os.path.join(ROOT, "tests", "golden", fixture)
    _, codes = smafa_amd.read_db(path)
    n, L = codes.shape
    D = L  # few rows: at the sequence length every row lists every other, nearest first
    for k in (None, 1):
        offsets, nb, ds = brute_neighbours(codes, D, k)
        assert len(nb) == (n * (n - 1) if k is None else n)
        text = "".join("%d\t%d\t%d\n" % (i, nb[e], ds[e]) for i in range(n) for e in range(int(offsets[i]), int(offsets[i + 1]))).encode()
        extra = [] if k is None else ["--max-num-hits", str(k)]
        p = subprocess.run([_lib.CLI_PATH, "neighbours", "-d", path, "--max-divergence", str(D), *extra], capture_output=True)
        assert p.returncode == 0, p.stderr
        assert p.stdout == text
    out = str(tmp_path / "nb.tsv")
    with open(out, "wb") as f:
        smafa_amd.neighbours(path, D, 1, out_fd=f.fileno())
    assert open(out, "rb").read() == text
    # a missing --max-divergence: the usage error and exit status of the sibling commands
    p = subprocess.run([_lib.CLI_PATH, "neighbours", "-d", path], capture_output=True)
    q = subprocess.run([_lib.CLI_PATH, "peaks", "-d", path], capture_output=True)
    assert p.returncode == q.returncode == 2 and b"neighbours needs --max-divergence" in p.stderr and p.stdout == b""

"""Abundance-peak clusters with given weights (smafa_db_self_peaks_weighted): with every weight 1 every array is byte-equal to
smafa_db_self_peaks on the stores of tests/peaks_cases.py and tests/test_gpu_peaks.py; with random weights, zeros among them,
every array equals brute force (tests/peaks_weighted_cases.py); the peaks of a raw store are the peaks of its distinct rows under
their sizes, lifted; the device form; the verb."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib
from peaks_weighted_cases import brute_weighted_peaks, expected_derep, identity_store, lifted, random_weights
from peaks_cases import climb_chain, valley_store
from self_join_cases import SHAPES, planted_store
from subset_cases import DeviceArray

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIMBED = ["smafa_pk::init_peaks_kernel", "smafa_pk::weigh_keep_kernel", "smafa_pk::climb_kernel", "smafa_pk::settle_kernel", "smafa_pk::jump_kernel"]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def same(got, want):
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert got[3] == want[3], (got[3], want[3])


def pk_kernels(store):
    return [k for k in store.last_call_kernels() if k.startswith("smafa_pk::")]


STORES = ["valley", "chain"] + [s[0] for s in SHAPES]


def store_case(name):
    """-> (kind, codes, D): the valley, the climb chain, or a planted store of a shape of the self-join tests"""
    if name == "valley":
        return "nt", valley_store(3)[0], 1
    if name == "chain":
        return "nt", climb_chain(), 1
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    return kind, planted_store(11 + 150 + len(name), kind, L, 150, n_frac), D


@pytest.mark.parametrize("name", STORES)
def test_ones_are_the_plain_call_and_random_weights_equal_brute_force(name):
    kind, codes, D = store_case(name)
    n = len(codes)
    store = make_store(codes, kind)
    ones = np.ones(n, dtype=np.uint32)
    w = random_weights(n, len(name))
    assert (w == 0).any() and (w > 1).any()
    for radius in (0, None):
        same(store.self_peaks(D, radius, weights_in=ones), store.self_peaks(D, radius))
        got = store.self_peaks(D, radius, weights_in=w)
        same(got, brute_weighted_peaks(codes, D, radius, w))
        assert "smafa_pk::weigh_keep_kernel" in store.last_call_kernels()
    labels, parents, weights, _ = store.self_peaks(D, 0, parents=False, weights=False, weights_in=w)
    assert parents is None and weights is None and labels.tobytes() == brute_weighted_peaks(codes, D, 0, w)[0].tobytes()
    store.close()


def test_kernels_and_launches_are_the_plain_calls():
    """the weights are an argument of smafa_pk::init_peaks_kernel (mode 2) and smafa_pk::weigh_keep_kernel: the call with given
    weights launches what the plain call launches, kernel for kernel"""
    codes = climb_chain()
    store = make_store(codes, "nt")
    store.self_peaks(1, 0)  # (the inverse order map is current from here on)
    store.self_peaks(1, 0)
    plain, launches = store.last_call_kernels(), store.last_call_stats()["launches"]
    store.self_peaks(1, 0, weights_in=np.ones(len(codes), dtype=np.uint32))
    assert pk_kernels(store) == CLIMBED and store.last_call_kernels() == plain and store.last_call_stats()["launches"] == launches
    store.close()


# ---- the identity: what the weights are for
@pytest.mark.parametrize("kind", ("nt", "aa"))
def test_peaks_of_the_raw_store_are_the_lifted_peaks_of_its_distinct_rows(kind):
    codes, D = identity_store(kind), 3
    derep = expected_derep(codes)  # on the host: unique_of, old_of_new, sizes
    raw = make_store(codes, kind)
    uniques = make_store(np.ascontiguousarray(codes[derep[1]]), kind)
    for radius in (0, None):
        want = raw.self_peaks(D, radius)
        got = uniques.self_peaks(D, radius, weights_in=derep[2])
        assert not lifted(want, derep, got), (kind, radius)
        assert lifted(want, derep, uniques.self_peaks(D, radius))  # ... and not without the sizes
    raw_pairs, unique_pairs = len(raw.self_pairs(D)), len(uniques.self_pairs(D))  # what either side's join keeps
    assert 0 < unique_pairs < raw_pairs and not (uniques.self_pairs(D)["dist"] == 0).any()
    uniques.close(), raw.close()


def test_edges_and_errors():
    codes = planted_store(5, "nt", 60, 30)
    n, L = codes.shape
    store = make_store(codes, "nt")
    w = random_weights(n, 1)
    ones = np.ones(n, dtype=np.uint32)
    total = int(w.astype(np.uint64).sum())
    # max_div >= seq_len: one peak; the weights from a count-only join at r, or — r >= seq_len too — the sum of the weights
    for radius in (0, 2, L, None):
        same(store.self_peaks(L, radius, weights_in=ones), store.self_peaks(L, radius))
        got = store.self_peaks(L + 5, radius, weights_in=w)
        same(got, brute_weighted_peaks(codes, L, radius, w))
        assert got[3] == 1 and "smafa_pk::crown_kernel" in store.last_call_kernels()
        if radius in (L, None):
            assert (got[2] == total).all() and store.last_call_stats()["scans"] == 0
    # a sum past 32 bits
    big = np.full(n, 0xFFFFFFFF // n, dtype=np.uint32)
    same(store.self_peaks(2, 0, weights_in=big), brute_weighted_peaks(codes, 2, 0, big))
    big[3] += 0xFFFFFFFF - int(big.astype(np.uint64).sum()) + 1
    with pytest.raises(smafa_amd.SmafaError, match="smafa_db_self_peaks_weighted: the weights sum to 4294967296") as e:
        store.self_peaks(2, 0, weights_in=big)
    assert e.value.code == _lib.ERR_INVALID
    same(store.self_peaks(2, 0, weights_in=w), brute_weighted_peaks(codes, 2, 0, w))  # the handle goes on
    # the arguments
    l = _lib.lib()
    labels, count = np.full(n, 7, dtype=np.uint32), C.c_uint64(9)
    for args, text in (((2, 0, None, labels.ctypes.data, None, None, n), b"NULL weights_in"),
                       ((2, 3, w.ctypes.data, labels.ctypes.data, None, None, n), b"radius 3 is larger than max_div 2"),
                       ((_lib.NONE, 0, w.ctypes.data, labels.ctypes.data, None, None, n), b"peaks need a bound"),
                       ((2, 0, w.ctypes.data, None, None, None, n), b"NULL labels"),
                       ((2, 0, w.ctypes.data, labels.ctypes.data, None, None, n - 1), b"labels holds")):
        assert l.smafa_db_self_peaks_weighted(store._h, *args, C.byref(count)) == _lib.ERR_INVALID
        assert b"smafa_db_self_peaks_weighted: " in l.smafa_last_error() and text in l.smafa_last_error(), l.smafa_last_error()
    assert (labels == 7).all() and count.value == 9  # nothing was written
    with pytest.raises(ValueError, match="weights_in has shape"):
        store.self_peaks(2, 0, weights_in=w[:-1])
    store.close()
    # one row, and none
    one = make_store(codes[:1], "nt")
    got = one.self_peaks(2, 0, weights_in=np.array([41], dtype=np.uint32))
    assert [a.tolist() for a in got[:3]] == [[0], [0], [41]] and got[3] == 1
    one.close()
    empty = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    got = empty.self_peaks(2, 0, weights_in=np.zeros(0, dtype=np.uint32))
    assert len(got[0]) == 0 and got[3] == 0
    empty.close()


def test_launch_form():
    codes = planted_store(6, "aa", 60, 100)
    n = len(codes)
    w = random_weights(n, 4)
    want = brute_weighted_peaks(codes, 5, 0, w)
    store = make_store(codes, "aa")
    d_w, d_count = DeviceArray(w), DeviceArray(np.full(1, 99, dtype=np.uint64))
    d_labels, d_parents, d_weights = (DeviceArray(np.full(n, 9, dtype=np.uint32)) for _ in range(3))
    store.self_peaks_weighted_launch(5, 0, d_w.ptr, d_labels.ptr, d_parents.ptr, d_weights.ptr, d_count.ptr)
    store.sync()
    same((d_labels.get(), d_parents.get(), d_weights.get(), int(d_count.get()[0])), want)
    store.self_peaks_weighted_launch(5, 0, d_w.ptr, d_labels.ptr, 0, 0, d_count.ptr)  # labels alone
    store.sync()
    assert d_labels.get().tobytes() == want[0].tobytes() and int(d_count.get()[0]) == want[3]
    for d in (d_w, d_count, d_labels, d_parents, d_weights):
        d.free()
    store.close()


def test_device_form():
    """smafa_db_self_peaks_weighted_launch on torch buffers — tests/peaks_weighted_worker.py, a process of its own: torch has to
    initialise HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "peaks_weighted_worker.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "weighted peaks device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---- the verb
def run_cli(*args, stdin=None):
    return subprocess.run([_lib.CLI_PATH, *args], input=stdin, capture_output=True)


def test_the_verb(golden, tmp_path):
    """`smafa peaks --sizes` on the distinct sequences of a FASTA with repeated records, lifted, equals `smafa peaks` on all of them"""
    records = [r.rstrip("\n") for r in open(golden + "/subjects.fa").read().split(">")[1:]]
    rng = np.random.default_rng(1)
    order = np.concatenate([np.arange(len(records)), rng.integers(0, len(records), size=len(records) // 2)])
    rng.shuffle(order)
    fa, db, u_fa, u_db = (str(tmp_path / f) for f in ("raw.fa", "raw.db", "u.fa", "u.db"))
    open(fa, "w").write("".join(">%d_%s\n" % (k, records[i]) for k, i in enumerate(order)))
    assert run_cli("makedb", "-i", fa, "-d", db).returncode == 0
    codes = smafa_amd.read_db(db)[1]
    unique_of, old_of_new, sizes = expected_derep(codes)
    assert len(old_of_new) < len(codes)
    open(u_fa, "w").write("".join(">%d_%s\n" % (k, records[order[k]]) for k in old_of_new))
    assert run_cli("makedb", "-i", u_fa, "-d", u_db).returncode == 0
    listed = "".join("%d\t%d\t%d\n" % (u, sizes[u], old_of_new[u]) for u in reversed(range(len(sizes)))).encode()  # any order, a third column
    want = run_cli("peaks", "-d", db, "--max-divergence", "3")
    got = run_cli("peaks", "-d", u_db, "--max-divergence", "3", "--sizes", "-", stdin=listed)
    assert want.returncode == 0 and got.returncode == 0, got.stderr
    u_rows = [line.split("\t") for line in got.stdout.decode().splitlines()]
    raw_rows = [line.split("\t") for line in want.stdout.decode().splitlines()]
    assert len(u_rows) == len(sizes) and len(raw_rows) == len(codes)
    for i, (_, label, _, weight) in enumerate(raw_rows):
        u = u_rows[unique_of[i]]
        assert int(label) == old_of_new[int(u[1])] and weight == u[3], i
    (tmp_path / "sizes.tsv").write_bytes(listed)
    again = run_cli("peaks", "-d", u_db, "--max-divergence", "3", "--sizes", str(tmp_path / "sizes.tsv"))
    assert again.returncode == 0 and again.stdout == got.stdout
    # failing runs exit non-zero and print nothing
    for stdin, text in ((b"0\tx\n", b"smafa_peaks_weighted: weights line 1"), (b"0\t1\n0\t2\n", b"a second line for this sequence"),
                        (b"%d\t1\n" % len(sizes), b"the sequence number is not one of the database's"),
                        (b"0\t4294967295\n1\t1\n", b"the weights sum to 4294967296")):
        r = run_cli("peaks", "-d", u_db, "--max-divergence", "3", "--sizes", "-", stdin=stdin)
        assert r.returncode == 1 and text in r.stderr and r.stdout == b"", r.stderr
    r = run_cli("peaks", "-d", u_db, "--max-divergence", "3", "--sizes", str(tmp_path / "nothing"))
    assert r.returncode == 1 and b"cannot open weights file" in r.stderr and r.stdout == b""

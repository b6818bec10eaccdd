"""The consensus call's entry points: exported symbols, the header as C99 and the NULL-handle checks without a GPU; with one,
every argument check in the documented order with its text, sentinels around every output ("nothing written"), the capacity
protocol, the illegal-label error, the empty store, all labels SMAFA_NONE, and the device form against the host form."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib
from consensus_cases import NONE, chunk_case, expected_consensus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_consensus_launch", "smafa_db_consensus", "smafa_consensus")
DECLARATIONS = (
    "int smafa_db_consensus_launch(smafa_db *db, const void *d_labels, void *d_ids, void *d_sizes, void *d_codes, "
    "void *d_nearest /* may be NULL */, void *d_div /* may be NULL */, uint64_t cap_clusters, uint64_t *n_clusters /* host */);",
    "int smafa_db_consensus(smafa_db *db, const uint32_t *labels, uint32_t *ids, uint32_t *sizes, uint8_t *codes, uint32_t *nearest, "
    "uint32_t *div, uint64_t cap_clusters, uint64_t *n_clusters);",
    "int smafa_consensus(const char *db_path, const char *labels_path, int out_fd, int device);",
)
gpu = pytest.mark.gpu


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.consensus)
    assert callable(smafa_amd.SubjectStore.cluster_consensus) and callable(smafa_amd.SubjectStore.cluster_consensus_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_components_update(") < text.index("smafa_db_consensus_launch(")  # behind the self-store calls
    assert "a tie goes to the smallest code" in text and "SMAFA_CONSENSUS_CHUNK" in text


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, const void *, void *, void *, void *, void *, void *, uint64_t, uint64_t *) = "
                   "smafa_db_consensus_launch;\n"
                   "int (*const host_form)(smafa_db *, const uint32_t *, uint32_t *, uint32_t *, uint8_t *, uint32_t *, uint32_t *, uint64_t, "
                   "uint64_t *) = smafa_db_consensus;\n"
                   "int (*const file_form)(const char *, const char *, int, int) = smafa_consensus;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_and_paths_are_invalid():
    l = _lib.lib()
    count = C.c_uint64(9)
    labels = np.zeros(4, dtype=np.uint32)
    assert l.smafa_db_consensus(None, labels.ctypes.data, None, None, None, None, None, 0, C.byref(count)) == _lib.ERR_INVALID
    assert b"smafa_db_consensus: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_consensus_launch(None, None, None, None, None, None, None, 0, None) == _lib.ERR_INVALID
    assert b"smafa_db_consensus_launch: NULL handle" in l.smafa_last_error() and count.value == 9
    assert l.smafa_consensus(None, b"-", 1, 0) == _lib.ERR_INVALID and b"NULL path" in l.smafa_last_error()
    assert l.smafa_consensus(b"/nonexistent", None, 1, 0) == _lib.ERR_INVALID and b"NULL labels path" in l.smafa_last_error()


def test_help_and_usage_name_the_verb():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"consensus -d, --database <FILE>  --labels <FILE|->" in r.stdout
    assert b"label<TAB>size<TAB>nearest<TAB>max_div<TAB>SEQUENCE" in r.stdout
    r = subprocess.run([_lib.CLI_PATH, "consensus", "--labels", "-"], capture_output=True)
    assert r.returncode == 2 and b"consensus needs --database" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "components", "-d", "x", "--max-divergence", "2", "--labels", "-"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --labels" in r.stderr  # the flag belongs to `consensus` alone


class Outputs:
    """every output of the host form between sentinels: K entries asked for, a guard entry on each side of every array"""

    def __init__(self, K, n, L):
        self.K, self.n, self.L = K, n, L
        self.ids, self.sizes, self.nearest = (np.full(K + 2, 5, dtype=np.uint32) for _ in range(3))
        self.div = np.full(n + 2, 5, dtype=np.uint32)
        self.codes = np.full((K + 2) * L, 5, dtype=np.uint8)
        self.count = C.c_uint64(9)

    def args(self, nearest=True, div=True):
        inner = lambda a, step=1: a.ctypes.data + step * a.itemsize  # noqa: E731
        return (inner(self.ids), inner(self.sizes), inner(self.codes, self.L), inner(self.nearest) if nearest else None,
                inner(self.div) if div else None)

    def untouched(self):
        return all((a == 5).all() for a in (self.ids, self.sizes, self.nearest, self.div, self.codes)) and self.count.value == 9

    def guards_hold(self):
        return all(a[0] == 5 and a[-1] == 5 for a in (self.ids, self.sizes, self.nearest, self.div)) and \
            (self.codes[: self.L] == 5).all() and (self.codes[-self.L:] == 5).all()

    def arrays(self):
        return (self.ids[1:-1], self.sizes[1:-1], self.codes[self.L: -self.L].reshape(self.K, self.L), self.nearest[1:-1], self.div[1:-1])


@pytest.fixture()
def case():
    codes, labellings = chunk_case()
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_NT)
    store.push(codes)
    yield store, codes, labellings["random"]
    store.close()


@gpu
def test_argument_checks_in_order(case):
    """handle, labels, n_clusters, then ids, sizes and codes while a capacity is given: with several arguments wrong the first
    of these is the one named, in both forms, and nothing is written"""
    store, codes, labels = case
    l = _lib.lib()
    want = expected_consensus(codes, labels)
    K = len(want[0])
    o = Outputs(K, *codes.shape)
    ids, sizes, cons, nearest, div = o.args()
    p = labels.ctypes.data
    for form, who in ((l.smafa_db_consensus, b"smafa_db_consensus"), (l.smafa_db_consensus_launch, b"smafa_db_consensus_launch")):
        for args, text in (((None, None, None, None, None, None, K, None), b"NULL labels"),
                           ((p, None, None, None, None, None, K, None), b"NULL n_clusters"),
                           ((p, None, None, None, nearest, div, K, C.byref(o.count)), b"NULL ids"),
                           ((p, ids, None, None, nearest, div, K, C.byref(o.count)), b"NULL sizes"),
                           ((p, ids, sizes, None, nearest, div, K, C.byref(o.count)), b"NULL codes")):
            assert form(store._h, *args) == _lib.ERR_INVALID
            assert who + b": " + text in l.smafa_last_error(), l.smafa_last_error()
            assert o.untouched()


@gpu
def test_capacity_reports_k_and_the_retry_succeeds(case):
    store, codes, labels = case
    l = _lib.lib()
    want = expected_consensus(codes, labels)
    K = len(want[0])
    o = Outputs(K, *codes.shape)
    p = labels.ctypes.data
    assert l.smafa_db_consensus(store._h, p, None, None, None, None, None, 0, C.byref(o.count)) == _lib.ERR_CAPACITY  # asking for K
    assert o.count.value == K and b"%d clusters, capacity 0" % K in l.smafa_last_error()
    o.count.value = 9
    assert l.smafa_db_consensus(store._h, p, *o.args(), K - 1, C.byref(o.count)) == _lib.ERR_CAPACITY
    assert o.count.value == K
    o.count.value = 9
    assert o.untouched()
    assert l.smafa_db_consensus(store._h, p, *o.args(), K, C.byref(o.count)) == _lib.OK
    assert o.count.value == K and o.guards_hold()
    assert all(g.tobytes() == w.tobytes() for g, w in zip(o.arrays(), want))
    # the optional outputs left out, and a capacity above K: entries from K on stay as they were
    o = Outputs(K + 3, *codes.shape)
    assert l.smafa_db_consensus(store._h, p, *o.args(nearest=False, div=False), K + 3, C.byref(o.count)) == _lib.OK
    got = o.arrays()
    assert o.count.value == K and (o.nearest == 5).all() and (o.div == 5).all() and o.guards_hold()
    assert all(g[:K].tobytes() == w.tobytes() and (g[K:] == 5).all() for g, w in zip(got[:3], want[:3]))


@gpu
def test_an_illegal_label_names_the_smallest_row(case):
    store, codes, labels = case
    l = _lib.lib()
    n = len(codes)
    o = Outputs(n, *codes.shape)
    bad = labels.copy()
    bad[[1400, 33, 700]] = [n, n + 7, 0xFFFFFFFE]
    for _ in range(2):  # the same text every run
        assert l.smafa_db_consensus(store._h, bad.ctypes.data, *o.args(), n, C.byref(o.count)) == _lib.ERR_INVALID
        assert b"smafa_db_consensus: labels[33] is %d," % (n + 7) in l.smafa_last_error(), l.smafa_last_error()
        assert o.untouched()
    bad[33] = n - 1  # legal, and nobody's own label before
    assert l.smafa_db_consensus(store._h, bad.ctypes.data, *o.args(), n, C.byref(o.count)) == _lib.ERR_INVALID
    assert b"labels[700] is 4294967294," in l.smafa_last_error() and o.untouched()


@gpu
def test_empty_store_and_all_none():
    l = _lib.lib()
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    o = Outputs(4, 4, 60)
    labels = np.full(4, NONE, dtype=np.uint32)
    assert l.smafa_db_consensus(store._h, labels.ctypes.data, *o.args(), 4, C.byref(o.count)) == _lib.OK
    assert o.count.value == 0
    o.count.value = 9
    assert o.untouched()  # an empty store: the count and nothing else
    store.push(np.zeros((4, 60), dtype=np.uint8))
    assert l.smafa_db_consensus(store._h, labels.ctypes.data, *o.args(), 4, C.byref(o.count)) == _lib.OK
    assert o.count.value == 0 and (o.div[1:-1] == NONE).all() and o.guards_hold()
    assert all((a == 5).all() for a in (o.ids, o.sizes, o.nearest, o.codes))
    assert l.smafa_db_consensus(store._h, labels.ctypes.data, None, None, None, None, None, 0, C.byref(o.count)) == _lib.OK  # K = 0 fits
    store.close()


@gpu
def test_device_form_equals_the_host_form():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "consensus_worker.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "consensus device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]

"""The chimera check's entry points: exported symbols, the header as C99, the NULL-handle checks and the help text without a GPU;
with one, every argument check in the documented order with its text, sentinels around every output ("nothing written"), NULL
optional arrays, the empty store and one row, and the device form against the host form and the model."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib
from chimera_cases import NONE, expected, planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_self_chimeras_launch", "smafa_db_self_chimeras", "smafa_chimeras")
DECLARATIONS = (
    "int smafa_db_self_chimeras_launch(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t min_fold, "
    "const void *d_weights_in /* may be NULL */, void *d_flags, void *d_left_parent, void *d_left_len, void *d_right_parent, "
    "void *d_right_len, void *d_weights /* the last five may be NULL */, void *d_n_chimeras /* uint64 */);",
    "int smafa_db_self_chimeras(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t min_fold, const uint32_t *weights_in, "
    "uint32_t *flags, uint32_t *left_parent, uint32_t *left_len, uint32_t *right_parent, uint32_t *right_len, uint32_t *weights, "
    "uint64_t cap, uint64_t *n_chimeras);",
    "int smafa_chimeras(const char *db_path, uint32_t max_divergence, uint32_t radius, uint32_t min_fold, const char *weights_path, "
    "int out_fd, int device);",
)
FIELDS = ("flags", "left_parent", "left_len", "right_parent", "right_len", "weights")
gpu = pytest.mark.gpu


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.chimeras)
    assert callable(smafa_amd.SubjectStore.self_chimeras) and callable(smafa_amd.SubjectStore.self_chimeras_launch)
    assert smafa_amd.Chimeras._fields == FIELDS + ("n_chimeras",)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_peaks(") < text.index("smafa_db_self_chimeras_launch(")  # behind the call whose weights it shares
    # what the issue asks the header to state
    for phrase in ("One parent can never satisfy", "always has two distinct parents", "reproduces q as left_parent[:b] + right_parent[b:]",
                   "D has to be at least the divergence of the parents", "Checks, in this order"):
        assert phrase in " ".join(text.replace(" * ", " ").split()), phrase


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, uint32_t, uint32_t, const void *, void *, void *, void *, void *, void *, "
                   "void *, void *) = smafa_db_self_chimeras_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, uint32_t, uint32_t, const uint32_t *, uint32_t *, uint32_t *, uint32_t *, "
                   "uint32_t *, uint32_t *, uint32_t *, uint64_t, uint64_t *) = smafa_db_self_chimeras;\n"
                   "int (*const file_form)(const char *, uint32_t, uint32_t, uint32_t, const char *, int, int) = smafa_chimeras;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_and_paths_are_invalid():
    l = _lib.lib()
    count = C.c_uint64(9)
    flags = np.full(4, 5, dtype=np.uint32)
    assert l.smafa_db_self_chimeras(None, 3, 0, 2, None, flags.ctypes.data, None, None, None, None, None, 4, C.byref(count)) == _lib.ERR_INVALID
    assert b"smafa_db_self_chimeras: NULL handle" in l.smafa_last_error() and count.value == 9 and (flags == 5).all()
    assert l.smafa_db_self_chimeras_launch(None, 3, 0, 2, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_chimeras_launch: NULL handle" in l.smafa_last_error()
    assert l.smafa_chimeras(None, 3, 0, 2, None, 1, 0) == _lib.ERR_INVALID and b"smafa_chimeras: NULL path" in l.smafa_last_error()
    assert l.smafa_chimeras(b"/nonexistent", _lib.NONE, 0, 2, None, 1, 0) == _lib.ERR_INVALID and b"bound" in l.smafa_last_error()
    assert l.smafa_chimeras(b"/nonexistent", 2, 3, 2, None, 1, 0) == _lib.ERR_INVALID and b"radius 3" in l.smafa_last_error()
    assert l.smafa_chimeras(b"/nonexistent", 2, 0, 0, None, 1, 0) == _lib.ERR_INVALID and b"min_fold" in l.smafa_last_error()


def test_help_and_usage_name_the_verb():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0
    assert b"chimeras -d, --database <FILE>  --max-divergence <INT>  [--min-fold <INT>] [--radius <INT>] [--weights <FILE|->]" in r.stdout
    assert b"i<TAB>flag<TAB>left_parent<TAB>left_len<TAB>right_parent<TAB>right_len<TAB>weight" in r.stdout
    r = subprocess.run([_lib.CLI_PATH, "chimeras", "--max-divergence", "3"], capture_output=True)
    assert r.returncode == 2 and b"chimeras needs --database" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "chimeras", "-d", "x"], capture_output=True)
    assert r.returncode == 2 and b"chimeras needs --max-divergence" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "chimeras", "-d", "x", "--max-divergence", "3", "--min-fold", "0"], capture_output=True)
    assert r.returncode == 2 and b"--min-fold needs a positive integer" in r.stderr
    for flag in ("--weights", "--min-fold"):  # the flags belong to `chimeras` alone
        r = subprocess.run([_lib.CLI_PATH, "peaks", "-d", "x", "--max-divergence", "2", flag, "1"], capture_output=True)
        assert r.returncode == 2 and b"unexpected argument " + flag.encode() in r.stderr


class Outputs:
    """every output of the host form between sentinels: n entries asked for, a guard entry on each side of every array"""

    def __init__(self, n):
        self.n = n
        self.arrays = [np.full(n + 2, 5, dtype=np.uint32) for _ in range(6)]
        self.count = C.c_uint64(9)

    def args(self, optional=True):
        inner = [a.ctypes.data + a.itemsize for a in self.arrays]
        return [inner[0]] + [p if optional else None for p in inner[1:]]

    def untouched(self):
        return all((a == 5).all() for a in self.arrays) and self.count.value == 9

    def guards_hold(self):
        return all(a[0] == 5 and a[-1] == 5 for a in self.arrays)

    def inner(self):
        return [a[1:-1] for a in self.arrays]


@pytest.fixture()
def case():
    codes = planted("nt60")[0]
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_NT)
    store.push(codes)
    yield store, codes, expected("nt60", 3, 0, 2)
    store.close()


@gpu
def test_argument_checks_in_order(case):
    """handle, flags, n_chimeras, max_div, radius, min_fold, then (host form) cap: with several arguments wrong the first of these
    is the one named, in both forms, and nothing is written — the count included"""
    store, codes, _ = case
    l = _lib.lib()
    n = len(codes)
    o = Outputs(n)
    flags, *rest = o.args()
    cnt = C.byref(o.count)
    # (max_div, radius, min_fold, flags, has count) -> text; every later argument is wrong as well, the capacity (n - 1) too
    for (D, r, F, fl, has_count), text in (((_lib.NONE, 7, 0, None, False), b"NULL flags"),
                                           ((_lib.NONE, 7, 0, flags, False), b"NULL n_chimeras"),
                                           ((_lib.NONE, 7, 0, flags, True), b"(max_div)"),
                                           ((3, 7, 0, flags, True), b"radius 7 is larger than max_div 3"),
                                           ((3, 3, 0, flags, True), b"min_fold is 0"),
                                           ((3, _lib.NONE, 1, flags, True), b"cap: flags holds %d entries" % (n - 1))):
        assert l.smafa_db_self_chimeras(store._h, D, r, F, None, fl, *rest, n - 1, cnt if has_count else None) == _lib.ERR_INVALID
        assert b"smafa_db_self_chimeras: " in l.smafa_last_error() and text in l.smafa_last_error(), l.smafa_last_error()
        assert o.untouched()
        if text.startswith(b"cap"):
            continue
        assert l.smafa_db_self_chimeras_launch(store._h, D, r, F, None, fl, *rest, cnt if has_count else None) == _lib.ERR_INVALID
        assert b"smafa_db_self_chimeras_launch: " in l.smafa_last_error() and text in l.smafa_last_error(), l.smafa_last_error()
        assert o.untouched()


@gpu
def test_outputs_between_sentinels_and_null_optional_arrays(case):
    store, codes, want = case
    l = _lib.lib()
    n = len(codes)
    o = Outputs(n)
    assert l.smafa_db_self_chimeras(store._h, 3, 0, 2, None, *o.args(), n, C.byref(o.count)) == _lib.OK
    assert o.count.value == want.n_chimeras and o.guards_hold()
    assert all(g.tobytes() == getattr(want, f).tobytes() for g, f in zip(o.inner(), FIELDS))
    o = Outputs(n)
    assert l.smafa_db_self_chimeras(store._h, 3, 0, 2, None, *o.args(optional=False), n + 1, C.byref(o.count)) == _lib.OK  # a capacity above n
    assert o.count.value == want.n_chimeras and o.inner()[0].tobytes() == want.flags.tobytes() and o.guards_hold()
    assert all((a == 5).all() for a in o.arrays[1:])
    # each optional array alone
    for k in range(1, 6):
        o = Outputs(n)
        args = o.args(optional=False)
        args[k] = o.arrays[k].ctypes.data + 4
        assert l.smafa_db_self_chimeras(store._h, 3, 0, 2, None, *args, n, C.byref(o.count)) == _lib.OK
        assert o.inner()[k].tobytes() == getattr(want, FIELDS[k]).tobytes() and o.guards_hold()
        assert all((a == 5).all() for j, a in enumerate(o.arrays) if j not in (0, k))
    # weights_in is read, never written
    given = want.weights.copy()
    o = Outputs(n)
    assert l.smafa_db_self_chimeras(store._h, 3, 0, 2, given.ctypes.data, *o.args(), n, C.byref(o.count)) == _lib.OK
    assert given.tobytes() == want.weights.tobytes() and o.inner()[5].tobytes() == given.tobytes() and o.count.value == want.n_chimeras


@gpu
def test_empty_store_and_one_row():
    l = _lib.lib()
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    o = Outputs(4)
    assert l.smafa_db_self_chimeras(store._h, 3, 0, 2, None, *o.args(), 4, C.byref(o.count)) == _lib.OK
    assert o.count.value == 0
    o.count.value = 9
    assert o.untouched()  # an empty store: the count and nothing else
    store.push(np.zeros((1, 60), dtype=np.uint8))
    assert l.smafa_db_self_chimeras(store._h, 3, 0, 2, None, *o.args(), 4, C.byref(o.count)) == _lib.OK
    assert o.count.value == 0 and o.guards_hold()
    assert [int(a[1]) for a in o.arrays] == [0, NONE, 0, NONE, 0, 1] and all((a[2:] == 5).all() for a in o.arrays)
    store.close()


@gpu
def test_device_form_equals_the_host_form():
    """chimera::init_sides_kernel, chimera::offer_sides_kernel and chimera::verdict_kernel on the caller's device buffers"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chimera_worker.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "chimeras device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]

"""The neighbours call's entry points without a GPU: exported symbols, the header as C99, argument checks, the CLI's `neighbours`."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import smafa_amd
from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_self_neighbours_launch", "smafa_db_self_neighbours", "smafa_neighbours")
DECLARATIONS = (
    "int smafa_db_self_neighbours_launch(smafa_db *db, uint32_t max_div, uint32_t max_num_hits, "
    "void *d_offsets /* n_subjects + 1 uint64 */, void *d_neighbours /* cap uint32, may be NULL if cap == 0 */, "
    "void *d_dists /* cap uint32 or NULL */, uint64_t cap, void *d_total /* uint64 */);",
    "int smafa_db_self_neighbours(smafa_db *db, uint32_t max_div, uint32_t max_num_hits, uint64_t *offsets, uint32_t *neighbours, "
    "uint32_t *dists /* may be NULL */, uint64_t cap, uint64_t *n_out);",
    "int smafa_neighbours(const char *db_path, uint32_t max_divergence, uint32_t max_num_hits, int out_fd, int device);",
)


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.neighbours) and callable(smafa_amd.SubjectStore.self_neighbours)
    assert callable(smafa_amd.SubjectStore.self_neighbours_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_peaks(") < text.index("smafa_db_self_neighbours_launch(")  # after the peaks section
    for phrase in ("ordered by (distance, j) ascending", "ties at the cut go to the smaller subject number",
                   "offsets[n_subjects] = total", "SMAFA_NEIGHBOUR_SORT", "max_div >= seq_len is no shortcut", "2^31 - 1 entries"):
        assert phrase in text, phrase


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, uint32_t, void *, void *, void *, uint64_t, void *) = "
                   "smafa_db_self_neighbours_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, uint32_t, uint64_t *, uint32_t *, uint32_t *, uint64_t, uint64_t *) = "
                   "smafa_db_self_neighbours;\n"
                   "int (*const file_form)(const char *, uint32_t, uint32_t, int, int) = smafa_neighbours;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_invalid_arguments_name_themselves_and_write_nothing():
    """the argument checks run in front of anything that needs the handle, so every one of them is reachable without a device"""
    l = _lib.lib()
    n_out = (C.c_uint64 * 1)(9)
    offsets = (C.c_uint64 * 4)(7, 7, 7, 7)
    nb = (C.c_uint32 * 4)(7, 7, 7, 7)
    for form, total_name in (("smafa_db_self_neighbours", b"NULL n_out"), ("smafa_db_self_neighbours_launch", b"NULL total")):
        f = getattr(l, form)
        for args, word in (((None, 5, 3, offsets, nb, None, 4, n_out), b"NULL handle"),
                           ((None, 5, 3, None, nb, None, 4, n_out), b"NULL offsets"),
                           ((None, 5, 3, offsets, nb, None, 4, None), total_name),
                           ((None, 5, 3, offsets, None, None, 4, n_out), b"NULL neighbours with a capacity"),
                           ((None, _lib.NONE, 3, offsets, nb, None, 4, n_out), b"bound (max_div)"),
                           ((None, 5, 0, offsets, nb, None, 4, n_out), b"max_num_hits is 0")):
            assert f(*args) == _lib.ERR_INVALID, (form, word)
            assert form.encode() + b": " in l.smafa_last_error() and word in l.smafa_last_error(), l.smafa_last_error()
            assert list(n_out) == [9] and list(offsets) == [7] * 4 and list(nb) == [7] * 4
    assert l.smafa_neighbours(None, 5, _lib.NONE, 1, 0) == _lib.ERR_INVALID
    assert b"NULL path" in l.smafa_last_error()
    assert l.smafa_neighbours(b"/nonexistent", _lib.NONE, _lib.NONE, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert l.smafa_neighbours(b"/nonexistent", 2, 0, 1, 0) == _lib.ERR_INVALID
    assert b"max_num_hits is 0" in l.smafa_last_error()
    assert l.smafa_neighbours(b"/nonexistent", 2, _lib.NONE, 1, 0) != _lib.ERR_INVALID  # no cut: the path fails, not the cut


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGA\n>b\nACGTACGT\n>c\nTTTTACGA\n>d\nACGTACGT\n")
    smafa_amd.makedb(fa, path)
    return path


def test_neighbours_without_a_gpu_says_so(db):
    args = [_lib.CLI_PATH, "neighbours", "-d", db, "--max-divergence", "1"]
    if smafa_amd.device_count() > 0:
        # b = d, a at 1 of both, c far from all
        r = subprocess.run(args, capture_output=True)
        assert r.returncode == 0 and r.stdout == b"0\t1\t1\n0\t3\t1\n1\t3\t0\n1\t0\t1\n3\t1\t0\n3\t0\t1\n", r.stderr
        r = subprocess.run(args + ["--max-num-hits", "1"], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"0\t1\t1\n1\t3\t0\n3\t1\t0\n", r.stderr
        return
    r = subprocess.run(args, capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.neighbours(db, 1)
    assert e.value.code == _lib.ERR_DEVICE


def test_neighbours_usage_errors(db):
    r = subprocess.run([_lib.CLI_PATH, "neighbours", "-d", db], capture_output=True)
    assert r.returncode == 2 and b"neighbours needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "neighbours", "--max-divergence", "2"], capture_output=True)
    assert r.returncode == 2 and b"neighbours needs --database" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "neighbours", "-d", db, "--max-divergence", "2", "--max-num-hits", "x"], capture_output=True)
    assert r.returncode == 2 and b"--max-num-hits needs an unsigned integer" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "neighbours", "-d", db, "--max-divergence", "2", "--max-num-hits", "0"], capture_output=True)
    assert r.returncode == 2 and b"--max-num-hits needs a positive integer" in r.stderr and r.stdout == b""


def test_help_names_the_command():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"neighbours -d, --database <FILE>  --max-divergence <INT>  [--max-num-hits <INT>]" in r.stdout
    assert b"i<TAB>j<TAB>divergence" in r.stdout

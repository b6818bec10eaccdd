"""The peaks call's entry points without a GPU: exported symbols, the header as C99, argument checks, the CLI's `peaks`."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import smafa_amd
from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_self_peaks_launch", "smafa_db_self_peaks", "smafa_peaks")
DECLARATIONS = (
    "int smafa_db_self_peaks_launch(smafa_db *db, uint32_t max_div, uint32_t radius, void *d_labels, "
    "void *d_parents /* may be NULL */, void *d_weights /* may be NULL */, void *d_n_peaks /* uint64 */);",
    "int smafa_db_self_peaks(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t *labels, "
    "uint32_t *parents /* may be NULL */, uint32_t *weights /* may be NULL */, uint64_t cap, uint64_t *n_peaks);",
    "int smafa_peaks(const char *db_path, uint32_t max_divergence, uint32_t radius, int out_fd, int device);",
)


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.peaks) and callable(smafa_amd.SubjectStore.self_peaks)
    assert callable(smafa_amd.SubjectStore.self_peaks_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_density(") < text.index("smafa_db_self_peaks_launch(")  # after the density section
    for phrase in ("weight[i]", "key(i)", "parent[i]", "makes i a PEAK", "labels[labels[i]] == labels[i]", "need not be <= i",
                   "radius = SMAFA_NONE means r = D", "SMAFA_DENSITY_KEEP_MAX is the capacity of that one shared list",
                   "at most 33 rounds"):
        assert phrase in text, phrase


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, uint32_t, void *, void *, void *, void *) = "
                   "smafa_db_self_peaks_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, uint32_t, uint32_t *, uint32_t *, uint32_t *, uint64_t, uint64_t *) = "
                   "smafa_db_self_peaks;\n"
                   "int (*const file_form)(const char *, uint32_t, uint32_t, int, int) = smafa_peaks;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_invalid():
    l = _lib.lib()
    count = (C.c_uint64 * 1)(9)
    labels = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert l.smafa_db_self_peaks(None, 5, 0, labels, None, None, 4, count) == _lib.ERR_INVALID
    assert b"smafa_db_self_peaks: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_peaks_launch(None, 5, 0, None, None, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_peaks_launch: NULL handle" in l.smafa_last_error()
    assert list(count) == [9] and list(labels) == [7, 7, 7, 7]
    assert l.smafa_peaks(None, 5, 0, 1, 0) == _lib.ERR_INVALID
    assert b"NULL path" in l.smafa_last_error()
    assert l.smafa_peaks(b"/nonexistent", _lib.NONE, 0, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert l.smafa_peaks(b"/nonexistent", 2, 3, 1, 0) == _lib.ERR_INVALID
    assert b"radius 3" in l.smafa_last_error()
    assert l.smafa_peaks(b"/nonexistent", 2, _lib.NONE, 1, 0) != _lib.ERR_INVALID  # radius NONE is r = D: the path fails, not the radius


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGA\n>b\nACGTACGT\n>c\nTTTTACGA\n>d\nACGTACGT\n")
    smafa_amd.makedb(fa, path)
    return path


def test_peaks_without_a_gpu_says_so(db):
    args = [_lib.CLI_PATH, "peaks", "-d", db, "--max-divergence", "1"]
    if smafa_amd.device_count() > 0:
        # b = d, a at 1 of both, c far from all: abundances 1, 2, 1, 2; a climbs to b, the smaller copy; c is a peak of its own
        r = subprocess.run(args, capture_output=True)
        assert r.returncode == 0 and r.stdout == b"0\t1\t1\t1\n1\t1\t1\t2\n2\t2\t2\t1\n3\t1\t1\t2\n", r.stderr
        r = subprocess.run(args + ["--radius", "1"], capture_output=True)  # ball counts 3, 3, 1, 3: the tie goes to a
        assert r.returncode == 0 and r.stdout == b"0\t0\t0\t3\n1\t0\t0\t3\n2\t2\t2\t1\n3\t0\t0\t3\n", r.stderr
        return
    r = subprocess.run(args, capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.peaks(db, 1)
    assert e.value.code == _lib.ERR_DEVICE


def test_peaks_usage_errors(db):
    r = subprocess.run([_lib.CLI_PATH, "peaks", "-d", db], capture_output=True)
    assert r.returncode == 2 and b"peaks needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "peaks", "--max-divergence", "2"], capture_output=True)
    assert r.returncode == 2 and b"peaks needs --database" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "peaks", "-d", db, "--max-divergence", "2", "--radius", "x"], capture_output=True)
    assert r.returncode == 2 and b"--radius needs an unsigned integer" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "peaks", "-d", db, "--max-divergence", "2", "--radius", "3"], capture_output=True)
    assert r.returncode == 1 and b"radius 3 is larger" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "density", "-d", db, "--max-divergence", "2", "--min-pts", "3", "--radius", "1"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --radius" in r.stderr  # the flag belongs to `peaks` alone


def test_help_names_the_command():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"peaks   -d, --database <FILE>  --max-divergence <INT>  [--radius <INT>]" in r.stdout
    assert b"i<TAB>label<TAB>parent<TAB>weight" in r.stdout

"""The density call's entry points without a GPU: exported symbols, the header as C99, argument checks, the CLI's
`density`."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import smafa_amd
from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_self_density_launch", "smafa_db_self_density", "smafa_density")
DECLARATIONS = (
    "int smafa_db_self_density_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, void *d_labels, "
    "void *d_degrees /* may be NULL */, void *d_counts /* 3 x uint64 */);",
    "int smafa_db_self_density(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t *labels, "
    "uint32_t *degrees /* may be NULL */, uint64_t cap, uint64_t counts[3]);",
    "int smafa_density(const char *db_path, uint32_t max_divergence, uint32_t min_pts, int out_fd, int device);",
)


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.density) and callable(smafa_amd.SubjectStore.self_density)
    assert callable(smafa_amd.SubjectStore.self_density_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_levels(") < text.index("smafa_db_self_density_launch(")  # after the levels' section
    for phrase in ("degree[i] + 1 >= min_pts", "smallest CORE subject number", "for CORE rows only", "SMAFA_DENSITY_KEEP_MAX",
                   "min_pts <= 1", "min_pts == 2"):
        assert phrase in text, phrase


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, uint32_t, void *, void *, void *) = smafa_db_self_density_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, uint32_t, uint32_t *, uint32_t *, uint64_t, uint64_t *) = "
                   "smafa_db_self_density;\n"
                   "int (*const file_form)(const char *, uint32_t, uint32_t, int, int) = smafa_density;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_invalid():
    l = _lib.lib()
    counts = (C.c_uint64 * 3)(9, 9, 9)
    labels = (C.c_uint32 * 4)()
    assert l.smafa_db_self_density(None, 5, 3, labels, None, 4, counts) == _lib.ERR_INVALID
    assert b"smafa_db_self_density: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_density_launch(None, 5, 3, None, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_density_launch: NULL handle" in l.smafa_last_error()
    assert list(counts) == [9, 9, 9]
    assert l.smafa_density(None, 5, 3, 1, 0) == _lib.ERR_INVALID
    assert b"NULL path" in l.smafa_last_error()
    assert l.smafa_density(b"/nonexistent", _lib.NONE, 3, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGT\n>b\nACGTACGA\n>c\nTTTTACGA\n>d\nACGTACGT\n")
    smafa_amd.makedb(fa, path)
    return path


def test_density_without_a_gpu_says_so(db):
    if smafa_amd.device_count() > 0:
        r = subprocess.run([_lib.CLI_PATH, "density", "-d", db, "--max-divergence", "1", "--min-pts", "3"], capture_output=True)
        # a = d, b at 1 of both, c at 3 of b: a, b, d have two neighbours and are core; c is noise
        assert r.returncode == 0 and r.stdout == b"0\t0\t2\n1\t0\t2\n2\t-1\t0\n3\t0\t2\n", r.stderr
        return
    r = subprocess.run([_lib.CLI_PATH, "density", "-d", db, "--max-divergence", "1", "--min-pts", "3"], capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.density(db, 1, 3)
    assert e.value.code == _lib.ERR_DEVICE


def test_density_usage_errors(db):
    r = subprocess.run([_lib.CLI_PATH, "density", "-d", db, "--min-pts", "3"], capture_output=True)
    assert r.returncode == 2 and b"density needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "density", "-d", db, "--max-divergence", "2"], capture_output=True)
    assert r.returncode == 2 and b"density needs --min-pts" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "density", "--max-divergence", "2", "--min-pts", "3"], capture_output=True)
    assert r.returncode == 2 and b"density needs --database" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "components", "-d", db, "--max-divergence", "2", "--min-pts", "3"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --min-pts" in r.stderr  # the flag belongs to `density` alone


def test_help_names_the_command():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"density -d, --database <FILE>  --max-divergence <INT>  --min-pts <INT>" in r.stdout
    assert b"-1 for noise" in r.stdout

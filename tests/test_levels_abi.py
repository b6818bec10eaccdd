"""The levels' entry points without a GPU: exported symbols, the header as C99, argument checks, the CLI's
`components --levels`."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import smafa_amd
from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_self_levels_launch", "smafa_db_self_levels", "smafa_component_levels")
DECLARATIONS = (
    "int smafa_db_self_levels_launch(smafa_db *db, uint32_t max_div, void *d_labels, void *d_n_components);",
    "int smafa_db_self_levels(smafa_db *db, uint32_t max_div, uint32_t *labels, uint64_t cap, uint64_t *n_components);",
    "int smafa_component_levels(const char *db_path, uint32_t max_divergence, int out_fd, int device);",
)


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.component_levels) and callable(smafa_amd.SubjectStore.self_component_levels)
    assert callable(smafa_amd.SubjectStore.self_component_levels_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_components(") < text.index("smafa_db_self_levels_launch(")  # after the components' section
    assert "level-major" in text


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, void *, void *) = smafa_db_self_levels_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, uint32_t *, uint64_t, uint64_t *) = smafa_db_self_levels;\n"
                   "int (*const file_form)(const char *, uint32_t, int, int) = smafa_component_levels;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_invalid():
    l = _lib.lib()
    counts = (C.c_uint64 * 6)()
    labels = (C.c_uint32 * 24)()
    assert l.smafa_db_self_levels(None, 5, labels, 24, counts) == _lib.ERR_INVALID
    assert b"smafa_db_self_levels: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_levels_launch(None, 5, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_levels_launch: NULL handle" in l.smafa_last_error()
    assert l.smafa_component_levels(None, 5, 1, 0) == _lib.ERR_INVALID
    assert b"NULL path" in l.smafa_last_error()
    assert l.smafa_component_levels(b"/nonexistent", _lib.NONE, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGT\n>b\nACGTACGA\n>c\nTTTTACGA\n")
    smafa_amd.makedb(fa, path)
    return path


def test_levels_without_a_gpu_says_so(db):
    if smafa_amd.device_count() > 0:
        r = subprocess.run([_lib.CLI_PATH, "components", "-d", db, "--max-divergence", "3", "--levels"], capture_output=True)
        # a-b at 1, b-c at 3, a-c at 4
        assert r.returncode == 0 and r.stdout == b"0\t0\t0\t0\t0\n1\t1\t0\t0\t0\n2\t2\t2\t2\t0\n", r.stderr
        return
    r = subprocess.run([_lib.CLI_PATH, "components", "-d", db, "--max-divergence", "2", "--levels"], capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.component_levels(db, 2)
    assert e.value.code == _lib.ERR_DEVICE


def test_levels_usage_errors(db):
    r = subprocess.run([_lib.CLI_PATH, "components", "-d", db, "--levels"], capture_output=True)
    assert r.returncode == 2 and b"components needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "components", "--max-divergence", "2", "--levels"], capture_output=True)
    assert r.returncode == 2 and b"components needs --database" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", "2", "--levels"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --levels" in r.stderr  # the flag belongs to `components` alone


def test_help_names_the_flag():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"--levels" in r.stdout
    assert b"components -d, --database <FILE>  --max-divergence <INT>" in r.stdout

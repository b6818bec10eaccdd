"""The forest's entry points without a GPU: exported symbols, the header as C99, argument checks, the CLI's `forest`."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_self_forest_launch", "smafa_db_self_forest", "smafa_forest")
DECLARATIONS = (
    "int smafa_db_self_forest_launch(smafa_db *db, uint32_t max_div, void *d_edges /* n_subjects - 1 smafa_hit */, "
    "void *d_level_ends /* max_div + 1 uint64 */);",
    "int smafa_db_self_forest(smafa_db *db, uint32_t max_div, smafa_hit *edges, uint64_t cap, uint64_t *level_ends);",
    "int smafa_forest(const char *db_path, uint32_t max_divergence, int out_fd, int device);",
)


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.forest) and callable(smafa_amd.forest_linkage)
    assert callable(smafa_amd.SubjectStore.self_forest) and callable(smafa_amd.SubjectStore.self_forest_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_levels(") < text.index("smafa_db_self_forest_launch(")  # after the levels' section
    assert "level_ends[t]" in text and "may differ from run to run" in text


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, void *, void *) = smafa_db_self_forest_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, smafa_hit *, uint64_t, uint64_t *) = smafa_db_self_forest;\n"
                   "int (*const file_form)(const char *, uint32_t, int, int) = smafa_forest;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_invalid():
    l = _lib.lib()
    ends = (C.c_uint64 * 6)(*[9] * 6)
    edges = np.full(24, 7, dtype=smafa_amd.HIT_DTYPE)
    assert l.smafa_db_self_forest(None, 5, edges.ctypes.data, 24, ends) == _lib.ERR_INVALID
    assert b"smafa_db_self_forest: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_forest_launch(None, 5, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_forest_launch: NULL handle" in l.smafa_last_error()
    assert list(ends) == [9] * 6 and (edges["dist"] == 7).all()
    assert l.smafa_forest(None, 5, 1, 0) == _lib.ERR_INVALID
    assert b"NULL path" in l.smafa_last_error()
    assert l.smafa_forest(b"/nonexistent", _lib.NONE, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGT\n>b\nACGTACGA\n>c\nTTTTACGA\n")
    smafa_amd.makedb(fa, path)
    return path


def test_forest_without_a_gpu_says_so(db):
    if smafa_amd.device_count() > 0:
        r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "4"], capture_output=True)
        # a-b at 1, b-c at 3, a-c at 4: the heaviest pair closes a cycle
        assert r.returncode == 0 and r.stdout == b"0\t1\t1\n1\t2\t3\n", r.stderr
        return
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "2"], capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.forest(db, 2)
    assert e.value.code == _lib.ERR_DEVICE


def test_forest_usage_errors(db):
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db], capture_output=True)
    assert r.returncode == 2 and b"forest needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "forest", "--max-divergence", "2"], capture_output=True)
    assert r.returncode == 2 and b"forest needs --database" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "2", "--levels"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --levels" in r.stderr  # the flag belongs to `components` alone


def test_help_names_the_verb():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"forest  -d, --database <FILE>  --max-divergence <INT>" in r.stdout
    assert b"a<TAB>b<TAB>divergence" in r.stdout

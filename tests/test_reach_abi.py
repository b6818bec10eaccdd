"""The mutual-reachability forest's entry points without a GPU: exported symbols, the header as C99, argument checks, the
Python callables, the CLI's `forest --min-pts / --cores`."""
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
SYMBOLS = ("smafa_db_self_reach_forest_launch", "smafa_db_self_reach_forest", "smafa_reach_forest")
DECLARATIONS = (
    "int smafa_db_self_reach_forest_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, void *d_edges /* n_subjects - 1 smafa_hit */, "
    "void *d_level_ends /* max_div + 1 uint64 */, void *d_cores /* n_subjects uint32, may be NULL */);",
    "int smafa_db_self_reach_forest(smafa_db *db, uint32_t max_div, uint32_t min_pts, smafa_hit *edges, uint64_t cap, "
    "uint64_t *level_ends, uint32_t *cores /* n_subjects entries, may be NULL */);",
    "int smafa_reach_forest(const char *db_path, uint32_t max_divergence, uint32_t min_pts, int cores, int out_fd, int device);",
)


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.reach_forest) and callable(smafa_amd.forest_linkage)
    assert callable(smafa_amd.SubjectStore.self_reach_forest) and callable(smafa_amd.SubjectStore.self_reach_forest_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_forest(") < text.index("smafa_db_self_reach_forest_launch(")  # after the forest's section
    assert text.index("int smafa_forest(") < text.index("int smafa_reach_forest(")
    assert "max(distance(a, b), core[a], core[b])" in text and "may differ from run to run" in text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert "pub fn %s(" % name in integration, name


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, uint32_t, void *, void *, void *) = smafa_db_self_reach_forest_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, uint32_t, smafa_hit *, uint64_t, uint64_t *, uint32_t *) = "
                   "smafa_db_self_reach_forest;\n"
                   "int (*const file_form)(const char *, uint32_t, uint32_t, int, int, int) = smafa_reach_forest;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_invalid():
    l = _lib.lib()
    ends = (C.c_uint64 * 6)(*[9] * 6)
    edges = np.full(24, 7, dtype=smafa_amd.HIT_DTYPE)
    cores = np.full(25, 5, dtype=np.uint32)
    assert l.smafa_db_self_reach_forest(None, 5, 4, edges.ctypes.data, 24, ends, cores.ctypes.data) == _lib.ERR_INVALID
    assert b"smafa_db_self_reach_forest: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_reach_forest_launch(None, 5, 4, None, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_reach_forest_launch: NULL handle" in l.smafa_last_error()
    assert list(ends) == [9] * 6 and (edges["dist"] == 7).all() and (cores == 5).all()
    assert l.smafa_reach_forest(None, 5, 4, 0, 1, 0) == _lib.ERR_INVALID
    assert b"smafa_reach_forest: NULL path" in l.smafa_last_error()
    assert l.smafa_reach_forest(b"/nonexistent", _lib.NONE, 4, 0, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGT\n>b\nACGTACGA\n>c\nTTTTACGA\n")
    smafa_amd.makedb(fa, path)
    return path


def test_reach_forest_without_a_gpu_says_so(db):
    if smafa_amd.device_count() > 0:
        # a-b at 1, b-c at 3, a-c at 4; min_pts 2: cores 1, 1, 3
        r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "4", "--min-pts", "2"], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"0\t1\t1\n1\t2\t3\n", r.stderr
        r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "2", "--min-pts", "2", "--cores"], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"0\t1\n1\t1\n2\t-1\n", r.stderr
        return
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "2", "--min-pts", "2"], capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.reach_forest(db, 2, 2)
    assert e.value.code == _lib.ERR_DEVICE


def test_usage_errors(db):
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "2", "--cores"], capture_output=True)
    assert r.returncode == 2 and b"--cores needs --min-pts" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--min-pts", "3"], capture_output=True)
    assert r.returncode == 2 and b"forest needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "forest", "-d", db, "--max-divergence", "2", "--min-pts"], capture_output=True)
    assert r.returncode == 2 and b"--min-pts needs an unsigned integer" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "components", "-d", db, "--max-divergence", "2", "--cores"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --cores" in r.stderr  # the flag belongs to `forest` alone


def test_help_names_the_flags():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"[--min-pts <INT> [--cores]]" in r.stdout and b"i<TAB>core" in r.stdout


def test_forest_linkage_takes_these_edges():
    """five rows, the last one sparse: a tree of one, merged at max_divergence + 1"""
    edges = np.zeros(3, dtype=smafa_amd.HIT_DTYPE)
    edges["query"], edges["subject"], edges["dist"] = [2, 0, 0], [3, 1, 2], [0, 2, 2]
    Z = smafa_amd.forest_linkage(edges, 5, 3)
    assert Z.shape == (4, 4) and Z[:, 2].tolist() == [0.0, 2.0, 2.0, 4.0] and Z[:, 3].tolist() == [2.0, 2.0, 4.0, 5.0]
    assert sorted(Z[3, :2].tolist()) == [4.0, 7.0]

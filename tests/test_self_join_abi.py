"""The self-join's entry points without a GPU: argument checks, exported symbols, the CLI's `pairs` subcommand."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib


def test_symbols_are_exported():
    for name in ("smafa_db_self_launch", "smafa_db_self_hits", "smafa_pairs"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)


def test_null_handle_and_null_count_are_invalid():
    l = _lib.lib()
    n_out = C.c_uint64(0)
    assert l.smafa_db_self_hits(None, 5, None, 0, C.byref(n_out)) == _lib.ERR_INVALID
    assert b"NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_launch(None, 5, None, 0, None) == _lib.ERR_INVALID
    assert b"NULL handle" in l.smafa_last_error()
    assert l.smafa_pairs(None, 5, 1, 0) == _lib.ERR_INVALID
    assert l.smafa_last_error() != b""
    if smafa_amd.device_count() < 1:
        pytest.skip("the NULL-handle half is checked; a NULL count behind a live handle needs a device to make the handle")
    store = smafa_amd.SubjectStore(8, smafa_amd.ALPHABET_NT)
    assert l.smafa_db_self_hits(store._h, 5, None, 0, None) == _lib.ERR_INVALID
    assert b"NULL count" in l.smafa_last_error()
    assert l.smafa_db_self_launch(store._h, 5, None, 0, None) == _lib.ERR_INVALID
    assert b"NULL count" in l.smafa_last_error()
    store.close()


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGT\n>b\nACGTACGA\n>c\nTTTTACGA\n")
    smafa_amd.makedb(fa, path)
    return path


def test_pairs_without_a_gpu_says_so(db):
    if smafa_amd.device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_gpu_self_join.py::test_cli_pairs runs the command")
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", "2"], capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.pairs(db, 2)
    assert e.value.code == _lib.ERR_DEVICE


def test_pairs_usage_errors(db):
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db], capture_output=True)
    assert r.returncode == 2 and b"pairs needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "pairs", "--max-divergence", "2"], capture_output=True)
    assert r.returncode == 2 and b"pairs needs --database" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", "x"], capture_output=True)
    assert r.returncode == 2


def test_help_lists_pairs():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"pairs" in r.stdout and b"--max-divergence <INT>" in r.stdout
    for word in (b"Usage: smafa", b"makedb", b"query", b"cluster", b"count"):
        assert word in r.stdout


def test_header_declares_the_join_in_c():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "smafa_amd.h")).read()
    for decl in ("int smafa_db_self_launch(smafa_db *db, uint32_t max_div, void *d_hits, uint64_t cap, void *d_count);",
                 "int smafa_db_self_hits(smafa_db *db, uint32_t max_div, smafa_hit *out, uint64_t cap, uint64_t *n_out);",
                 "int smafa_pairs(const char *db_path, uint32_t max_divergence, int out_fd, int device);"):
        assert decl in text
    assert np.dtype(smafa_amd.HIT_DTYPE).itemsize == 12

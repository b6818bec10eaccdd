"""The stable-cluster entry points without a GPU: exported symbols, the header as C99, the argument checks that need no handle,
the Python callables, the CLI's `stable`.  The checks that need a handle — their documented order, that a refused call writes
nothing, the join's SMAFA_ERR_NOMEM — are tests/test_gpu_stable.py::test_a_refused_call_writes_nothing, ::test_argument_checks_in_order
and ::test_a_chunk_that_cannot_fit_fails_as_the_join_does."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_self_stable_launch", "smafa_db_self_stable", "smafa_stable")
DECLARATIONS = (
    "int smafa_db_self_stable_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t min_cluster_size, "
    "void *d_labels /* n_subjects uint32 */, void *d_joined /* n_subjects uint32, may be NULL */, "
    "void *d_cores /* n_subjects uint32, may be NULL */, uint64_t *n_clusters /* host */);",
    "int smafa_db_self_stable(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t min_cluster_size, uint32_t *labels, "
    "uint32_t *joined /* may be NULL */, uint32_t *cores /* may be NULL */, uint64_t cap, uint64_t *n_clusters);",
    "int smafa_stable(const char *db_path, uint32_t max_divergence, uint32_t min_pts, uint32_t min_cluster_size, int joined, int out_fd, "
    "int device);",
)


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.stable_clusters)
    assert callable(smafa_amd.SubjectStore.self_stable_clusters) and callable(smafa_amd.SubjectStore.self_stable_clusters_launch)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS:
        assert decl in text, decl
    assert text.index("smafa_db_self_reach_forest(") < text.index("smafa_db_self_stable_launch(")  # behind the reach forest's section
    assert text.index("int smafa_reach_forest(") < text.index("int smafa_stable(")
    # the definition, the words the issue asks for, and the order of the checks
    for words in ("kids(0, .) = 0", "a tie goes to the parent", "lambda measured in LEVELS", "depends on D through the roots' lifetime",
                  "a\n * NULL handle; NULL labels; NULL n_clusters; max_div == SMAFA_NONE; host form only: cap < n_subjects"):
        assert words in text, words
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert "pub fn %s(" % name in integration, name


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, uint32_t, uint32_t, uint32_t, void *, void *, void *, uint64_t *) = "
                   "smafa_db_self_stable_launch;\n"
                   "int (*const host_form)(smafa_db *, uint32_t, uint32_t, uint32_t, uint32_t *, uint32_t *, uint32_t *, uint64_t, uint64_t *) = "
                   "smafa_db_self_stable;\n"
                   "int (*const file_form)(const char *, uint32_t, uint32_t, uint32_t, int, int, int) = smafa_stable;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_a_null_handle_comes_first_and_nothing_is_written():
    l = _lib.lib()
    labels, joined, cores = (np.full(25, 5, dtype=np.uint32) for _ in range(3))
    count = C.c_uint64(9)
    args = (labels.ctypes.data, joined.ctypes.data, cores.ctypes.data)
    assert l.smafa_db_self_stable(None, 5, 4, 0, *args, 25, C.byref(count)) == _lib.ERR_INVALID
    assert b"smafa_db_self_stable: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_stable(None, _lib.NONE, 4, 0, None, None, None, 0, None) == _lib.ERR_INVALID  # whatever else is wrong
    assert b"smafa_db_self_stable: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_self_stable_launch(None, _lib.NONE, 4, 0, None, None, None, None) == _lib.ERR_INVALID
    assert b"smafa_db_self_stable_launch: NULL handle" in l.smafa_last_error()
    assert (labels == 5).all() and (joined == 5).all() and (cores == 5).all() and count.value == 9
    assert l.smafa_stable(None, 5, 4, 0, 0, 1, 0) == _lib.ERR_INVALID
    assert b"smafa_stable: NULL path" in l.smafa_last_error()
    assert l.smafa_stable(b"/nonexistent", _lib.NONE, 4, 0, 0, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()


def test_the_checks_are_coded_in_the_documented_order():
    """handle, labels, n_clusters, bound (self_args), then the capacity, then the first write — read off the source, since the checks
    behind the handle's need a handle"""
    text = open(os.path.join(ROOT, "smafa_amd", "csrc", "self_join_abi.hip.h")).read()
    body = text[text.index("int smafa_db_self_stable(smafa_db *db"):]
    body = body[: body.index("} catch")]
    first = body.index('self_args("smafa_db_self_stable", db, labels, "labels", n_clusters, "n_clusters", max_div, "stable clusters need a bound")')
    cap = body.index('labels_cap_arg("smafa_db_self_stable", db, cap)')
    write = body.index("*n_clusters = 0;")
    assert first < cap < write < body.index("join_stable(")
    args = text[text.index("static int self_args("):]
    order = [args.index(w) for w in ('missing(who, "handle")', "missing(who, a)", "missing(who, b)", "max_div == SMAFA_NONE")]
    assert order == sorted(order)
    launch = text[text.index("int smafa_db_self_stable_launch("):]
    launch = launch[: launch.index("} catch")]
    assert re.search(r'self_args\("smafa_db_self_stable_launch", db, d_labels, "labels", n_clusters, "n_clusters", max_div', launch)


@pytest.fixture()
def db(tmp_path):
    fa, path = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGT\n>b\nACGTACGA\n>c\nTTTTACGA\n")
    smafa_amd.makedb(fa, path)
    return path


def test_stable_without_a_gpu_says_so(db):
    if smafa_amd.device_count() > 0:
        r = subprocess.run([_lib.CLI_PATH, "stable", "-d", db, "--max-divergence", "2", "--min-pts", "2"], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"0\t0\n1\t0\n2\t-1\n", r.stderr
        return
    r = subprocess.run([_lib.CLI_PATH, "stable", "-d", db, "--max-divergence", "2", "--min-pts", "2"], capture_output=True)
    assert r.returncode != 0 and r.stdout == b""
    assert b"no HIP device visible" in r.stderr
    with pytest.raises(smafa_amd.SmafaError) as e:
        smafa_amd.stable_clusters(db, 2, 2)
    assert e.value.code == _lib.ERR_DEVICE


def test_usage_errors(db):
    base = [_lib.CLI_PATH, "stable", "-d", db]
    r = subprocess.run(base + ["--max-divergence", "2"], capture_output=True)
    assert r.returncode == 2 and b"stable needs --min-pts" in r.stderr and r.stdout == b""
    r = subprocess.run(base + ["--min-pts", "3"], capture_output=True)
    assert r.returncode == 2 and b"stable needs --max-divergence" in r.stderr and r.stdout == b""
    r = subprocess.run(base + ["--max-divergence", "2", "--min-pts", "2", "--min-cluster-size"], capture_output=True)
    assert r.returncode == 2 and b"--min-cluster-size needs an unsigned integer" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "stable", "--max-divergence", "2", "--min-pts", "2"], capture_output=True)
    assert r.returncode == 2 and b"stable needs --database" in r.stderr
    for flag in ("--joined", "--min-cluster-size"):  # the flags belong to `stable` alone
        r = subprocess.run([_lib.CLI_PATH, "density", "-d", db, "--max-divergence", "2", "--min-pts", "2", flag], capture_output=True)
        assert r.returncode == 2 and b"unexpected argument " + flag.encode() in r.stderr


def test_help_names_the_flags():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"stable  -d, --database <FILE>" in r.stdout and b"[--min-cluster-size <INT>] [--joined]" in r.stdout

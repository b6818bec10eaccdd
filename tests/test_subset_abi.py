"""The entry points of the subset and rows calls: exported symbols, the header as C99 against the library, and every check that
needs no device — the NULL arguments of the four calls and of the verb, with their texts in smafa_last_error."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(HERE, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_subset_launch", "smafa_db_subset", "smafa_db_rows_launch", "smafa_db_rows", "smafa_subset")


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    for method in ("subset", "subset_launch", "rows", "rows_launch"):
        assert callable(getattr(smafa_amd.SubjectStore, method))
    assert callable(smafa_amd.subset)


def test_header_and_integration_declare_them():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    for decl in ("int smafa_db_subset_launch(smafa_db *db, const void *d_keep /* n_subjects uint32 */, int invert, smafa_db **out, "
                 "void *d_old_of_new /* n_subjects uint32, may be NULL */, uint64_t *n_kept /* host */);",
                 "int smafa_db_subset(smafa_db *db, const uint32_t *keep, int invert, smafa_db **out, uint32_t *old_of_new /* may be NULL */, "
                 "uint64_t cap, uint64_t *n_kept);",
                 "int smafa_db_rows_launch(smafa_db *db, const void *d_subjects /* m uint32; NULL: first .. first+m-1 */, uint64_t first, "
                 "uint64_t m, void *d_codes /* m * seq_len bytes */);",
                 "int smafa_db_rows(smafa_db *db, const uint32_t *subjects, uint64_t first, uint64_t m, uint8_t *codes);",
                 "int smafa_subset(const char *db_path, const char *keep_path, const char *drop_path, const char *out_path, int out_fd, int device);"):
        assert decl in flat, decl
    assert text.index("smafa_db_classify(") < text.index("smafa_db_subset_launch(") < text.index("smafa_group_create(")
    for word in ("Checks, in this order", "The SOURCE is not modified", "a row of 0xff bytes", "*out stays NULL"):
        assert word in text, word
    mirror = open(os.path.join(HERE, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert "pub fn %s(" % name in mirror, name


def test_prototypes_compile_as_c99_and_link(tmp_path):
    """the pattern of tests/abi_c_check.c: a C99 program that takes the addresses under the header's own prototypes, links against
    the library and calls what needs no device"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "subset_c_check.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, const void *, int, smafa_db **, void *, uint64_t *) = smafa_db_subset_launch;\n"
                   "int (*const host_form)(smafa_db *, const uint32_t *, int, smafa_db **, uint32_t *, uint64_t, uint64_t *) = smafa_db_subset;\n"
                   "int (*const rows_launch_form)(smafa_db *, const void *, uint64_t, uint64_t, void *) = smafa_db_rows_launch;\n"
                   "int (*const rows_host_form)(smafa_db *, const uint32_t *, uint64_t, uint64_t, uint8_t *) = smafa_db_rows;\n"
                   "int (*const file_form)(const char *, const char *, const char *, const char *, int, int) = smafa_subset;\n"
                   "int main(void) {\n"
                   "    smafa_db *out = (smafa_db *)&out;\n"
                   "    uint64_t k = 7;\n"
                   "    if (host_form(NULL, NULL, 0, &out, NULL, 0, &k) != SMAFA_ERR_INVALID) return 1;\n"
                   '    if (!strstr(smafa_last_error(), "smafa_db_subset: NULL handle")) return 2;\n'
                   "    if (rows_host_form(NULL, NULL, 0, 0, NULL) != SMAFA_ERR_INVALID) return 3;\n"
                   '    if (file_form("x.db", NULL, NULL, "y.db", 1, 0) != SMAFA_ERR_INVALID) return 4;\n'
                   '    puts("ok");\n    return 0;\n}\n')
    exe = tmp_path / "subset_c_check"
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe), "-L", lib_dir,
                        "-lsmafa_amd", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stderr)


def test_null_arguments_need_no_device():
    l = _lib.lib()
    out, kept = C.c_void_p(5), C.c_uint64(9)
    keep = np.ones(4, dtype=np.uint32)
    for call, who in ((lambda: l.smafa_db_subset(None, keep.ctypes.data, 0, C.byref(out), None, 0, C.byref(kept)), b"smafa_db_subset"),
                      (lambda: l.smafa_db_subset_launch(None, None, 0, C.byref(out), None, C.byref(kept)), b"smafa_db_subset_launch"),
                      (lambda: l.smafa_db_rows(None, None, 0, 0, None), b"smafa_db_rows"),
                      (lambda: l.smafa_db_rows_launch(None, None, 0, 4, None), b"smafa_db_rows_launch")):
        assert call() == _lib.ERR_INVALID
        assert who + b": NULL handle" in l.smafa_last_error(), l.smafa_last_error()
    assert out.value == 5 and kept.value == 9  # the handle is checked first: nothing is written
    verb = lambda *a: l.smafa_subset(*a, 1, 0)  # noqa: E731
    for args, text in (((None, b"k", None, b"o.db"), b"smafa_subset: NULL path"),
                       ((b"x.db", b"k", None, None), b"smafa_subset: NULL output path"),
                       ((b"x.db", b"k", b"d", b"o.db"), b"smafa_subset: a keep list or a drop list, not both"),
                       ((b"x.db", None, None, b"o.db"), b"smafa_subset: a keep list or a drop list is needed")):
        assert verb(*args) == _lib.ERR_INVALID
        assert text in l.smafa_last_error(), l.smafa_last_error()


def test_help_and_usage_name_the_verb():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"subset  -d, --database <FILE>  (--keep <FILE|-> | --drop <FILE|->)  --output <FILE>" in r.stdout
    assert b"new<TAB>old" in r.stdout and b"smafa subset -d DB --drop - --output CLEAN.db" in r.stdout
    for args, text in ((("--keep", "k"), b"subset needs --database and --output"),
                       (("-d", "x.db", "--output", "o.db"), b"subset needs --keep or --drop"),
                       (("-d", "x.db", "--output", "o.db", "--keep", "a", "--drop", "b"), b"--keep and --drop exclude each other"),
                       (("-d", "x.db", "--output", "o.db", "--keep"), b"--keep needs a file, or - for stdin")):
        r = subprocess.run([_lib.CLI_PATH, "subset", *args], capture_output=True)
        assert r.returncode == 2 and text in r.stderr and r.stdout == b"", (args, r.stderr)
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", "x", "--max-divergence", "1", "--keep", "k"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --keep" in r.stderr  # the flag belongs to `subset` alone


def test_the_verb_fails_loudly_without_a_gpu(tmp_path):
    """no device, no store — an error code and its text, never an output file"""
    if smafa_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    from smafa_amd import synth

    codes = synth.subjects(50, 60, 0, seed=2)
    fa, db, out = str(tmp_path / "s.fa"), str(tmp_path / "s.db"), str(tmp_path / "o.db")
    synth.write_fasta(fa, codes, 0)
    open(str(tmp_path / "k"), "w").write("0\n")
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db], capture_output=True).returncode == 0
    r = subprocess.run([_lib.CLI_PATH, "subset", "-d", db, "--keep", str(tmp_path / "k"), "--output", out], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"no HIP device visible" in r.stderr and not os.path.exists(out), r.stderr

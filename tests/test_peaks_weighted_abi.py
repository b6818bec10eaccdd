"""The entry points of the peaks with given weights: exported symbols, the header as C99 against the library, and every check that
needs no device — the NULL arguments of the two calls and of the verb, with their texts in smafa_last_error."""
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
SYMBOLS = ("smafa_db_self_peaks_weighted_launch", "smafa_db_self_peaks_weighted", "smafa_peaks_weighted")


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.SubjectStore.self_peaks_weighted_launch) and callable(smafa_amd.peaks_weighted)


def test_header_and_integration_declare_them():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    for decl in ("int smafa_db_self_peaks_weighted_launch(smafa_db *db, uint32_t max_div, uint32_t radius, const void *d_weights_in "
                 "/* n_subjects uint32 */, void *d_labels, void *d_parents /* may be NULL */, void *d_weights /* may be NULL */, "
                 "void *d_n_peaks /* uint64 */);",
                 "int smafa_db_self_peaks_weighted(smafa_db *db, uint32_t max_div, uint32_t radius, const uint32_t *weights_in, uint32_t *labels, "
                 "uint32_t *parents, uint32_t *weights, uint64_t cap, uint64_t *n_peaks);",
                 "int smafa_peaks_weighted(const char *db_path, uint32_t max_divergence, uint32_t radius, const char *weights_path, int out_fd, "
                 "int device);"):
        assert decl in flat, decl
    assert text.index("smafa_db_rows(") < text.index("smafa_db_self_peaks_weighted_launch(") < text.index("smafa_peaks_weighted(") < text.index("smafa_group_create(")
    for word in ("the OTHER subjects", "A weight of 0 is allowed", "above 4294967295", "old_of_new[labels_S[unique_of[i]]]"):
        assert word in text, word
    mirror = open(os.path.join(HERE, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert "pub fn %s(" % name in mirror, name


def test_prototypes_compile_as_c99_and_link(tmp_path):
    """the pattern of tests/abi_c_check.c: a C99 program that takes the addresses under the header's own prototypes, links against
    the library and calls what needs no device"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "peaks_weighted_c_check.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "smafa_amd.h"\n'
                   "int (*const peaks_launch)(smafa_db *, uint32_t, uint32_t, const void *, void *, void *, void *, void *) = smafa_db_self_peaks_weighted_launch;\n"
                   "int (*const peaks_host)(smafa_db *, uint32_t, uint32_t, const uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint64_t, uint64_t *) = smafa_db_self_peaks_weighted;\n"
                   "int (*const peaks_file)(const char *, uint32_t, uint32_t, const char *, int, int) = smafa_peaks_weighted;\n"
                   "int main(void) {\n"
                   "    uint64_t u = 7;\n"
                   "    uint32_t labels[1] = {0};\n"
                   "    if (peaks_host(NULL, 2, 0, labels, labels, NULL, NULL, 1, &u) != SMAFA_ERR_INVALID || u != 7) return 1;\n"
                   '    if (!strstr(smafa_last_error(), "smafa_db_self_peaks_weighted: NULL handle")) return 2;\n'
                   "    if (peaks_launch(NULL, 2, 0, labels, labels, NULL, NULL, &u) != SMAFA_ERR_INVALID) return 3;\n"
                   '    if (peaks_file("x.db", 2, 0, NULL, 1, 0) != SMAFA_ERR_INVALID) return 4;\n'
                   '    puts("ok");\n    return 0;\n}\n')
    exe = tmp_path / "peaks_weighted_c_check"
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe), "-L", lib_dir,
                        "-lsmafa_amd", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stderr)


def test_null_arguments_need_no_device():
    l = _lib.lib()
    u = C.c_uint64(9)
    w = np.ones(4, dtype=np.uint32)
    for call, who in ((lambda: l.smafa_db_self_peaks_weighted(None, 2, 0, w.ctypes.data, w.ctypes.data, None, None, 4, C.byref(u)),
                       b"smafa_db_self_peaks_weighted"),
                      (lambda: l.smafa_db_self_peaks_weighted_launch(None, 2, 0, None, None, None, None, None), b"smafa_db_self_peaks_weighted_launch")):
        assert call() == _lib.ERR_INVALID
        assert who + b": NULL handle" in l.smafa_last_error(), l.smafa_last_error()
    assert u.value == 9  # the handle is checked first: nothing is written
    for args, text in (((None, 2, 0, b"w"), b"smafa_peaks_weighted: NULL path"), ((b"x.db", 2, 0, None), b"smafa_peaks_weighted: NULL weights path"),
                       ((b"x.db", _lib.NONE, 0, b"w"), b"smafa_peaks_weighted: a bound (max_divergence) is needed"),
                       ((b"x.db", 2, 3, b"w"), b"smafa_peaks_weighted: radius 3 is larger than max_divergence 2")):
        assert l.smafa_peaks_weighted(*args, 1, 0) == _lib.ERR_INVALID
        assert text in l.smafa_last_error(), l.smafa_last_error()


def test_help_and_usage_name_the_flag():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"--max-divergence <INT>  [--radius <INT>] [--sizes <FILE|->]" in r.stdout
    assert b"the sequence's own weight + those of the other sequences within the radius" in r.stdout
    r = subprocess.run([_lib.CLI_PATH, "peaks", "-d", "x", "--max-divergence", "1", "--sizes"], capture_output=True)
    assert r.returncode == 2 and b"--sizes needs a file, or - for stdin" in r.stderr and r.stdout == b""
    for verb in ("pairs", "chimeras", "density"):  # the flag belongs to `peaks` alone
        r = subprocess.run([_lib.CLI_PATH, verb, "-d", "x", "--max-divergence", "1", "--sizes", "f"], capture_output=True)
        assert r.returncode == 2 and b"unexpected argument --sizes" in r.stderr


def test_the_verb_fails_loudly_without_a_gpu(tmp_path):
    """no device, no store — an error code and its text, never a line of output"""
    if smafa_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    from smafa_amd import synth

    codes = synth.subjects(50, 60, 0, seed=2)
    fa, db = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    synth.write_fasta(fa, codes, 0)
    open(str(tmp_path / "w"), "w").write("0\t3\n")
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db], capture_output=True).returncode == 0
    r = subprocess.run([_lib.CLI_PATH, "peaks", "-d", db, "--max-divergence", "1", "--sizes", str(tmp_path / "w")], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"no HIP device visible" in r.stderr, r.stderr

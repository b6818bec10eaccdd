"""The delta join's entry points without a GPU: exported symbols, the header as C99, ctypes signatures against the header, the
argument checks that need no device, the CLI's `pairs --since`."""
import ctypes as C
import os
import re
import shutil
import subprocess

import smafa_amd
from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
DECLARATIONS = {
    "smafa_db_self_since_launch": "int smafa_db_self_since_launch(smafa_db *db, uint64_t first_row, uint32_t max_div, void *d_hits, "
                                  "uint64_t cap, void *d_count);",
    "smafa_db_self_hits_since": "int smafa_db_self_hits_since(smafa_db *db, uint64_t first_row, uint32_t max_div, smafa_hit *out, "
                                "uint64_t cap, uint64_t *n_out);",
    "smafa_db_self_components_update_launch": "int smafa_db_self_components_update_launch(smafa_db *db, uint64_t first_row, "
                                              "uint32_t max_div, void *d_labels, void *d_n_components);",
    "smafa_db_self_components_update": "int smafa_db_self_components_update(smafa_db *db, uint64_t first_row, uint32_t max_div, "
                                       "uint32_t *labels, uint64_t cap, uint64_t *n_components);",
    "smafa_pairs_since": "int smafa_pairs_since(const char *db_path, uint64_t first_row, uint32_t max_divergence, int out_fd, int device);",
}
CTYPES = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}


def test_symbols_are_exported():
    for name in DECLARATIONS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    for method in ("self_pairs_since", "self_since_launch", "self_components_update", "self_components_update_launch"):
        assert callable(getattr(smafa_amd.SubjectStore, method))
    assert callable(smafa_amd.pairs_since)


def test_header_declares_them_verbatim():
    text = open(HEADER).read()
    for decl in DECLARATIONS.values():
        assert decl in text, decl
    assert text.index("smafa_db_self_neighbours(") < text.index("smafa_db_self_since_launch(")  # after the neighbours section
    for phrase in ("j >= first_row", "byte for byte what smafa_db_self_components(db, max_div) returns", "labels[labels[i]] ==",
                   "first_row > n_subjects"):
        assert phrase in text, phrase


def test_ctypes_signatures_match_the_header():
    l = _lib.lib()
    for name, decl in DECLARATIONS.items():
        params = decl[decl.index("(") + 1:decl.rindex(")")].split(", ")
        kinds = []
        for p in params:
            base = re.sub(r"\bconst\b", "", p).rsplit(" ", 1)[0].strip()
            kinds.append("pointer" if "*" in p else base)
        args = getattr(l, name).argtypes
        assert len(args) == len(kinds), name
        for a, k in zip(args, kinds):
            if k == "pointer":
                assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, a)
            else:
                assert a is CTYPES[k], (name, a, k)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const a)(smafa_db *, uint64_t, uint32_t, void *, uint64_t, void *) = smafa_db_self_since_launch;\n"
                   "int (*const b)(smafa_db *, uint64_t, uint32_t, smafa_hit *, uint64_t, uint64_t *) = smafa_db_self_hits_since;\n"
                   "int (*const c)(smafa_db *, uint64_t, uint32_t, void *, void *) = smafa_db_self_components_update_launch;\n"
                   "int (*const d)(smafa_db *, uint64_t, uint32_t, uint32_t *, uint64_t, uint64_t *) = smafa_db_self_components_update;\n"
                   "int (*const e)(const char *, uint64_t, uint32_t, int, int) = smafa_pairs_since;\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_invalid_arguments_name_themselves_and_write_nothing():
    l = _lib.lib()
    n_out = (C.c_uint64 * 1)(9)
    buf = (C.c_uint32 * 6)(*([7] * 6))
    for form, cases in (
            ("smafa_db_self_hits_since", (((None, 0, 5, buf, 2, n_out), b"NULL handle"),)),
            ("smafa_db_self_since_launch", (((None, 0, 5, buf, 2, n_out), b"NULL handle"),)),
            ("smafa_db_self_components_update", (((None, 0, 5, buf, 6, n_out), b"NULL handle"),)),
            ("smafa_db_self_components_update_launch", (((None, 0, 5, buf, n_out), b"NULL handle"),))):
        for args, word in cases:
            assert getattr(l, form)(*args) == _lib.ERR_INVALID, (form, word)
            assert form.encode() + b": " in l.smafa_last_error() and word in l.smafa_last_error(), l.smafa_last_error()
            assert list(n_out) == [9] and list(buf) == [7] * 6
    assert l.smafa_pairs_since(None, 0, 5, 1, 0) == _lib.ERR_INVALID
    assert b"smafa_pairs_since: NULL path" in l.smafa_last_error()
    assert l.smafa_pairs_since(b"/nonexistent", 0, _lib.NONE, 1, 0) == _lib.ERR_INVALID
    assert b"bound" in l.smafa_last_error()
    assert l.smafa_pairs_since(b"/nonexistent", 0, 2, 1, 0) != _lib.ERR_INVALID  # the path fails, not an argument


def test_cli_since_usage(tmp_path):
    fa, db = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    with open(fa, "wb") as f:
        f.write(b">a\nACGTACGA\n>b\nACGTACGT\n>c\nTTTTACGA\n>d\nACGTACGT\n")
    smafa_amd.makedb(fa, db)
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", "1", "--since", "x"], capture_output=True)
    assert r.returncode == 2 and b"--since needs an unsigned integer" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", "1", "--since"], capture_output=True)
    assert r.returncode == 2 and b"--since needs an unsigned integer" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "components", "-d", db, "--max-divergence", "1", "--since", "1"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --since" in r.stderr  # a flag of `pairs` alone
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"[--since <ROW>]" in r.stdout
    assert b"pairs   -d, --database <FILE>  --max-divergence <INT>  [--device <N>]" in r.stdout  # the line as it was
    args = [_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", "1", "--since", "3"]
    r = subprocess.run(args, capture_output=True)
    if smafa_amd.device_count() > 0:
        # b = d, a at 1 of both, c far from all: of (0,1,1) (0,3,1) (1,3,0) the two with j >= 3
        assert r.returncode == 0 and r.stdout == b"0\t3\t1\n1\t3\t0\n", r.stderr
    else:
        assert r.returncode != 0 and r.stdout == b"" and b"no HIP device visible" in r.stderr

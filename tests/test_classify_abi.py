"""The classification's entry points: exported symbols, the header as C99 and the checks that need no device without a GPU; with
one, every argument check in the documented order with its text, sentinels around every output ("nothing written"), the point
from which totals[] is zeroed, the host-side checks in front of any device work, and the capacity protocol."""
import ctypes as C  # noqa: F401
import os
import shutil
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib
from assign_cases import NONE, TABLE_DTYPE, random_samples, random_weights
from classify_cases import FIELDS, ROOT, expected_classify, tie_case, tie_lineage

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(HERE, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_classify_launch", "smafa_db_classify", "smafa_classify")
CASE = ("aa60", 150, 5, 4)
gpu = pytest.mark.gpu


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.classify) and callable(smafa_amd.SubjectStore.classify) and callable(smafa_amd.SubjectStore.classify_launch)
    assert smafa_amd.Classified._fields == FIELDS and smafa_amd.TAXON_ROOT == ROOT == 0xFFFFFFFE


def test_header_and_integration_declare_them():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    for decl in ("#define SMAFA_TAXON_ROOT 0xfffffffeu",
                 "int smafa_db_classify_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, uint32_t slack, const void *d_lineage",
                 "int smafa_db_classify(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div, uint32_t slack, "
                 "const uint32_t *lineage, uint32_t n_ranks, const uint32_t *samples, uint32_t n_samples, const uint32_t *weights, "
                 "uint32_t *subject, uint32_t *dist, uint32_t *taxon, uint32_t *depth, uint32_t *ties, smafa_table_entry *entries, "
                 "uint64_t cap, uint64_t totals[6]);",
                 "int smafa_classify(const char *db_path, const char *query_fasta, uint32_t max_divergence, uint32_t slack, "
                 "const char *taxonomy_path, const char *samples_path, const char *weights_path, int per_read, int out_fd, int device);"):
        assert decl in flat, decl
    assert text.index("smafa_db_assign(") < text.index("smafa_db_classify_launch(") < text.index("smafa_group_create(")
    for word in ("Checks, in this order", "totals[] is zeroed", "Ids are compared WITHOUT their ancestors", "up to its first SMAFA_NONE"):
        assert word in text, word
    mirror = open(os.path.join(HERE, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert "pub fn %s(" % name in mirror, name
    assert "SMAFA_TAXON_ROOT" in mirror


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, smafa_qset *, uint32_t, uint32_t, const void *, uint32_t, const void *, uint32_t, "
                   "const void *, void *, void *, void *, void *, void *, void *, uint64_t, void *) = smafa_db_classify_launch;\n"
                   "int (*const host_form)(smafa_db *, const uint8_t *, uint64_t, uint32_t, uint32_t, const uint32_t *, uint32_t, const uint32_t *, "
                   "uint32_t, const uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t *, smafa_table_entry *, uint64_t, "
                   "uint64_t *) = smafa_db_classify;\n"
                   "int (*const file_form)(const char *, const char *, uint32_t, uint32_t, const char *, const char *, const char *, int, int, "
                   "int) = smafa_classify;\n"
                   "typedef char root_is_below_none[SMAFA_TAXON_ROOT + 1u == SMAFA_NONE ? 1 : -1];\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_and_paths_are_invalid():
    l = _lib.lib()
    totals = np.full(6, 9, dtype=np.uint64)
    assert l.smafa_db_classify(None, None, 0, 3, 0, None, 7, None, 1, None, None, None, None, None, None, None, 0, totals.ctypes.data) == _lib.ERR_INVALID
    assert b"smafa_db_classify: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_classify_launch(None, None, 3, 0, None, 7, None, 1, None, None, None, None, None, None, None, 0, None) == _lib.ERR_INVALID
    assert b"smafa_db_classify_launch: NULL handle" in l.smafa_last_error() and (totals == 9).all()
    verb = lambda *a: l.smafa_classify(*a, 0, 1, 0)  # noqa: E731
    assert verb(None, b"r.fa", 3, 0, b"t", None, None) == _lib.ERR_INVALID and b"smafa_classify: NULL path" in l.smafa_last_error()
    assert verb(b"x.db", b"r.fa", _lib.NONE, 0, b"t", None, None) == _lib.ERR_INVALID and b"a bound" in l.smafa_last_error()
    assert verb(b"x.db", None, 3, 0, b"t", None, None) == _lib.ERR_INVALID and b"NULL reads path" in l.smafa_last_error()
    assert verb(b"x.db", b"r.fa", 3, 0, None, None, None) == _lib.ERR_INVALID and b"NULL taxonomy path" in l.smafa_last_error()
    assert verb(b"x.db", b"r.fa", 3, 0, b"-", None, b"-") == _lib.ERR_INVALID and b"at most one of" in l.smafa_last_error()


def test_help_and_usage_name_the_verb():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"classify -d, --database <FILE>  -q, --query <FILE>  --max-divergence <INT>  --taxonomy <FILE|->" in r.stdout
    assert b"lineage<TAB>sample<TAB>count" in r.stdout and b"read<TAB>subject<TAB>divergence<TAB>ties<TAB>depth<TAB>lineage" in r.stdout
    r = subprocess.run([_lib.CLI_PATH, "classify", "-q", "r.fa", "--max-divergence", "3", "--taxonomy", "t"], capture_output=True)
    assert r.returncode == 2 and b"classify needs --database and --query" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "classify", "-d", "x.db", "-q", "r.fa", "--taxonomy", "t"], capture_output=True)
    assert r.returncode == 2 and b"classify needs --max-divergence" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "classify", "-d", "x.db", "-q", "r.fa", "--max-divergence", "3"], capture_output=True)
    assert r.returncode == 2 and b"classify needs --taxonomy" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "table", "-d", "x", "-q", "r.fa", "--taxonomy", "-"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --taxonomy" in r.stderr  # the flag belongs to `classify` alone


def test_the_verb_fails_loudly_without_a_gpu(tmp_path):
    """no device, no answer — an error code and its text, never an empty table"""
    if smafa_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    from smafa_amd import synth

    codes = synth.subjects(50, 60, 0, seed=2)
    fa, db, tx = str(tmp_path / "s.fa"), str(tmp_path / "s.db"), str(tmp_path / "t.tsv")
    synth.write_fasta(fa, codes, 0)
    open(tx, "w").write("0\tRoot; d__A\n")
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db], capture_output=True).returncode == 0
    r = subprocess.run([_lib.CLI_PATH, "classify", "-d", db, "-q", fa, "--max-divergence", "3", "--taxonomy", tx], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"no HIP device visible" in r.stderr, r.stderr


class Outputs:
    """every output of the host form between sentinels: a guard entry on each side of every array"""

    def __init__(self, K, m):
        self.K = K
        self.entries = np.full(2 * (K + 2), 5, dtype=np.uint64)
        self.reads = [np.full(m + 2, 5, dtype=np.uint32) for _ in range(5)]  # subject, dist, taxon, depth, ties
        self.totals = np.full(8, 5, dtype=np.uint64)

    def args(self, cap=None, entries=True, totals=True, per_read=True):
        inner = lambda a, step=1: a.ctypes.data + step * a.itemsize  # noqa: E731
        return (*[inner(a) if per_read else None for a in self.reads], inner(self.entries, 2) if entries else None,
                self.K if cap is None else cap, inner(self.totals) if totals else None)

    def untouched(self, but_totals=False):
        return all((a == 5).all() for a in (self.entries, *self.reads)) and (but_totals or (self.totals == 5).all())

    def guards_hold(self):
        return all(a[0] == 5 and a[-1] == 5 for a in (*self.reads, self.totals)) and (self.entries[:2] == 5).all() and (self.entries[-2:] == 5).all()

    def arrays(self):
        return (self.entries[2:-2].view(TABLE_DTYPE), *[a[1:-1] for a in self.reads], self.totals[1:-1])


@pytest.fixture()
def case():
    codes, reads, dmat = tie_case(*CASE)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    samples, weights = random_samples(len(reads), 3, 4), random_weights(len(reads), 5)
    yield store, codes, reads, dmat, np.ascontiguousarray(tie_lineage(*CASE, 7)), samples, weights
    store.close()


@gpu
def test_argument_checks_in_order(case):
    """handle, the reads, totals, the bound, n_samples, entries with a capacity, n_ranks, the lineage — then the launch form's
    foreign query set and the host form's code bytes, sample numbers and lineage rows: with several arguments wrong the first of
    these is the one named, and nothing is written, totals[] included"""
    store, codes, reads, _, lineage, samples, weights = case
    l = _lib.lib()
    m = len(reads)
    o = Outputs(m, m)
    *per_read, entries, cap, totals = o.args()
    q, s, w, t = reads.ctypes.data, samples.ctypes.data, weights.ctypes.data, lineage.ctypes.data
    host = lambda *a: l.smafa_db_classify(store._h, *a)  # noqa: E731
    for args, text in (((None, m, NONE, 1, None, 0, s, 0, w, *per_read, None, cap, None), b"NULL query_codes"),
                       ((q, m, NONE, 1, None, 0, s, 0, w, *per_read, None, cap, None), b"NULL totals"),
                       ((q, m, NONE, 1, None, 0, s, 0, w, *per_read, None, cap, totals), b"a table needs a bound (max_div)"),
                       ((q, m, 5, 1, None, 0, s, 0, w, *per_read, None, cap, totals), b"n_samples is 0"),
                       ((q, m, 5, 1, None, 0, s, 2, w, *per_read, None, cap, totals), b"NULL entries with a capacity"),
                       ((q, m, 5, 1, None, 0, s, 2, w, *per_read, entries, cap, totals), b"n_ranks is 0 (1 .. 16)"),
                       ((q, m, 5, 1, None, 17, s, 2, w, *per_read, entries, cap, totals), b"n_ranks is 17 (1 .. 16)"),
                       ((q, m, 5, 1, None, 7, s, 2, w, *per_read, entries, cap, totals), b"NULL lineage")):
        assert host(*args) == _lib.ERR_INVALID
        assert b"smafa_db_classify: " + text in l.smafa_last_error(), l.smafa_last_error()
        assert o.untouched()
    # the host-side checks, in front of any device work: code bytes, then samples, then the lineage — the first place is named
    broken = lineage.copy()
    broken[3, 2] = ROOT
    first = int(np.flatnonzero(samples >= 2)[0])
    bad = reads.copy()
    bad[3, 3] = 28
    assert host(bad.ctypes.data, m, 5, 1, broken.ctypes.data, 7, s, 2, w, *per_read, entries, cap, totals) == _lib.ERR_INVALID
    assert b"outside the alphabet" in l.smafa_last_error() and o.untouched()
    assert host(q, m, 5, 1, broken.ctypes.data, 7, s, 2, w, *per_read, entries, cap, totals) == _lib.ERR_INVALID
    assert b"smafa_db_classify: samples[%d] is 2, n_samples is 2" % first in l.smafa_last_error() and o.untouched()
    assert host(q, m, 5, 1, broken.ctypes.data, 7, s, 3, w, *per_read, entries, cap, totals) == _lib.ERR_INVALID
    assert b"smafa_db_classify: lineage[3][2] is SMAFA_TAXON_ROOT" in l.smafa_last_error() and o.untouched()
    broken[3] = [1, NONE, NONE, NONE, 4, NONE, NONE]
    assert host(q, m, 5, 1, broken.ctypes.data, 7, s, 3, w, *per_read, entries, cap, totals) == _lib.ERR_INVALID
    assert b"smafa_db_classify: lineage[3][4] holds an id behind a SMAFA_NONE" in l.smafa_last_error() and o.untouched()
    # the launch form: the same order, then the query set of another store
    other = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    qset = smafa_amd.QuerySet(other, reads[:4])
    launch = lambda *a: l.smafa_db_classify_launch(store._h, *a)  # noqa: E731
    nothing = (None,) * 5
    for args, text in (((None, NONE, 0, None, 0, None, 0, None, *nothing, None, 4, None), b"NULL query set"),
                       ((qset._h, NONE, 0, None, 0, None, 0, None, *nothing, None, 4, None), b"NULL totals"),
                       ((qset._h, NONE, 0, None, 0, None, 0, None, *nothing, None, 4, totals), b"a table needs a bound (max_div)"),
                       ((qset._h, 5, 0, None, 0, None, 0, None, *nothing, None, 4, totals), b"n_samples is 0"),
                       ((qset._h, 5, 0, None, 0, None, 1, None, *nothing, None, 4, totals), b"NULL entries with a capacity"),
                       ((qset._h, 5, 0, None, 0, None, 1, None, *nothing, None, 0, totals), b"n_ranks is 0 (1 .. 16)"),
                       ((qset._h, 5, 0, None, 7, None, 1, None, *nothing, None, 0, totals), b"NULL lineage"),
                       ((qset._h, 5, 0, t, 7, None, 1, None, *nothing, None, 0, totals), b"the query set was packed for a different store")):
        assert launch(*args) == _lib.ERR_INVALID
        assert b"smafa_db_classify_launch: " + text in l.smafa_last_error(), l.smafa_last_error()
        assert o.untouched()
    qset.close()
    other.close()


@gpu
def test_the_host_side_checks_run_no_kernel(case):
    store, codes, reads, _, lineage, samples, weights = case
    l = _lib.lib()
    m = len(reads)
    o = Outputs(m, m)
    store.classify(reads[:5], 5, lineage)  # (a call that clears the list and fills it)
    assert store.last_call_kernels()
    store.self_components(0)               # ... and one whose list names no classify:: kernel
    before = store.last_call_kernels()
    assert before and not any(k.startswith("classify::") for k in before)
    broken = lineage.copy()
    broken[len(codes) - 1, 6] = ROOT
    for tax, sam, n_samples in ((lineage, samples, 1), (broken, samples, 3)):
        assert l.smafa_db_classify(store._h, reads.ctypes.data, m, 5, 0, tax.ctypes.data, 7, sam.ctypes.data, n_samples, None, *o.args()) == _lib.ERR_INVALID
        assert store.last_call_kernels() == before and o.untouched()  # nothing was launched, nothing was reset


@gpu
def test_capacity_reports_the_count_and_the_retry_succeeds(case):
    store, codes, reads, dmat, lineage, samples, weights = case
    l = _lib.lib()
    m = len(reads)
    want = expected_classify(codes, reads, 5, lineage, 1, samples, 3, weights, dmat=dmat)
    K = len(want[0])
    o = Outputs(K, m)
    q, s, w, t = reads.ctypes.data, samples.ctypes.data, weights.ctypes.data, lineage.ctypes.data
    *per_read, entries, cap, totals = o.args()
    head = (store._h, q, m, 5, 1, t, 7, s, 3, w)
    assert l.smafa_db_classify(*head, *per_read, None, 0, totals) == _lib.ERR_CAPACITY  # asking for the count
    assert b"%d entries needed, capacity 0" % K in l.smafa_last_error()
    assert o.arrays()[6].tobytes() == want[6].tobytes() and o.untouched(but_totals=True) and o.guards_hold()
    assert l.smafa_db_classify(*head, *per_read, entries, K - 1, totals) == _lib.ERR_CAPACITY
    assert int(o.arrays()[6][0]) == K and o.untouched(but_totals=True)
    assert l.smafa_db_classify(*head, *per_read, entries, K, totals) == _lib.OK
    assert o.guards_hold()
    for name, g, x in zip(FIELDS, o.arrays(), want):
        assert g.tobytes() == x.tobytes(), name
    # the optional outputs left out, and a capacity above the count: entries behind it stay as they were
    o = Outputs(K + 3, m)
    *per_read, entries, cap, totals = o.args(per_read=False)
    assert l.smafa_db_classify(*head, *per_read, entries, cap, totals) == _lib.OK
    got = o.arrays()
    assert got[0][:K].tobytes() == want[0].tobytes() and (o.entries[2 + 2 * K:] == 5).all() and got[6].tobytes() == want[6].tobytes()
    assert all((a == 5).all() for a in o.reads)


@gpu
def test_totals_are_zeroed_behind_the_checks():
    """a call that passes its checks and fails behind them: SMAFA_ERR_NOMEM from a row limit no span of 64 reads fits (a
    store of one row 3 000 times) leaves totals[] zero and every other output as it was"""
    from test_gpu_assign import copies_case

    codes, reads = copies_case()
    os.environ["SMAFA_ASSIGN_ROWS_MAX"] = "100000"  # (read when the handle is made)
    try:
        store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    finally:
        del os.environ["SMAFA_ASSIGN_ROWS_MAX"]
    store.push(codes)
    m = len(reads)
    lineage = np.ones((3000, 7), dtype=np.uint32)
    o = Outputs(m, m)
    assert _lib.lib().smafa_db_classify(store._h, reads.ctypes.data, m, 3, 1, lineage.ctypes.data, 7, None, 1, None, *o.args()) == _lib.ERR_NOMEM
    assert (o.arrays()[6] == 0).all() and o.untouched(but_totals=True) and o.guards_hold()
    store.close()

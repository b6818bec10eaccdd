"""The abundance table's entry points: exported symbols, the header as C99 and the checks that need no device without a GPU; with
one, every argument check in the documented order with its text, sentinels around every output ("nothing written"), the point
from which totals[] is zeroed, the host-side sample check in front of any device work, and the capacity protocol."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib
from assign_cases import NONE, TABLE_DTYPE, expected_assign, random_samples, random_weights, shape_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smafa_amd.h")
SYMBOLS = ("smafa_db_assign_launch", "smafa_db_assign", "smafa_table")
gpu = pytest.mark.gpu


def test_symbols_are_exported():
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert callable(smafa_amd.table) and callable(smafa_amd.SubjectStore.assign) and callable(smafa_amd.SubjectStore.assign_launch)
    assert smafa_amd.TableEntry.itemsize == 16 and smafa_amd.TableEntry.names == ("label", "sample", "count")
    assert smafa_amd.Assigned._fields == ("entries", "subject", "dist", "subject_counts", "totals")


def test_header_declares_them():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    for decl in ("typedef struct { uint32_t label; uint32_t sample; uint64_t count; } smafa_table_entry;",
                 "int smafa_db_assign_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, const void *d_labels",
                 "int smafa_db_assign(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div, const uint32_t *labels, "
                 "const uint32_t *samples, uint32_t n_samples, const uint32_t *weights, uint32_t *subject, uint32_t *dist, "
                 "uint64_t *subject_counts, smafa_table_entry *entries, uint64_t cap, uint64_t totals[4]);",
                 "int smafa_table(const char *db_path, const char *query_fasta, uint32_t max_divergence, const char *labels_path, "
                 "const char *samples_path, const char *weights_path, int per_read, int per_sequence, int out_fd, int device);"):
        assert decl in flat, decl
    assert text.index("smafa_db_consensus(") < text.index("smafa_db_assign_launch(") < text.index("smafa_group_create(")
    for word in ("Checks, in this order", "totals[] is zeroed", "SMAFA_ASSIGN_SPAN", "SMAFA_ASSIGN_ROWS_MAX", "a tie to the smaller subject number"):
        assert word in text, word


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "take_addresses.c"
    src.write_text('#include "smafa_amd.h"\n'
                   "int (*const launch_form)(smafa_db *, smafa_qset *, uint32_t, const void *, const void *, uint32_t, const void *, void *, void *, "
                   "void *, void *, uint64_t, void *) = smafa_db_assign_launch;\n"
                   "int (*const host_form)(smafa_db *, const uint8_t *, uint64_t, uint32_t, const uint32_t *, const uint32_t *, uint32_t, "
                   "const uint32_t *, uint32_t *, uint32_t *, uint64_t *, smafa_table_entry *, uint64_t, uint64_t *) = smafa_db_assign;\n"
                   "int (*const file_form)(const char *, const char *, uint32_t, const char *, const char *, const char *, int, int, int, int) = "
                   "smafa_table;\n"
                   "typedef char entry_is_16_bytes[sizeof(smafa_table_entry) == 16 ? 1 : -1];\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(src), "-o",
                        str(tmp_path / "take_addresses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_and_paths_are_invalid():
    l = _lib.lib()
    totals = np.full(4, 9, dtype=np.uint64)
    assert l.smafa_db_assign(None, None, 0, 3, None, None, 1, None, None, None, None, None, 0, totals.ctypes.data) == _lib.ERR_INVALID
    assert b"smafa_db_assign: NULL handle" in l.smafa_last_error()
    assert l.smafa_db_assign_launch(None, None, 3, None, None, 1, None, None, None, None, None, 0, None) == _lib.ERR_INVALID
    assert b"smafa_db_assign_launch: NULL handle" in l.smafa_last_error() and (totals == 9).all()
    assert l.smafa_table(None, b"r.fa", 3, None, None, None, 0, 0, 1, 0) == _lib.ERR_INVALID and b"smafa_table: NULL path" in l.smafa_last_error()
    assert l.smafa_table(b"x.db", b"r.fa", _lib.NONE, None, None, None, 0, 0, 1, 0) == _lib.ERR_INVALID and b"a bound" in l.smafa_last_error()
    assert l.smafa_table(b"x.db", None, 3, None, None, None, 0, 0, 1, 0) == _lib.ERR_INVALID and b"NULL reads path" in l.smafa_last_error()
    assert l.smafa_table(b"x.db", b"r.fa", 3, None, None, None, 1, 1, 1, 0) == _lib.ERR_INVALID and b"exclude each other" in l.smafa_last_error()
    assert l.smafa_table(b"x.db", b"r.fa", 3, b"-", None, b"-", 0, 0, 1, 0) == _lib.ERR_INVALID and b"at most one of" in l.smafa_last_error()


def test_help_and_usage_name_the_verb():
    r = subprocess.run([_lib.CLI_PATH, "--help"], capture_output=True)
    assert r.returncode == 0 and b"table   -d, --database <FILE>  -q, --query <FILE>  --max-divergence <INT>" in r.stdout
    assert b"label<TAB>sample<TAB>count" in r.stdout and b"--per-sequence | smafa chimeras" in r.stdout
    r = subprocess.run([_lib.CLI_PATH, "table", "-q", "r.fa", "--max-divergence", "3"], capture_output=True)
    assert r.returncode == 2 and b"table needs --database and --query" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, "table", "-d", "x.db", "-q", "r.fa"], capture_output=True)
    assert r.returncode == 2 and b"table needs --max-divergence" in r.stderr
    r = subprocess.run([_lib.CLI_PATH, "consensus", "-d", "x", "--labels", "-", "--samples", "-"], capture_output=True)
    assert r.returncode == 2 and b"unexpected argument --samples" in r.stderr  # the flag belongs to `table` alone


def test_the_verb_fails_loudly_without_a_gpu(tmp_path):
    """as test_scan_fails_loudly_without_gpu: no device, no answer — an error code and its text, never an empty table"""
    if smafa_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    from smafa_amd import synth

    codes = synth.subjects(50, 60, 0, seed=2)
    fa, db = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    synth.write_fasta(fa, codes, 0)
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db], capture_output=True).returncode == 0
    r = subprocess.run([_lib.CLI_PATH, "table", "-d", db, "-q", fa, "--max-divergence", "3"], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"no HIP device visible" in r.stderr, r.stderr


class Outputs:
    """every output of the host form between sentinels: a guard entry on each side of every array"""

    def __init__(self, K, n, m):
        self.K = K
        self.entries = np.full(2 * (K + 2), 5, dtype=np.uint64)
        self.subject, self.dist = np.full(m + 2, 5, dtype=np.uint32), np.full(m + 2, 5, dtype=np.uint32)
        self.counts = np.full(n + 2, 5, dtype=np.uint64)
        self.totals = np.full(6, 5, dtype=np.uint64)

    def args(self, cap=None, entries=True, totals=True):
        inner = lambda a, step=1: a.ctypes.data + step * a.itemsize  # noqa: E731
        return (inner(self.subject), inner(self.dist), inner(self.counts), inner(self.entries, 2) if entries else None,
                self.K if cap is None else cap, inner(self.totals) if totals else None)

    def untouched(self, but_totals=False):
        return all((a == 5).all() for a in (self.entries, self.subject, self.dist, self.counts)) and (but_totals or (self.totals == 5).all())

    def guards_hold(self):
        return all(a[0] == 5 and a[-1] == 5 for a in (self.subject, self.dist, self.counts, self.totals)) and \
            (self.entries[:2] == 5).all() and (self.entries[-2:] == 5).all()

    def arrays(self):
        return (self.entries[2:-2].view(TABLE_DTYPE), self.subject[1:-1], self.dist[1:-1], self.counts[1:-1], self.totals[1:-1])


@pytest.fixture()
def case():
    codes, reads, _, _ = shape_reads("aa60", 150, 5, 4)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    samples, weights = random_samples(len(reads), 3, 4), random_weights(len(reads), 5)
    yield store, codes, reads, samples, weights
    store.close()


@gpu
def test_argument_checks_in_order(case):
    """handle, the reads, totals, the bound, n_samples, entries with a capacity — then the launch form's foreign query set and
    the host form's code bytes and sample numbers: with several arguments wrong the first of these is the one named, and nothing
    is written, totals[] included"""
    store, codes, reads, samples, weights = case
    l = _lib.lib()
    n, m = len(codes), len(reads)
    o = Outputs(m, n, m)
    subject, dist, counts, entries, cap, totals = o.args()
    q, s, w = reads.ctypes.data, samples.ctypes.data, weights.ctypes.data
    host = lambda *a: l.smafa_db_assign(store._h, *a)  # noqa: E731
    for args, text in (((None, m, NONE, None, s, 0, w, subject, dist, counts, None, cap, None), b"NULL query_codes"),
                       ((q, m, NONE, None, s, 0, w, subject, dist, counts, None, cap, None), b"NULL totals"),
                       ((q, m, NONE, None, s, 0, w, subject, dist, counts, None, cap, totals), b"a table needs a bound (max_div)"),
                       ((q, m, 5, None, s, 0, w, subject, dist, counts, None, cap, totals), b"n_samples is 0"),
                       ((q, m, 5, None, s, 2, w, subject, dist, counts, None, cap, totals), b"NULL entries with a capacity")):
        assert host(*args) == _lib.ERR_INVALID
        assert b"smafa_db_assign: " + text in l.smafa_last_error(), l.smafa_last_error()
        assert o.untouched()
    # the sample check: on the host, before any device work — the first offending read is named and no kernel has run
    first = int(np.flatnonzero(samples >= 2)[0])
    store.scan(reads[:1], max_divergence=1)
    assert store.last_call_kernels()
    assert host(q, m, 5, None, s, 2, w, subject, dist, counts, entries, cap, totals) == _lib.ERR_INVALID
    assert b"smafa_db_assign: samples[%d] is 2, n_samples is 2" % first in l.smafa_last_error(), l.smafa_last_error()
    assert o.untouched()
    bad = reads.copy()
    bad[3, 3] = 28
    assert host(bad.ctypes.data, m, 5, None, s, 2, w, subject, dist, counts, entries, cap, totals) == _lib.ERR_INVALID
    assert b"outside the alphabet" in l.smafa_last_error() and o.untouched()  # (the code bytes come before the samples)
    # the launch form: the same order, then the query set of another store
    other = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    qset = smafa_amd.QuerySet(other, reads[:4])
    launch = lambda *a: l.smafa_db_assign_launch(store._h, *a)  # noqa: E731
    for args, text in (((None, NONE, None, None, 0, None, None, None, None, None, 4, None), b"NULL query set"),
                       ((qset._h, NONE, None, None, 0, None, None, None, None, None, 4, None), b"NULL totals"),
                       ((qset._h, NONE, None, None, 0, None, None, None, None, None, 4, totals), b"a table needs a bound (max_div)"),
                       ((qset._h, 5, None, None, 0, None, None, None, None, None, 4, totals), b"n_samples is 0"),
                       ((qset._h, 5, None, None, 1, None, None, None, None, None, 4, totals), b"NULL entries with a capacity"),
                       ((qset._h, 5, None, None, 1, None, None, None, None, None, 0, totals), b"the query set was packed for a different store")):
        assert launch(*args) == _lib.ERR_INVALID
        assert b"smafa_db_assign_launch: " + text in l.smafa_last_error(), l.smafa_last_error()
        assert o.untouched()
    qset.close()
    other.close()


@gpu
def test_the_sample_check_runs_no_kernel(case):
    store, codes, reads, samples, weights = case
    l = _lib.lib()
    m = len(reads)
    o = Outputs(m, len(codes), m)
    store.assign(reads[:5], 5)  # (a call that clears the list and fills it)
    assert store.last_call_kernels()
    components = store.self_components(0)  # ... and one whose list names no assign:: kernel
    before = store.last_call_kernels()
    assert before and not any(k.startswith("assign::") for k in before)
    assert l.smafa_db_assign(store._h, reads.ctypes.data, m, 5, None, samples.ctypes.data, 1, None, *o.args()) == _lib.ERR_INVALID
    assert store.last_call_kernels() == before and o.untouched()  # nothing was launched, nothing was reset
    assert components[1] > 0


@gpu
def test_capacity_reports_the_count_and_the_retry_succeeds(case):
    store, codes, reads, samples, weights = case
    l = _lib.lib()
    n, m = len(codes), len(reads)
    want = expected_assign(codes, reads, 5, None, samples, 3, weights)
    K = len(want[0])
    o = Outputs(K, n, m)
    q, s, w = reads.ctypes.data, samples.ctypes.data, weights.ctypes.data
    subject, dist, counts, entries, cap, totals = o.args()
    assert l.smafa_db_assign(store._h, q, m, 5, None, s, 3, w, subject, dist, counts, None, 0, totals) == _lib.ERR_CAPACITY  # asking for the count
    assert b"%d entries needed, capacity 0" % K in l.smafa_last_error()
    assert o.arrays()[4].tobytes() == want[4].tobytes() and o.untouched(but_totals=True) and o.guards_hold()
    assert l.smafa_db_assign(store._h, q, m, 5, None, s, 3, w, subject, dist, counts, entries, K - 1, totals) == _lib.ERR_CAPACITY
    assert int(o.arrays()[4][0]) == K and o.untouched(but_totals=True)
    assert l.smafa_db_assign(store._h, q, m, 5, None, s, 3, w, subject, dist, counts, entries, K, totals) == _lib.OK
    assert o.guards_hold()
    for name, g, x in zip(smafa_amd.Assigned._fields, o.arrays(), want):
        assert g.tobytes() == x.tobytes(), name
    # the optional outputs left out, and a capacity above the count: entries behind it stay as they were
    o = Outputs(K + 3, n, m)
    _, _, _, entries, cap, totals = o.args()
    assert l.smafa_db_assign(store._h, q, m, 5, None, s, 3, w, None, None, None, entries, cap, totals) == _lib.OK
    got = o.arrays()
    assert got[0][:K].tobytes() == want[0].tobytes() and (o.entries[2 + 2 * K:] == 5).all() and got[4].tobytes() == want[4].tobytes()
    assert (o.subject == 5).all() and (o.dist == 5).all() and (o.counts == 5).all()


@gpu
def test_totals_are_zeroed_behind_the_checks(case):
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
    o = Outputs(m, len(codes), m)
    assert _lib.lib().smafa_db_assign(store._h, reads.ctypes.data, m, 3, None, None, 1, None, *o.args()) == _lib.ERR_NOMEM
    assert (o.arrays()[4] == 0).all() and o.untouched(but_totals=True) and o.guards_hold()
    store.close()

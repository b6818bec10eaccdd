"""The abundance table of a resident store (smafa_db_assign / smafa_db_assign_launch / `smafa table`): every read assigned to its
nearest subject within a bound, and counted per (label, sample).

Expected values never come from the code under test (tests/assign_cases.py): the model is the header's definition in plain numpy
on the code bytes, and every output — entries, subject, dist, subject_counts, totals — is held to it byte for byte."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from assign_cases import (ASSIGN_KERNELS, NONE, expected_assign, planted_reads, random_samples, random_weights, read_lines,
                          sequence_lines, shape_reads, table_lines)
from components_cases import labels_from_pairs_numpy
from consensus_cases import random_grouping
from self_join_cases import SHAPE_STORES, SHAPE_TABLE, replaned_case, shape_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AA60 = ("aa60", 150, 5, 4)


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    if len(codes):
        store.push(codes)
    return store


def check(store, codes, reads, D, labels=None, samples=None, n_samples=None, weights=None, kernels=ASSIGN_KERNELS):
    """one host-form call with every output asked for, against the model; -> the bytes of all five outputs"""
    want = expected_assign(codes, reads, D, labels, samples, n_samples, weights)
    got = store.assign(reads, D, labels=labels, samples=samples, n_samples=n_samples, weights=weights, subject_counts=True)
    for name, g, w in zip(got._fields, got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    if kernels is not None:
        assert store.last_call_kernels()[-len(kernels):] == kernels  # the scan family first, then the call's own
    return [g.tobytes() for g in got]


@pytest.mark.parametrize("name,families,D,max_subs", SHAPE_STORES)
def test_every_shape_equals_the_model(name, families, D, max_subs):
    """every store shape (two, three and five planes, one to twenty-two words) under three labellings — the components at the
    shape's bound, identity, a random grouping with SMAFA_NONE labels —, one and three samples, no weights and weights 0 .. 5.  The
    kernels are assign::init_kernel, assign::best_kernel, assign::bin_kernel, assign::heads_kernel and assign::fold_kernel."""
    codes, reads, _, _ = shape_reads(name, families, D, max_subs)
    n, m = len(codes), len(reads)
    store = make_store(codes, SHAPE_TABLE[name][0])
    components = labels_from_pairs_numpy(n, shape_case(name, families, D, max_subs)[1])
    for labels, n_samples, weighted in itertools.product((components, None, random_grouping(n, 100 + n)), (1, 3), (False, True)):
        check(store, codes, reads, D, labels, random_samples(m, n_samples, 1) if n_samples > 1 else None, n_samples,
              random_weights(m, 2) if weighted else None)
    stats = store.last_call_stats()
    assert stats["scans"] == 1 and stats["kernel_ms"] > 0 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    store.close()


@pytest.mark.parametrize("m", [1, 64, 65, 2000])
def test_read_counts(m):
    """one read, the few-query scan form's last size, the first size behind it, and a big batch"""
    codes, _ = shape_case(*AA60)
    reads = planted_reads(codes, 5, m, 50 + m, strangers=0 if m == 1 else None)
    store = make_store(codes, "aa")
    check(store, codes, reads, 5, random_grouping(len(codes), 3), random_samples(m, 3, 4), 3, random_weights(m, 5))
    store.close()


def test_spans_of_64_give_the_same_bytes(monkeypatch):
    """SMAFA_ASSIGN_SPAN=64 on 200 reads: four spans, the last short"""
    codes, _ = shape_case(*AA60)
    reads = planted_reads(codes, 5, 200, 77)
    args = (codes, reads, 5, random_grouping(len(codes), 3), random_samples(200, 3, 4), 3, random_weights(200, 5))
    store = make_store(codes, "aa")
    default = check(store, *args)
    assert store.last_call_stats()["scans"] == 1
    store.close()
    monkeypatch.setenv("SMAFA_ASSIGN_SPAN", "64")  # (read when the handle is made)
    store = make_store(codes, "aa")
    monkeypatch.delenv("SMAFA_ASSIGN_SPAN")
    assert check(store, *args) == default and store.last_call_stats()["scans"] == 4
    store.close()


def copies_case():
    """one row copied 3 000 times, and 256 reads of which 200 are that row: 3 000 rows at the minimum distance each"""
    rng = np.random.default_rng(9)
    row = rng.integers(0, 4, size=60).astype(np.uint8)
    codes = np.repeat(row[None], 3000, axis=0)
    reads = np.concatenate([np.repeat(row[None], 200, axis=0), rng.integers(0, 4, size=(56, 60)).astype(np.uint8)])
    return codes, reads[rng.permutation(256)]


def test_a_small_row_limit_grows_then_halves_then_fails(monkeypatch):
    """engine.h's rule (assign_first_room, assign_span_rule) with SMAFA_ASSIGN_SPAN=256: the first room is 64 x 256 = 16 384 rows.
    SMAFA_ASSIGN_ROWS_MAX=250000: the 256 reads' 600 000 rows do not fit, the room doubles up to 250 000, then the span is cut to
    128 and to 64 reads (at most 192 000 rows: they fit) — the same bytes as under the default limit.  SMAFA_ASSIGN_ROWS_MAX=100000:
    a span of 64 reads may still hold more than 33 copies of the row, 64 reads alone overflow the limit and the call fails with
    SMAFA_ERR_NOMEM — an error code, and the handle answers the next call (a store without the copies) under the same limit."""
    codes, reads = copies_case()
    samples, weights = random_samples(256, 3, 4), random_weights(256, 5)
    store = make_store(codes, "nt")
    default = check(store, codes, reads, 3, None, samples, 3, weights)
    assert store.last_call_stats()["scans"] == 1
    store.close()
    monkeypatch.setenv("SMAFA_ASSIGN_SPAN", "256")
    monkeypatch.setenv("SMAFA_ASSIGN_ROWS_MAX", "250000")
    store = make_store(codes, "nt")
    assert check(store, codes, reads, 3, None, samples, 3, weights) == default
    assert store.last_call_stats()["scans"] > 4  # the rooms 16 384 .. 250 000, the two cuts, then the spans of 64
    store.close()
    monkeypatch.setenv("SMAFA_ASSIGN_ROWS_MAX", "100000")
    store = make_store(codes, "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.assign(reads, 3)
    assert e.value.code == _lib.ERR_NOMEM and "64 reads have more rows" in str(e.value)
    few = codes[:1000]
    small = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    small.push(few)
    check(small, few, reads[:20], 3)  # 20 reads x 1 000 copies fit the limit
    small.close()
    check(store, codes, reads[:30], 3)  # ... and the handle that failed: 30 reads x 3 000 copies fit too
    store.close()


def test_one_long_run_and_runs_of_one():
    """1 500 of 2 000 reads in one (label, sample): a run that crosses 24 waves of assign::fold_kernel; then labels and samples
    such that every read is an entry of its own — 2 000 runs of one"""
    codes, _ = shape_case(*AA60)
    rng = np.random.default_rng(31)
    n = len(codes)
    one = codes[rng.integers(0, n, size=1500)]
    reads = np.concatenate([one, planted_reads(codes, 5, 500, 32)])[rng.permutation(2000)]
    store = make_store(codes, "aa")
    everything = np.full(n, 7, dtype=np.uint32)
    check(store, codes, reads, 5, everything, None, 1, random_weights(2000, 6))
    entries = store.assign(reads, 5, labels=everything).entries
    assert int(entries["count"].max()) >= 1500
    own = np.arange(2000, dtype=np.uint32)  # a sample per read: every (label, sample) holds one read
    check(store, codes, reads, 5, None, own, 2000)
    assert len(store.assign(reads, 5, samples=own, n_samples=2000).entries) == 2000
    store.close()


def test_store_states():
    """the re-planed store pushed in its three pieces (the first N arrives late), then a store appended to between two calls:
    subject numbers stay in append order"""
    pieces, _ = replaned_case()
    store = make_store(pieces[0], "nt")
    held = pieces[0]
    reads = planted_reads(np.concatenate(pieces), 5, 300, 12)
    for piece, planes in ((None, 2), (pieces[1], 2), (pieces[2], 3)):
        if piece is not None:
            store.push(piece)
            held = np.concatenate([held, piece])
        assert store.info().planes == planes
        check(store, held, reads, 5, random_grouping(len(held), len(held)), random_samples(300, 3, 1), 3)
    store.close()


def test_every_scan_setting_gives_the_same_bytes():
    codes, reads, _, _ = shape_reads(*AA60)
    args = (codes, reads, 5, random_grouping(len(codes), 3), random_samples(len(reads), 3, 4), 3, random_weights(len(reads), 5))
    store = make_store(codes, "aa")
    default = check(store, *args)
    store.build_index(5)
    for prefilter, zone, index in itertools.product((True, False), (0, 1, 2), (0, 1)):
        store.set_prefilter(prefilter)
        store.set_zone_level(zone)
        store.set_index(index)
        assert check(store, *args) == default, (prefilter, zone, index)
    store.close()


def test_twice_and_behind_another_call():
    """the handle's scratch (the row list, the sort's buffers, J.parent) is shared with the self-store calls"""
    codes, reads, _, _ = shape_reads(*AA60)
    args = (codes, reads, 5, None, random_samples(len(reads), 3, 4), 3, random_weights(len(reads), 5))
    store = make_store(codes, "aa")
    first = check(store, *args)
    assert check(store, *args) == first
    components = store.self_components(5)[0]
    assert check(store, *args) == first
    assert store.self_components(5)[0].tobytes() == components.tobytes()
    store.close()


def test_empty_store_and_no_reads():
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    reads = np.random.default_rng(1).integers(0, 4, size=(70, 60)).astype(np.uint8)
    empty = np.zeros((0, 60), dtype=np.uint8)
    check(store, empty, reads, 5, None, random_samples(70, 3, 1), 3, kernels=ASSIGN_KERNELS[:1] + ASSIGN_KERNELS[2:])
    store.push(reads[:10])
    check(store, reads[:10], empty, 5, kernels=ASSIGN_KERNELS[:1])
    store.close()


def test_device_form():
    """cap = 0 with NULL entries counts only; half the capacity stores the first half in table order with the exact count; a
    sample number out of range shows in totals[3] and nowhere else (tests/assign_worker.py: torch initialises HIP first)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "assign_worker.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "table device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_cli_table(tmp_path):
    """`smafa table` on a DB file and its packed form, a reads FASTA and the three side files, in its three output forms, against
    lines built from the model; `table --per-sequence | chimeras --weights -` equals self_chimeras(weights=subject_counts)"""
    codes, reads, _, _ = shape_reads(*AA60)
    n, m, D = len(codes), len(reads), 5
    labels, samples, weights = random_grouping(n, 3), random_samples(m, 3, 4), random_weights(m, 5)
    labels[-4:] = NONE  # (the file may end early: the last four lines are left out)
    entries, subject, dist, counts, _ = expected_assign(codes, reads, D, labels, samples, 3, weights)
    fa, qa, db, packed, lab, sam, wei = (str(tmp_path / f) for f in ("s.fa", "q.fa", "s.db", "s.packed", "l.tsv", "s.tsv", "w.tsv"))
    synth.write_fasta(fa, codes, 1)
    synth.write_fasta(qa, reads, 1)
    for out, more in ((db, []), (packed, ["--packed"])):
        assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", out, "--alphabet", "aa", *more], capture_output=True).returncode == 0
    with open(lab, "wb") as f:
        f.write(b"".join(b"%d\t%d\n" % (i, -1 if v == NONE else v) for i, v in enumerate(labels[:-4].tolist())))
    with open(sam, "wb") as f:  # (reads of sample 0 have no line; in any order)
        f.write(b"".join(b"%d\t%d\n" % (q, samples[q]) for q in reversed(range(m)) if samples[q]))
    with open(wei, "wb") as f:  # (reads of weight 1 have no line)
        f.write(b"".join(b"%d\t%d\textra\n" % (q, weights[q]) for q in range(m) if weights[q] != 1))
    base = ["table", "-q", qa, "--max-divergence", str(D), "--labels", lab, "--samples", sam, "--weights", wei]
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, *base, "-d", path], capture_output=True)
        assert r.returncode == 0 and r.stdout == table_lines(entries), r.stderr
        assert b"table entries of %d reads in 3 samples" % m in r.stderr
    r = subprocess.run([_lib.CLI_PATH, *base, "-d", db, "--per-read"], capture_output=True)
    assert r.returncode == 0 and r.stdout == read_lines(subject, dist), r.stderr
    per_sequence = subprocess.run([_lib.CLI_PATH, *base, "-d", db, "--per-sequence", "--labels", "-"], input=open(lab, "rb").read(), capture_output=True)
    assert per_sequence.returncode == 0 and per_sequence.stdout == sequence_lines(counts), per_sequence.stderr
    out = str(tmp_path / "table.tsv")
    with open(out, "wb") as f:
        smafa_amd.table(db, qa, D, lab, sam, wei, out_fd=f.fileno())
    assert open(out, "rb").read() == table_lines(entries)
    # no side file at all: identity labels, one sample, every read weighs 1
    plain = expected_assign(codes, reads, D)
    r = subprocess.run([_lib.CLI_PATH, "table", "-d", db, "-q", qa, "--max-divergence", str(D)], capture_output=True)
    assert r.returncode == 0 and r.stdout == table_lines(plain[0]), r.stderr
    # ... and on into the chimera check
    r = subprocess.run([_lib.CLI_PATH, "chimeras", "-d", db, "--max-divergence", str(D), "--weights", "-"], input=per_sequence.stdout, capture_output=True)
    store = make_store(codes, "aa")
    c = store.self_chimeras(D, weights=counts.astype(np.uint32))
    store.close()
    show = lambda v: -1 if v == NONE else v  # noqa: E731
    want = b"".join(b"%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (i, c.flags[i], show(c.left_parent[i]), c.left_len[i], show(c.right_parent[i]), c.right_len[i],
                                                      c.weights[i]) for i in range(n))
    assert r.returncode == 0 and r.stdout == want, r.stderr
    # what the verb refuses: two files from stdin, both per-row forms, a read of another length, a line for a read that is not there
    r = subprocess.run([_lib.CLI_PATH, *base[:-4], "-d", db, "--samples", "-", "--weights", "-"], input=b"", capture_output=True)
    assert r.returncode == 1 and b"at most one of" in r.stderr and r.stdout == b""
    r = subprocess.run([_lib.CLI_PATH, *base, "-d", db, "--per-read", "--per-sequence"], capture_output=True)
    assert r.returncode == 2 and b"exclude each other" in r.stderr
    short = str(tmp_path / "short.fa")
    synth.write_fasta(short, reads[:3, :50], 1)
    r = subprocess.run([_lib.CLI_PATH, "table", "-d", db, "-q", short, "--max-divergence", "5"], capture_output=True)
    assert r.returncode == 101 and b"Cannot compute distances between seq of length 50 and windows of lengths 60" in r.stderr
    with open(sam, "wb") as f:
        f.write(b"0\t1\n%d\t2\n" % m)
    r = subprocess.run([_lib.CLI_PATH, *base, "-d", db], capture_output=True)
    assert r.returncode == 1 and b"smafa_table: samples line 2:" in r.stderr and r.stdout == b""

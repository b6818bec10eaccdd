"""The classification of a resident query set (smafa_db_classify / smafa_db_classify_launch / `smafa classify`): every read given
the lowest common ancestor of the lineages of its best hits, and counted per (taxon, sample).

Expected values never come from the code under test (tests/classify_cases.py): the model is the header's definition in plain numpy
on the code bytes, and every output — entries, subject, dist, taxon, depth, ties, totals — is held to it byte for byte."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from assign_cases import NONE, planted_reads, random_samples, random_weights
from classify_cases import (CLASSIFY_KERNELS, FIELDS, ROOT, coverage, entry_lines, expected_classify, intern_taxonomy, per_read_lines,
                            tie_case, tie_lineage, tree_lineage)
from self_join_cases import SHAPE_STORES, SHAPE_TABLE, replaned_case, shape_case
from test_gpu_assign import copies_case

pytestmark = pytest.mark.gpu
AA60 = ("aa60", 150, 5, 4)


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    if len(codes):
        store.push(codes)
    return store


def check(store, codes, reads, D, lineage, slack=0, samples=None, n_samples=None, weights=None, kernels=CLASSIFY_KERNELS, dmat=None):
    """one host-form call against the model; -> the bytes of all seven outputs"""
    want = expected_classify(codes, reads, D, lineage, slack, samples, n_samples, weights, dmat=dmat)
    got = store.classify(reads, D, lineage, slack=slack, samples=samples, n_samples=n_samples, weights=weights)
    assert got._fields == FIELDS
    for name, g, w in zip(got._fields, got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, slack)
    if kernels is not None:
        assert store.last_call_kernels()[-len(kernels):] == kernels  # the scan family first, then the call's own
    return [g.tobytes() for g in got]


@pytest.mark.parametrize("name,families,D,max_subs", SHAPE_STORES)
def test_every_shape_equals_the_model(name, families, D, max_subs):
    """every store shape (two, three and five planes, one to twenty-two words) with tie families appended, R in {1, 7, 16} (rows of
    7 ranks are not 16-byte aligned), slack in {0, 1, the bound}, one and three samples, weights off and on.  The model's own view of
    the inputs is asserted first: ties are the rule, every depth 0 .. R occurs, the anchor's lineage is the shortest somewhere,
    another member's somewhere else, and some read is unassigned.  The kernels are classify::start_kernel, assign::best_kernel,
    classify::agree_kernel, classify::key_kernel, assign::heads_kernel and assign::fold_kernel."""
    store_codes, reads, dmat = tie_case(name, families, D, max_subs)
    m = len(reads)
    store = make_store(store_codes, SHAPE_TABLE[name][0])
    sides = itertools.cycle(itertools.product((1, 3), (False, True)))
    for R, slack in itertools.product((1, 7, 16), (0, 1, D)):
        lineage = tie_lineage(name, families, D, max_subs, R)
        share, depths, anchor_shortest, other_shortest, unassigned = coverage(store_codes, dmat, D, lineage, slack)
        assert share >= 0.25 and depths == set(range(R + 1)) and anchor_shortest and other_shortest and unassigned
        n_samples, weighted = next(sides)
        check(store, store_codes, reads, D, lineage, slack, random_samples(m, n_samples, 1) if n_samples > 1 else None, n_samples,
              random_weights(m, 2) if weighted else None, dmat=dmat)
    stats = store.last_call_stats()
    assert stats["scans"] == 1 and stats["kernel_ms"] > 0 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    store.close()


@pytest.mark.parametrize("odd", [0, 63, 64, 2999])
def test_a_run_that_crosses_waves(odd):
    """3 000 copies of one row, every lineage equal except row `odd`'s, which leaves the others at rank 2 of 7: the 200 reads of the
    copied row come out at depth 2 with ties 3 000 — the minimum rests on one lane's value in the first, a middle or the last wave of
    the run"""
    codes, reads = copies_case()
    lineage = np.tile(np.arange(1, 8, dtype=np.uint32), (3000, 1))
    lineage[odd, 2:] = np.arange(100, 105)
    store = make_store(codes, "nt")
    got = store.classify(reads, 3, lineage)
    same = (reads == codes[0]).all(axis=1)
    assert same.sum() == 200
    assert (got.depth[same] == 2).all() and (got.ties[same] == 3000).all() and (got.taxon[same] == 2).all() and (got.subject[same] == 0).all()
    check(store, codes, reads, 3, lineage, 0, random_samples(256, 3, 4), 3, random_weights(256, 5))
    store.close()


@pytest.mark.parametrize("m", [1, 64, 65, 2000])
def test_read_counts(m):
    """one read, the few-query scan form's last size, the first size behind it, and a big batch"""
    codes, _ = shape_case(*AA60)
    reads = planted_reads(codes, 5, m, 50 + m, strangers=0 if m == 1 else None)
    store = make_store(codes, "aa")
    for slack in (0, 2):
        check(store, codes, reads, 5, tree_lineage(len(codes), 7, 3), slack, random_samples(m, 3, 4), 3, random_weights(m, 5))
    store.close()


def test_spans_of_64_give_the_same_bytes(monkeypatch):
    """SMAFA_ASSIGN_SPAN=64 on 200 reads: four spans, the last short"""
    codes, _ = shape_case(*AA60)
    reads = planted_reads(codes, 5, 200, 77)
    lineage = tree_lineage(len(codes), 7, 3)
    sides = (random_samples(200, 3, 4), 3, random_weights(200, 5))
    store = make_store(codes, "aa")
    default = [check(store, codes, reads, 5, lineage, slack, *sides) for slack in (0, 1)]
    assert store.last_call_stats()["scans"] == 1
    store.close()
    monkeypatch.setenv("SMAFA_ASSIGN_SPAN", "64")  # (read when the handle is made)
    store = make_store(codes, "aa")
    monkeypatch.delenv("SMAFA_ASSIGN_SPAN")
    assert [check(store, codes, reads, 5, lineage, slack, *sides) for slack in (0, 1)] == default and store.last_call_stats()["scans"] == 4
    store.close()


@pytest.mark.parametrize("slack", [0, 1])
def test_a_small_row_limit_grows_then_halves_then_fails(monkeypatch, slack):
    """the ladder of the table's test of this name: SMAFA_ASSIGN_SPAN=256 and SMAFA_ASSIGN_ROWS_MAX=250000 make the 256 reads' 600 000
    rows grow the room, then halve the span twice — a span scanned again has run no kernel of the call, so ties are 3 000 and not
    a multiple of it, and the bytes are the default's.  SMAFA_ASSIGN_ROWS_MAX=100000: 64 reads alone overflow it and the call fails
    with SMAFA_ERR_NOMEM — an error code, and the handle answers the next call."""
    codes, reads = copies_case()
    samples, weights = random_samples(256, 3, 4), random_weights(256, 5)
    lineage = np.tile(np.arange(1, 8, dtype=np.uint32), (3000, 1))
    lineage[1500, 4:] = NONE
    store = make_store(codes, "nt")
    default = check(store, codes, reads, 3, lineage, slack, samples, 3, weights)
    assert store.last_call_stats()["scans"] == 1
    store.close()
    monkeypatch.setenv("SMAFA_ASSIGN_SPAN", "256")
    monkeypatch.setenv("SMAFA_ASSIGN_ROWS_MAX", "250000")
    store = make_store(codes, "nt")
    assert check(store, codes, reads, 3, lineage, slack, samples, 3, weights) == default
    assert store.last_call_stats()["scans"] > 4  # the rooms 16 384 .. 250 000, the two cuts, then the spans of 64
    assert int(store.classify(reads, 3, lineage, slack=slack).ties.max()) == 3000
    store.close()
    monkeypatch.setenv("SMAFA_ASSIGN_ROWS_MAX", "100000")
    store = make_store(codes, "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.classify(reads, 3, lineage, slack=slack)
    assert e.value.code == _lib.ERR_NOMEM and "64 reads have more rows" in str(e.value)
    check(store, codes, reads[:30], 3, lineage, slack)  # the handle that failed: 30 reads x 3 000 copies fit
    store.close()


def test_store_states():
    """the re-planed store pushed in its three pieces (the first N arrives late): subject numbers stay in append order"""
    pieces, _ = replaned_case()
    store = make_store(pieces[0], "nt")
    held = pieces[0]
    reads = planted_reads(np.concatenate(pieces), 5, 300, 12)
    for piece, planes in ((None, 2), (pieces[1], 2), (pieces[2], 3)):
        if piece is not None:
            store.push(piece)
            held = np.concatenate([held, piece])
        assert store.info().planes == planes
        for slack in (0, 5):
            check(store, held, reads, 5, tree_lineage(len(held), 7, len(held)), slack, random_samples(300, 3, 1), 3)
    store.close()


def test_every_scan_setting_gives_the_same_bytes():
    store_codes, reads, dmat = tie_case(*AA60)
    lineage = tie_lineage(*AA60, 7)
    sides = (random_samples(len(reads), 3, 4), 3, random_weights(len(reads), 5))
    store = make_store(store_codes, "aa")
    default = {slack: check(store, store_codes, reads, 5, lineage, slack, *sides, dmat=dmat) for slack in (0, 2)}
    store.build_index(5)
    for prefilter, zone, index, slack in itertools.product((True, False), (0, 1, 2), (0, 1), (0, 2)):
        store.set_prefilter(prefilter)
        store.set_zone_level(zone)
        store.set_index(index)
        got = store.classify(reads, 5, lineage, slack=slack, samples=sides[0], n_samples=3, weights=sides[2])
        assert [g.tobytes() for g in got] == default[slack], (prefilter, zone, index, slack)
    store.close()


def test_twice_and_behind_another_call():
    """the handle's scratch (the row list, the sort's buffers, J.parent) is shared with the self-store calls and the table"""
    store_codes, reads, dmat = tie_case(*AA60)
    lineage = tie_lineage(*AA60, 7)
    args = (store_codes, reads, 5, lineage, 1, random_samples(len(reads), 3, 4), 3, random_weights(len(reads), 5))
    store = make_store(store_codes, "aa")
    first = check(store, *args, dmat=dmat)
    assert check(store, *args, dmat=dmat) == first
    components = store.self_components(5)[0]
    assert check(store, *args, dmat=dmat) == first
    assert store.self_components(5)[0].tobytes() == components.tobytes()
    store.close()


def test_empty_store_and_no_reads():
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    reads = np.random.default_rng(1).integers(0, 4, size=(70, 60)).astype(np.uint8)
    empty = np.zeros((0, 60), dtype=np.uint8)
    check(store, empty, reads, 5, np.zeros((0, 7), np.uint32), 0, random_samples(70, 3, 1), 3, kernels=CLASSIFY_KERNELS[:1] + CLASSIFY_KERNELS[3:])
    store.push(reads[:10])
    check(store, reads[:10], empty, 5, tree_lineage(10, 7, 1), 1, kernels=CLASSIFY_KERNELS[:1])
    store.close()


def test_subject_and_dist_are_the_tables_and_one_rank_gives_its_entries():
    """classify(...).subject and .dist equal assign(...)'s; with R = 1 and lineage[i] = [labels[i]] the entries equal
    assign(labels=...)'s wherever every read's best hits share one label — here: the labels are the exact-copy classes, and at slack
    0 the hits of a read at distance 0 are copies of each other; the reads are rows of the store"""
    codes, _ = shape_case(*AA60)
    _, labels = np.unique(codes, axis=0, return_inverse=True)
    labels = labels.reshape(-1).astype(np.uint32)
    reads = np.ascontiguousarray(codes[np.random.default_rng(3).integers(0, len(codes), size=300)])
    samples, weights = random_samples(300, 3, 4), random_weights(300, 5)
    store = make_store(codes, "aa")
    table = store.assign(reads, 0, labels=labels, samples=samples, n_samples=3, weights=weights)
    got = store.classify(reads, 0, labels[:, None], samples=samples, n_samples=3, weights=weights)
    assert got.subject.tobytes() == table.subject.tobytes() and got.dist.tobytes() == table.dist.tobytes()
    assert got.entries.tobytes() == table.entries.tobytes() and (got.depth == 1).all() and (got.ties > 1).any()
    assert got.totals[:4].tobytes() == table.totals.tobytes()
    planted = planted_reads(codes, 5, 300, 8)
    for slack in (0, 3):
        got = store.classify(planted, 5, tree_lineage(len(codes), 7, 3), slack=slack)
        table = store.assign(planted, 5)
        assert got.subject.tobytes() == table.subject.tobytes() and got.dist.tobytes() == table.dist.tobytes()
    store.close()


def test_what_the_host_form_refuses_of_a_lineage():
    codes, _ = shape_case(*AA60)
    reads = codes[:5]
    store = make_store(codes, "aa")
    lineage = tree_lineage(len(codes), 7, 3)
    for bad, row, col, text in ((ROOT, 9, 3, "lineage[9][3] is SMAFA_TAXON_ROOT"), (5, 11, 6, "lineage[11][6] holds an id behind a SMAFA_NONE")):
        broken = lineage.copy()
        broken[row] = [1, 2, 3, 4, 5, NONE, NONE]
        broken[row, col] = bad
        with pytest.raises(smafa_amd.SmafaError) as e:
            store.classify(reads, 5, broken)
        assert e.value.code == _lib.ERR_INVALID and text in str(e.value)
    for R in (0, 17):
        with pytest.raises(smafa_amd.SmafaError) as e:
            store.classify(reads, 5, np.ones((len(codes), R), np.uint32))
        assert e.value.code == _lib.ERR_INVALID and "n_ranks is %d (1 .. 16)" % R in str(e.value)
    check(store, codes, reads, 5, lineage)  # the handle answers the next call
    store.close()


def test_device_form():
    """cap = 0 with NULL entries counts only; half the capacity stores the first half in table order with the exact count; a
    sample number out of range shows in totals[3] and nowhere else (tests/classify_worker.py: torch initialises HIP first)"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "classify_worker.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "classify device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def taxonomy_file(n, seed):
    """-> (file bytes, [(i, names)] in file order): lines in a shuffled order, SingleM-style blanks, a further column on some lines,
    a trailing ';' on others, every tenth sequence without a line, some rows that end early; one genus name under two families"""
    rng = np.random.default_rng(seed)
    lines, text = [], []
    for i in rng.permutation(n):
        if i % 10 == 9:
            continue
        leaf = int(rng.integers(0, 12))
        path = ["Root", "d__D%d" % (leaf // 6), "p__P%d" % (leaf // 3), "f__F%d" % leaf, "g__shared" if leaf in (4, 7) else "g__G%d" % leaf]
        path = path[:int(rng.integers(1, 6))]
        lines.append((int(i), path))
        text.append("%d\t%s%s%s\n" % (i, "; ".join(path), ";" if i % 3 == 0 else "", "\tnote" if i % 4 == 0 else ""))
    return "".join(text).encode(), lines


def test_cli_classify(tmp_path):
    """`smafa classify` on a DB file and its packed form against lines built from the model: a taxonomy file with lines in any
    order, missing sequences and SingleM-style blanks, the two side files, --slack, --per-read; then every refusal, each with its
    exit status and an empty stdout"""
    store_codes, reads, dmat = tie_case(*AA60)
    n, m, D = len(store_codes), len(reads), 5
    tax, lines = taxonomy_file(n, 21)
    lineage, names, parents = intern_taxonomy(n, lines)
    assert lineage.shape[1] == 5 and (lineage[9] == NONE).all()
    samples, weights = random_samples(m, 3, 4), random_weights(m, 5)
    fa, qa, db, packed, tx, sam, wei = (str(tmp_path / f) for f in ("s.fa", "q.fa", "s.db", "s.packed", "t.tsv", "s.tsv", "w.tsv"))
    synth.write_fasta(fa, store_codes, 1)
    synth.write_fasta(qa, reads, 1)
    for out, more in ((db, []), (packed, ["--packed"])):
        assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", out, "--alphabet", "aa", *more], capture_output=True).returncode == 0
    open(tx, "wb").write(tax)
    with open(sam, "wb") as f:
        f.write(b"".join(b"%d\t%d\n" % (q, samples[q]) for q in reversed(range(m)) if samples[q]))
    with open(wei, "wb") as f:
        f.write(b"".join(b"%d\t%d\textra\n" % (q, weights[q]) for q in range(m) if weights[q] != 1))
    base = ["classify", "-q", qa, "--max-divergence", str(D), "--taxonomy", tx, "--samples", sam, "--weights", wei]
    want = {slack: expected_classify(store_codes, reads, D, lineage, slack, samples, 3, weights, dmat=dmat) for slack in (0, 1)}
    assert (want[0][5] > 1).any() and ROOT in want[1][3] and NONE in want[0][3]
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, *base, "-d", path], capture_output=True)
        assert r.returncode == 0 and r.stdout == entry_lines(want[0][0], names, parents), r.stderr
        assert b"taxon entries of %d reads in 3 samples" % m in r.stderr
    r = subprocess.run([_lib.CLI_PATH, *base, "-d", db, "--slack", "1"], capture_output=True)
    assert r.returncode == 0 and r.stdout == entry_lines(want[1][0], names, parents), r.stderr
    r = subprocess.run([_lib.CLI_PATH, *base[:-6], "-d", db, "--slack", "1", "--per-read", "--taxonomy", "-"], input=tax, capture_output=True)
    plain = expected_classify(store_codes, reads, D, lineage, 1, dmat=dmat)
    assert r.returncode == 0 and r.stdout == per_read_lines(*plain[1:3], plain[5], plain[4], plain[3], names, parents), r.stderr
    out = str(tmp_path / "classified.tsv")
    with open(out, "wb") as f:
        smafa_amd.classify(db, qa, D, tx, samples_path=sam, weights_path=wei, out_fd=f.fileno())
    assert open(out, "rb").read() == entry_lines(want[0][0], names, parents)

    def refused(text, status, needle, args=None, stdin=None):
        bad = str(tmp_path / "bad.tsv")
        if text is not None:
            open(bad, "wb").write(text)
        argv = args or ["classify", "-d", db, "-q", qa, "--max-divergence", str(D), "--taxonomy", bad]
        r = subprocess.run([_lib.CLI_PATH, *argv], input=stdin, capture_output=True)
        assert r.returncode == status and needle in r.stderr and r.stdout == b"", (argv, r.stderr)

    refused(b"0\ta;b\n1\t" + b";".join(b"n%d" % k for k in range(17)) + b"\n", 1, b"smafa_classify: taxonomy line 2: more than 16 names")
    refused(b"0\t root ;b\n", 1, b"taxonomy line 1: the first name is \"root\" or \"unassigned\"")
    refused(b"0\tunassigned\n", 1, b"taxonomy line 1: the first name is")
    refused(b"0\ta\n%d\ta\n" % n, 1, b"taxonomy line 2: the sequence number is not one of the database's")
    refused(b"0\ta\n0\tb\n", 1, b"taxonomy line 2: a second line for this sequence")
    refused(None, 1, b"at most one of", args=[*base[:-6], "-d", db, "--taxonomy", "-", "--weights", "-"], stdin=b"")
    refused(None, 2, b"classify needs --taxonomy", args=["classify", "-d", db, "-q", qa, "--max-divergence", "5"])
    refused(None, 2, b"classify needs --max-divergence", args=["classify", "-d", db, "-q", qa, "--taxonomy", tx])
    short = str(tmp_path / "short.fa")
    synth.write_fasta(short, reads[:3, :50], 1)
    refused(None, 101, b"Cannot compute distances between seq of length 50 and windows of lengths 60",
            args=["classify", "-d", db, "-q", short, "--max-divergence", "5", "--taxonomy", tx])

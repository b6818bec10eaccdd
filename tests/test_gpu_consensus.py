"""The consensus of every labelled cluster of a resident store (smafa_db_consensus / smafa_db_consensus_launch / `smafa
consensus`): ids, sizes, one consensus row per cluster, the nearest member and every row's divergence from its consensus.

Expected values never come from the code under test (tests/consensus_cases.py): the model is the header's definition in plain
numpy on the code bytes, and every output is held to it byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import dense_store
from consensus_cases import (NONE, check_consensus, chunk_case, cluster_lines, edge_codes, edge_labels, expected_consensus,
                             random_grouping)
from self_join_cases import SHAPE_STORES, SHAPE_TABLE, SPANS_FAMILIES, replaned_case, shape_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["consensus::mark_groups_kernel", "consensus::group_ids_kernel", "consensus::group_keys_kernel", "consensus::segment_bounds_kernel"]
TALLY = {2: "consensus::tally_vote_kernel<2>", 3: "consensus::tally_vote_kernel<3>", 5: "consensus::tally_vote_kernel<5>"}
TABLES = {2: "consensus::vote_tables_kernel<2>", 3: "consensus::vote_tables_kernel<3>", 5: "consensus::vote_tables_kernel<5>"}
TAIL = ["consensus::measure_kernel", "consensus::finish_groups_kernel"]


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    if len(codes):
        store.push(codes)
    return store


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def kernels_of(planes, windows):
    return HEAD + [TALLY[planes]] + ([TABLES[planes]] if windows > 1 else []) + TAIL


@pytest.mark.parametrize("name,families,D,max_subs", SHAPE_STORES)
def test_every_shape_equals_the_model(name, families, D, max_subs):
    """every store shape (two, three and five planes, one to twenty-two words) under three labellings: the components at the
    store's bound, a random grouping that ignores similarity, and all singletons — which hold the whole inverse of perm[] and
    tab[] and the padding columns to account: the consensus of a row alone is the row"""
    codes, _ = shape_case(name, families, D, max_subs)
    kind, planes = SHAPE_TABLE[name][0], SHAPE_TABLE[name][3]
    n = len(codes)
    store = make_store(codes, kind)
    assert store.info().planes == planes
    components, count = store.self_components(D)
    assert check_consensus(codes, components, store.cluster_consensus(components)) == count
    assert store.last_call_kernels() == kernels_of(planes, -(-n // 4096))  # ("consensus::tally_vote_kernel<5>" on the amino-acid stores)
    check_consensus(codes, random_grouping(n, 100 + n), store.cluster_consensus(random_grouping(n, 100 + n)))
    ids, sizes, cons, nearest, div = store.cluster_consensus(np.arange(n, dtype=np.uint32))
    assert cons.tobytes() == codes.tobytes() and not div.any() and (sizes == 1).all()
    assert ids.tolist() == nearest.tolist() == list(range(n))
    store.close()


@pytest.mark.parametrize("kind", ["nt", "aa"])
def test_chunks_of_64(kind, monkeypatch):
    """SMAFA_CONSENSUS_CHUNK=64 on a 1 520-row store: a group of 600 (ten windows, the last short), one of exactly 64, one of 65
    and one label over all rows.  The bytes are the default setting's and the model's; the groups that cross a window's edge
    are voted by consensus::vote_tables_kernel<2> (nucleotides) and consensus::vote_tables_kernel<5> (amino acids)"""
    if kind == "nt":
        codes, labellings = chunk_case()
    else:
        codes, _ = shape_case("aa60", SPANS_FAMILIES, 5, 4)
        labellings = chunk_case()[1]
    planes = 2 if kind == "nt" else 5
    wide = make_store(codes, kind)
    monkeypatch.setenv("SMAFA_CONSENSUS_CHUNK", "64")  # (read when the handle is made)
    narrow = make_store(codes, kind)
    monkeypatch.delenv("SMAFA_CONSENSUS_CHUNK")
    for name, labels in labellings.items():
        got = narrow.cluster_consensus(labels)
        check_consensus(codes, labels, got)
        assert narrow.last_call_kernels() == kernels_of(planes, 24), name
        assert same_bytes(got, wide.cluster_consensus(labels))
        assert wide.last_call_kernels() == kernels_of(planes, 1), name
    wide.close()
    narrow.close()


@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 65])
@pytest.mark.parametrize("kind", ["nt", "aa"])
def test_word_and_tile_edges(kind, L):
    """the last column at and around a plane word's edge, the last row at and around a tile's: rows drawn over the whole
    alphabet (amino acids: all 28 codes), few groups, and all singletons"""
    for n in (1, 255, 256, 257, 513):
        codes = edge_codes(kind, n, L, 1000 * L + n)
        store = make_store(codes, kind)
        labels = edge_labels(n, n + L)
        check_consensus(codes, labels, store.cluster_consensus(labels))
        alone = np.arange(n, dtype=np.uint32)
        assert store.cluster_consensus(alone)[2].tobytes() == codes.tobytes()
        store.close()


def test_store_states(monkeypatch):
    """Two planes, three planes, and two re-planed to three by a later push that brings the first N.  Then a 5 000-row sorted
    push with an unsorted tail of three pushes of 100 rows, and — behind pushes that make up a quarter of the store, the last of
    them with N — the store the next scan sorts again.  5 000 rows and more are two windows of 4 096: one label over all rows
    crosses the edge and is voted by consensus::vote_tables_kernel<2>, and on the re-planed store by consensus::tally_vote_kernel<3>
    and consensus::vote_tables_kernel<3>."""
    pieces, _ = replaned_case()
    store = make_store(pieces[0], "nt")
    held = pieces[0]
    for piece, planes in ((None, 2), (pieces[1], 2), (pieces[2], 3)):
        if piece is not None:
            store.push(piece)
            held = np.concatenate([held, piece])
        assert store.info().planes == planes
        labels = random_grouping(len(held), len(held))
        check_consensus(held, labels, store.cluster_consensus(labels))
        assert store.last_call_kernels() == kernels_of(planes, 1)
    store.close()
    with_n = make_store(pieces[2], "nt")  # three planes from the first push on
    assert with_n.info().planes == 3 and (pieces[2] == 4).any()
    labels = random_grouping(len(pieces[2]), 5)
    check_consensus(pieces[2], labels, with_n.cluster_consensus(labels))
    with_n.close()

    monkeypatch.setenv("SMAFA_RESORT_MIN", "1000")  # (read when the handle is made)
    rng = np.random.default_rng(21)
    held = rng.integers(0, 4, size=(5000, 60)).astype(np.uint8)
    held[1::2] = held[0::2]  # pairs of equal rows: the sort brings them together, wherever they were pushed
    store = make_store(held, "nt")
    monkeypatch.delenv("SMAFA_RESORT_MIN")

    def check(planes):
        n = len(held)
        for labels in (random_grouping(n, n), np.full(n, n - 1, dtype=np.uint32)):
            check_consensus(held, labels, store.cluster_consensus(labels))
        assert store.last_call_kernels() == kernels_of(planes, 2) and store.info().planes == planes

    check(2)
    for k in range(3):
        tail = held[rng.integers(0, len(held), size=100)].copy()
        tail[:, k] = (tail[:, k] + 1) % 4
        store.push(tail)
        held = np.concatenate([held, tail])
        check(2)
    more = held[rng.integers(0, len(held), size=1500)].copy()
    more[::7, 5] = 4  # the first N
    store.push(more)
    held = np.concatenate([held, more])
    check(3)
    store.scan(held[:4], max_divergence=2)  # a quarter of the store has arrived since the sort: this scan sorts it again
    check(3)
    store.close()


def test_dense_store():
    """2 000 copies each of two rows at distance 3.  Labelled by group: the two consensus rows are the two rows, every div is 0
    and the nearest member is the first copy.  One label over all rows: a 2 000-2 000 tie in each of the three differing
    columns, which goes to the smaller code.  The kernels are consensus::mark_groups_kernel, consensus::group_ids_kernel,
    consensus::group_keys_kernel, consensus::segment_bounds_kernel, consensus::tally_vote_kernel<2>, consensus::measure_kernel
    and consensus::finish_groups_kernel, in this order (4 000 rows are one window: no table is voted)."""
    codes, group = dense_store()
    store = make_store(codes, "nt")
    first = [int(np.flatnonzero(group == g)[0]) for g in (0, 1)]
    labels = np.where(group == 0, first[0], first[1]).astype(np.uint32)
    got = store.cluster_consensus(labels)
    check_consensus(codes, labels, got)
    ids, sizes, cons, nearest, div = got
    by_id = np.argsort(first)
    assert ids.tolist() == sorted(first) and sizes.tolist() == [2000, 2000] and nearest.tolist() == sorted(first) and not div.any()
    assert cons.tobytes() == codes[np.array(first)[by_id]].tobytes()
    assert store.last_call_kernels() == HEAD + ["consensus::tally_vote_kernel<2>"] + TAIL
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    assert stats["launches"] == store.last_scan_ms()[1] == 9 and stats["scans"] == 0
    everything = np.zeros(len(codes), dtype=np.uint32)
    ids, sizes, cons, nearest, div = got = store.cluster_consensus(everything)
    check_consensus(codes, everything, got)
    a, b = codes[first[0]], codes[first[1]]
    assert cons.tobytes() == np.minimum(a, b).tobytes() and (a != b).sum() == 3 and sizes.tolist() == [4000]
    assert sorted(set(div.tolist())) == sorted({int((a != cons[0]).sum()), int((b != cons[0]).sum())})
    # the optional outputs left out: no measure pass
    ids2, sizes2, cons2, none_a, none_b = store.cluster_consensus(everything, nearest=False, div=False)
    assert none_a is None and none_b is None and same_bytes((ids2, sizes2, cons2), (ids, sizes, cons))
    assert store.last_call_kernels() == HEAD + ["consensus::tally_vote_kernel<2>", "consensus::finish_groups_kernel"]
    store.close()


def test_the_same_bytes_twice_and_between_other_calls():
    """one handle: the call twice, then behind a density call, a neighbours call, a stable-clusters call and a query, which use
    the same handle-owned buffers (the sort's, sort_tmp, the kept list, pos_of[]) — and those calls' own answers behind it"""
    codes, _ = shape_case("nt330n", SPANS_FAMILIES, 5, 4)
    store = make_store(codes, "nt")
    labels = random_grouping(len(codes), 3)
    first = store.cluster_consensus(labels)
    check_consensus(codes, labels, first)
    assert same_bytes(store.cluster_consensus(labels), first)
    others = {
        "density": lambda: store.self_density(5, 3),
        "neighbours": lambda: store.self_neighbours(5, 4),
        "stable": lambda: store.self_stable_clusters(5, 3, 0, joined=True, cores=True),
        "query": lambda: (store.scan(codes[:50], max_divergence=5),),
    }
    flat = lambda out: [np.asarray(x).tobytes() for x in out]  # noqa: E731
    before = {}
    for name, call in others.items():
        before[name] = flat(call())
        assert same_bytes(store.cluster_consensus(labels), first), name
    for name, call in others.items():  # each of them directly behind a consensus call
        store.cluster_consensus(labels)
        assert flat(call()) == before[name], name
    store.close()


def test_tiny_and_unlabelled_stores():
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    ids, sizes, cons, nearest, div = store.cluster_consensus(np.zeros(0, dtype=np.uint32))  # no row
    assert ids.shape == sizes.shape == nearest.shape == div.shape == (0,) and cons.shape == (0, 60)
    codes = edge_codes("nt", 300, 60, 8)
    store.push(codes)
    nothing = np.full(300, NONE, dtype=np.uint32)
    ids, sizes, cons, nearest, div = store.cluster_consensus(nothing)
    assert len(ids) == len(sizes) == len(nearest) == 0 and cons.shape == (0, 60) and (div == NONE).all() and div.shape == (300,)
    with pytest.raises(smafa_amd.SmafaError) as e:
        bad = np.full(300, NONE, dtype=np.uint32)
        bad[[290, 17, 200]] = [300, 301, 5000]
        store.cluster_consensus(bad)
    assert e.value.code == _lib.ERR_INVALID and "labels[17] is 301" in str(e.value)
    with pytest.raises(ValueError):
        store.cluster_consensus(nothing[:299])
    store.close()


@pytest.mark.parametrize("kind", ["nt", "aa"])
def test_cli_consensus(tmp_path, kind):
    """`smafa stable ... | smafa consensus -d DB --labels -` and `--labels FILE` against lines built from the model; a labels
    file with a missing line, an out-of-order line or a label >= n exits 1 and names the line"""
    from stable_cases import expected_stable, planted_codes

    codes = planted_codes("aa" if kind == "aa" else "ntn")
    n = len(codes)
    D, M = 5, 2
    labels = expected_stable(codes, D, M, 0)[0]
    assert (labels == NONE).any() and len(np.unique(labels)) > 2
    letters = b"ACGTN" if kind == "nt" else bytes(smafa_amd.decode(np.arange(28, dtype=np.uint8), smafa_amd.ALPHABET_AA))
    want = cluster_lines(codes, labels, letters)
    fa, db, packed, tsv = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed", "labels.tsv"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    stable = subprocess.run([_lib.CLI_PATH, "stable", "-d", db, "--max-divergence", str(D), "--min-pts", str(M), "--joined"], capture_output=True)
    assert stable.returncode == 0
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, "consensus", "-d", path, "--labels", "-"], input=stable.stdout, capture_output=True)
        assert r.returncode == 0 and r.stdout == want, r.stderr
    lines = [b"%d\t%d\n" % (i, -1 if v == NONE else v) for i, v in enumerate(labels.tolist())]
    with open(tsv, "wb") as f:
        f.write(b"".join(lines))
    r = subprocess.run([_lib.CLI_PATH, "consensus", "-d", db, "--labels", tsv], capture_output=True)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    out = str(tmp_path / "consensus.tsv")
    with open(out, "wb") as f:
        smafa_amd.consensus(db, tsv, out_fd=f.fileno())
    assert open(out, "rb").read() == want
    swapped = lines[:8] + [lines[9], lines[8]] + lines[10:]
    over = lines[:12] + [b"12\t%d\n" % n] + lines[13:]
    for text, line in ((lines[:5] + lines[6:], 6), (swapped, 9), (over, 13), (lines[:-1], n), (lines + [b"%d\t0\n" % n], n + 1)):
        with open(tsv, "wb") as f:
            f.write(b"".join(text))
        r = subprocess.run([_lib.CLI_PATH, "consensus", "-d", db, "--labels", tsv], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and (b"labels line %d:" % line) in r.stderr, (line, r.stderr)
    r = subprocess.run([_lib.CLI_PATH, "consensus", "-d", db], capture_output=True)
    assert r.returncode == 2 and b"consensus needs --labels" in r.stderr

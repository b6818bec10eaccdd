"""Expected values and case builders of the consensus tests (tests/test_consensus_model.py, tests/test_gpu_consensus.py,
tests/test_consensus_abi.py, tests/consensus_worker.py).

Nothing here comes from the code under test: expected_consensus restates the definition of include/smafa_amd.h in plain numpy
on the code bytes — per group a bincount per column, argmax (whose FIRST maximum is the tie rule: the smallest code) and
`(row != consensus).sum(1)`."""
import functools

import numpy as np

NONE = 0xFFFFFFFF
CHUNK_ROWS = 1520  # the store of the chunk tests: self_join_cases' 150 families


def column_counts(rows):
    """counts[c, v] = how many of `rows` hold code v at column c: one bincount over (column, code)"""
    L = rows.shape[1]
    return np.bincount((np.arange(L)[None, :] * 32 + rows).ravel(), minlength=L * 32).reshape(L, 32)


def expected_consensus(codes, labels):
    """-> (ids, sizes, consensus[K, L] uint8, nearest, div) of code rows `codes` (n x L uint8) under `labels` (n uint32)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    labels = np.asarray(labels, dtype=np.uint32)
    n, L = codes.shape
    assert labels.shape == (n,) and ((labels == NONE) | (labels < n)).all()
    ids = np.unique(labels[labels != NONE]).astype(np.uint32)
    K = len(ids)
    sizes, nearest = np.zeros(K, dtype=np.uint32), np.zeros(K, dtype=np.uint32)
    cons = np.zeros((K, L), dtype=np.uint8)
    div = np.full(n, NONE, dtype=np.uint32)
    for k, r in enumerate(ids.tolist()):
        members = np.flatnonzero(labels == r)  # ascending subject numbers
        rows = codes[members]
        counts = column_counts(rows)
        cons[k] = counts.argmax(axis=1)  # the first maximum: the smallest code among the most frequent
        d = (rows != cons[k][None, :]).sum(axis=1)
        sizes[k] = len(members)
        div[members] = d
        nearest[k] = members[d.argmin()]  # the first minimum: the smallest subject number among the nearest
    return ids, sizes, cons, nearest, div


def check_consensus(codes, labels, got):
    """got = SubjectStore.cluster_consensus(labels): every array equal to the model's, byte for byte; -> K"""
    want = expected_consensus(codes, labels)
    names = ("ids", "sizes", "codes", "nearest", "div")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            where = np.argwhere(g != w)[:5].tolist()
            raise AssertionError("%s differs at %s: got %s, want %s" % (name, where, g[tuple(np.array(where).T)], w[tuple(np.array(where).T)]))
    return len(want[0])


def random_grouping(n, seed, big=600):
    """A seeded grouping that ignores similarity: groups of 1, 2, 3, 63, 64 and 65 rows and one of `big` (what n leaves of
    it; everything, where n is small), the other rows in groups of 1 .. 8, a tenth of all rows SMAFA_NONE, and the label VALUES
    drawn among all subject numbers, non-members included.  -> labels (uint32, n)"""
    rng = np.random.default_rng(seed)
    rows = rng.permutation(n)
    none = rows[: n // 10]
    rows = rows[n // 10:]
    sizes = []
    for s in (1, 2, 3, 63, 64, 65, big):
        if sum(sizes) + s <= len(rows):
            sizes.append(s)
    while sum(sizes) < len(rows):
        sizes.append(min(int(rng.integers(1, 9)), len(rows) - sum(sizes)))
    values = rng.choice(n, size=len(sizes), replace=False)
    labels = np.full(n, NONE, dtype=np.uint32)
    labels[rows] = np.repeat(values, sizes).astype(np.uint32)
    labels[none] = NONE
    return labels


def tied_columns(codes, labels):
    """how many (group, column) votes end in a tie for the greatest count — what the tie rule decides"""
    ties = 0
    for r in np.unique(labels[labels != NONE]).tolist():
        rows = codes[labels == r]
        counts = column_counts(rows)
        ties += int(((counts == counts.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return ties


@functools.lru_cache(maxsize=None)
def chunk_case():
    """-> (codes, {name: labels}) on the 1 520-row nt60 store: `random` (a group of 600 — ten windows of 64, the last short —
    one of exactly 64, one of 65, singletons, a tenth unlabelled) and `one` (one label over all rows, value 7)"""
    from self_join_cases import SPANS_FAMILIES, shape_case

    codes, _ = shape_case("nt60", SPANS_FAMILIES, 5, 4)
    assert len(codes) == CHUNK_ROWS
    random = random_grouping(len(codes), 11)
    one = np.full(len(codes), 7, dtype=np.uint32)
    return codes, {"random": random, "one": one}


def edge_codes(kind, n, L, seed):
    """n rows of L columns drawn over the whole alphabet: amino acids over all 28 codes, nucleotides over A C G T N"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 28 if kind == "aa" else 5, size=(n, L)).astype(np.uint8)


def edge_labels(n, seed):
    """few groups, so that every column of a small store has counts worth voting on, ties included; some rows unlabelled"""
    rng = np.random.default_rng(seed)
    values = rng.choice(n, size=min(n, 3), replace=False)
    labels = values[rng.integers(0, len(values), size=n)].astype(np.uint32)
    if n > 4:
        labels[rng.choice(n, size=n // 8, replace=False)] = NONE
    return labels


def cluster_lines(codes, labels, alphabet_letters):
    """the lines `smafa consensus` prints: "label\\tsize\\tnearest\\tmax_div\\tSEQUENCE" per cluster, from the model"""
    ids, sizes, cons, nearest, div = expected_consensus(codes, labels)
    out = []
    for k, r in enumerate(ids.tolist()):
        worst = int(div[labels == r].max())
        seq = bytes(alphabet_letters[c] for c in cons[k].tolist())
        out.append(b"%d\t%d\t%d\t%d\t%s\n" % (r, sizes[k], nearest[k], worst, seq))
    return b"".join(out)

"""Stores and expected rows of the delta self-join tests (tests/test_gpu_delta_join.py, tests/delta_worker.py, and the CPU model
tests/test_delta_model.py).

Nothing is expected from the code under test: the rows of a delta call at first_row are the brute-force pairs of the code
bytes (tests/self_join_cases.py: brute_pairs) whose larger subject number is >= first_row, and the labels are those of a
plain union-find over brute-force pairs (tests/components_cases.py: brute_labels)."""
import functools
import os
import tempfile

import numpy as np

from self_join_cases import SHAPES, brute_pairs, planted_store

FAMILIES = 300  # 3 020 rows


def kind_of(name):
    return next(s for s in SHAPES if s[0] == name)[1]


@functools.lru_cache(maxsize=None)
def store_case(name, families=FAMILIES):
    """-> (codes, expected rows of the whole store, D) of a shape of SHAPES at `families` x 10 + 20 rows"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    codes = planted_store(11 + families + len(name), kind, L, families, n_frac)
    want = brute_pairs(codes, D)
    assert len(want) > 0 and set(np.unique(want["dist"])) == set(range(D + 1)), (name, np.unique(want["dist"]))
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, want, D


def marks(n):
    """the first_row values of the issue's case 1"""
    return [0, 1, n // 2, n - 300, n - 1, n]


def since(want, first_row):
    """the rows of `want` (ordered (i, dist, j), i < j) with j >= first_row, in the same order"""
    return np.ascontiguousarray(want[want["subject"] >= first_row])


def has_both_kinds(rows, first_row, D):
    """old-new pairs (i < first_row <= j) and new-new pairs (first_row <= i) at every distance 0..D"""
    old_new = rows[(rows["query"] < first_row) & (rows["subject"] >= first_row)]
    new_new = rows[rows["query"] >= first_row]
    return set(np.unique(old_new["dist"])) == set(range(D + 1)) and set(np.unique(new_new["dist"])) == set(range(D + 1))


def pair_keys(rows):
    """one int64 per row: rows of exactly-once lists have distinct keys"""
    return (rows["query"].astype(np.int64) << 32) | rows["subject"].astype(np.int64)


def delta_filter(list_rows, rows_of):
    """numpy model of smafa_dl::delta_filter_kernel.  list_rows: HIT_DTYPE rows {query = record r, subject = s, dist} as a
    scan of the records against the whole store leaves them (self-pairs and mirror images included); rows_of[r] = the subject
    number of record r.  Kept iff s < rows_of[r], and it leaves as {s, rows_of[r], dist}."""
    a = rows_of[list_rows["query"]]
    keep = list_rows["subject"] < a
    out = np.zeros(int(keep.sum()), dtype=list_rows.dtype)
    out["query"], out["subject"], out["dist"] = list_rows["subject"][keep], a[keep], list_rows["dist"][keep]
    return out


def seed_and_link(labels, first_row, n, pairs):
    """numpy / plain-Python model of seed_parents_kernel + link_rows_kernel + flatten_labels_kernel: parent[i] = labels[i] for
    i < first_row and i behind it, the larger root hooked under the smaller for every pair, labels = roots.
    -> (labels of n rows, number of violations the seed counts)"""
    labels = np.asarray(labels, dtype=np.int64)
    parent = np.arange(n, dtype=np.int64)
    bad = 0
    for i in range(first_row):
        l = labels[i]
        if l > i or l >= first_row or labels[l] != l:
            bad += 1
        else:
            parent[i] = l

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        ra, rb = root(int(a)), root(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([root(i) for i in range(n)], dtype=np.uint32), bad


def library_log(fn):
    """fn() with the library's level-2 lines (stderr) captured -> (fn's result, the text)"""
    from smafa_amd import _lib

    lib = _lib.lib()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        lib.smafa_set_verbosity(2)
        try:
            out = fn()
        finally:
            lib.smafa_set_verbosity(0)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")

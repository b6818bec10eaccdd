"""The model and the fixtures of the abundance-table tests (tests/test_assign_model.py, tests/test_gpu_assign.py,
tests/test_assign_abi.py).

The expected answer never comes from the library: it is worked in numpy from the code bytes.  The distance of a read and a
subject is the number of columns whose codes differ; a read is assigned to the subject at the smallest distance within
the bound — numpy's argmin returns the first index of the minimum, the smaller subject number —, its label is the label of that
subject, SMAFA_NONE without one, and the table is np.unique over the (label, sample) keys of the reads of weight > 0 with their
weights summed."""
import functools

import numpy as np

from self_join_cases import shape_case

NONE = 0xFFFFFFFF
TABLE_DTYPE = np.dtype([("label", "<u4"), ("sample", "<u4"), ("count", "<u8")])
ASSIGN_KERNELS = ["assign::init_kernel", "assign::best_kernel", "assign::bin_kernel", "assign::heads_kernel", "assign::fold_kernel"]


def nearest(subject_codes, read_codes, D, slab=64):
    """-> (subject, dist), uint32 per read: the subject at the smallest distance <= D, the smaller number on a tie; NONE, NONE
    without one"""
    subjects = np.ascontiguousarray(subject_codes, dtype=np.uint8)
    reads = np.ascontiguousarray(read_codes, dtype=np.uint8).reshape(-1, subjects.shape[1])
    m = len(reads)
    subject, dist = np.full(m, NONE, dtype=np.uint32), np.full(m, NONE, dtype=np.uint32)
    if len(subjects) == 0:
        return subject, dist
    for a in range(0, m, slab):
        d = (reads[a:a + slab, None, :] != subjects[None, :, :]).sum(-1)
        arg = d.argmin(axis=1)
        low = d[np.arange(len(arg)), arg]
        ok = low <= D
        subject[a:a + slab][ok] = arg[ok]
        dist[a:a + slab][ok] = low[ok]
    return subject, dist


def expected_assign(subject_codes, read_codes, D, labels=None, samples=None, n_samples=None, weights=None):
    """-> (entries, subject, dist, subject_counts, totals) as the contract of include/smafa_amd.h defines them"""
    n = len(subject_codes)
    subject, dist = nearest(subject_codes, read_codes, D)
    m = len(subject)
    samples = np.zeros(m, dtype=np.uint32) if samples is None else np.asarray(samples, dtype=np.uint32)
    weights = np.ones(m, dtype=np.uint32) if weights is None else np.asarray(weights, dtype=np.uint32)
    if n_samples is None:
        n_samples = int(samples.max()) + 1 if m else 1
    labels = np.arange(n, dtype=np.uint32) if labels is None else np.asarray(labels, dtype=np.uint32)
    found = subject != NONE
    read_label = np.full(m, NONE, dtype=np.uint32)
    read_label[found] = labels[subject[found]]
    stray = samples >= n_samples  # such a read takes no part in anything but totals[3]
    w = np.where(stray, 0, weights).astype(np.uint64)
    live = w > 0
    keys = (read_label[live].astype(np.uint64) << np.uint64(32)) | samples[live].astype(np.uint64)
    uniq, inverse = np.unique(keys, return_inverse=True)
    entries = np.zeros(len(uniq), dtype=TABLE_DTYPE)
    entries["label"] = (uniq >> np.uint64(32)).astype(np.uint32)
    entries["sample"] = (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    np.add.at(entries["count"], inverse, w[live])
    subject_counts = np.zeros(n, dtype=np.uint64)
    np.add.at(subject_counts, subject[found], w[found])
    totals = np.array([len(entries), w[found].sum(), w[~found].sum(), stray.sum()], dtype=np.uint64)
    return entries, subject, dist, subject_counts, totals


def planted_reads(codes, D, m, seed, strangers=None):
    """m reads of a store: rows of it with 0 .. D + 2 substituted columns (distinct columns, each to another code that occurs in
    the store), so that every distance 0 .. D occurs and some reads fall outside the bound, and `strangers` (default m // 10)
    unrelated random rows; shuffled"""
    rng = np.random.default_rng(seed)
    codes = np.asarray(codes)
    n, L = codes.shape
    letters = np.unique(codes[codes != 4]) if codes.max() <= 4 else np.unique(codes)
    strangers = m // 10 if strangers is None else strangers
    k = m - strangers
    reads = codes[rng.integers(0, n, size=k)].copy()
    subs = np.arange(k) % (D + 3)
    for r in range(k):
        cols = rng.choice(L, size=min(int(subs[r]), L), replace=False)
        for c in cols:
            reads[r, c] = rng.choice(letters[letters != reads[r, c]])
    reads = np.concatenate([reads, letters[rng.integers(0, len(letters), size=(strangers, L))]])
    rng.shuffle(reads, axis=0)
    return np.ascontiguousarray(reads, dtype=np.uint8)


def random_samples(m, n_samples, seed):
    return np.random.default_rng(seed).integers(0, n_samples, size=m).astype(np.uint32)


def random_weights(m, seed):
    return np.random.default_rng(seed).integers(0, 6, size=m).astype(np.uint32)  # 0 .. 5: some reads weigh nothing


SHAPE_READS = 260  # reads per store of the every-shape test: five waves, the last short


@functools.lru_cache(maxsize=None)
def shape_reads(name, families, D, max_subs=4):
    """-> (store codes, reads, subject, dist) of a store of self_join_cases.SHAPE_STORES"""
    codes, _ = shape_case(name, families, D, max_subs)
    reads = planted_reads(codes, D, SHAPE_READS, 4000 + families + D + len(name))
    subject, dist = nearest(codes, reads, D)
    for a in (reads, subject, dist):
        a.setflags(write=False)
    return codes, reads, subject, dist


def check_against_oracle(subject_codes, read_codes, D, subject, dist, sample=64, seed=5):
    """oracle.scan_codes on a sample of the reads must give the model's subject and dist: its first row per query, in its
    (query, dist, subject) order, is the assignment"""
    import oracle

    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(len(read_codes), size=min(sample, len(read_codes)), replace=False))
    got = oracle.scan_codes(np.ascontiguousarray(subject_codes), np.ascontiguousarray(read_codes[pick]), D)
    for k, q in enumerate(pick):
        mine = got[got["query"] == k]
        if len(mine) == 0:
            assert subject[q] == NONE and dist[q] == NONE, q
        else:
            assert (int(mine["subject"][0]), int(mine["dist"][0])) == (int(subject[q]), int(dist[q])), q


def table_lines(entries):
    return b"".join(b"%d\t%d\t%d\n" % (-1 if e["label"] == NONE else e["label"], e["sample"], e["count"]) for e in entries)


def read_lines(subject, dist):
    return b"".join(b"%d\t%d\t%d\n" % (q, -1 if s == NONE else s, -1 if s == NONE else d) for q, (s, d) in enumerate(zip(subject, dist)))


def sequence_lines(subject_counts):
    return b"".join(b"%d\t%d\n" % (i, c) for i, c in enumerate(subject_counts))

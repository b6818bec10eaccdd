"""Expected labels of the components tests (tests/test_gpu_components.py, tests/components_worker.py).

Nothing here comes from the code under test: the edges are self_join_cases.brute_pairs — brute force on the code bytes —
and the labels a plain union-find over them, label = the smallest member of the set."""
import numpy as np

from self_join_cases import brute_pairs


def labels_from_pairs(n, rows):
    """rows (HIT_DTYPE or anything with "query" / "subject") -> uint32 labels[n]: the smallest member of each row's set.
    A textbook union-find: the larger root goes under the smaller, so a root is its set's minimum."""
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b in zip(rows["query"].tolist(), rows["subject"].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], dtype=np.uint32)


def labels_from_pairs_numpy(n, rows):
    """the same labels for row lists too long for a Python loop: every subject takes the smallest label among itself and
    its neighbours' roots, then labels = labels[labels] until flat, until no edge joins two roots (only edges whose ends
    still differ stay in play)"""
    labels = np.arange(n, dtype=np.int64)
    i, j = rows["query"].astype(np.int64), rows["subject"].astype(np.int64)
    while len(i):
        li, lj = labels[i], labels[j]  # roots: labels is flat here
        m = np.minimum(li, lj)
        np.minimum.at(labels, li, m)   # the larger root goes under the smallest root that reaches it
        np.minimum.at(labels, lj, m)
        while True:
            jumped = labels[labels]
            if (jumped == labels).all():
                break
            labels = jumped
        open_ = labels[i] != labels[j]
        i, j = i[open_], j[open_]
    return labels.astype(np.uint32)


def brute_labels(codes, D):
    """-> (labels, pairs) of a store at bound D"""
    pairs = brute_pairs(codes, D)
    return labels_from_pairs(len(codes), pairs), pairs


def n_components(labels):
    return int((labels == np.arange(len(labels))).sum())


def widest_chained_component(codes, labels, D):
    """(size, diameter) of a component of >= 3 rows whose two farthest members are more than D apart — rows joined only
    THROUGH other rows, what single linkage adds to a star around a centre — or None"""
    order = np.argsort(labels, kind="stable")
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    for members in np.split(order, cuts):
        if len(members) < 3:
            continue
        rows = codes[members[:512]]
        far = int((rows[:, None, :] != rows[None, :, :]).sum(axis=2).max())
        if far > D:
            return len(members), far
    return None


def chain_store(seed, chains=3, rows_per_chain=2048, L=60):
    """`chains` independent chains of 2-bit nucleotide rows: row k of a chain is its row k - 1 with column k % L set to
    (old + 1) % 4, so neighbours in a chain are at distance exactly 1; the chains are shuffled together.
    -> (codes, chain number of every row)"""
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(chains):
        row = rng.integers(0, 4, size=L).astype(np.uint8)
        rows = [row.copy()]
        for k in range(1, rows_per_chain):
            row[k % L] = (row[k % L] + 1) % 4
            rows.append(row.copy())
        blocks.append(np.array(rows, dtype=np.uint8))
    codes = np.concatenate(blocks)
    which = np.repeat(np.arange(chains), rows_per_chain)
    perm = rng.permutation(len(codes))
    return np.ascontiguousarray(codes[perm]), which[perm]


def dense_store():
    """the store of the self-join's dense test (tests/test_gpu_self_join.py): 2 000 copies of one row and 2 000 of a second
    row at distance 3, shuffled -> (codes, group of every row)"""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 4, size=60).astype(np.uint8)
    b = a.copy()
    b[[3, 30, 59]] = (b[[3, 30, 59]] + 1) % 4
    group = rng.permutation(np.repeat([0, 1], 2000))
    return np.where(group[:, None] == 0, a[None, :], b[None, :]).astype(np.uint8), group

"""Stores and expected rows of the self-join tests (tests/test_gpu_self_join.py, tests/self_join_worker.py).

The expected pairs never come from the code under test: they are the brute-force distances of the code bytes — the number
of columns whose codes differ.  For a store of n rows that is n^2 / 2 comparisons of L columns; numpy does them
slab by slab as a product of one-hot matrices (matches[a, b] = sum over columns and letters of onehot[a] * onehot[b], small
integers, exact in float32) and every pair that comes out within the bound is then recomputed literally, `(a != b).sum()`,
and asserted equal."""
import numpy as np

from smafa_amd import HIT_DTYPE, synth


def planted_store(seed, kind, L, families, n_frac=0.0, members=10, max_subs=4, copies=20):
    """`families` random seed rows x `members` members, each member = its seed with 0..max_subs substituted columns
    (distinct columns, each to a different letter), plus `copies` exact copies of random members; shuffled.  kind: "nt"
    (codes 0..3, with n_frac of the seeds' cells set to N = 4) or "aa"."""
    rng = np.random.default_rng(seed)
    lc = synth.letter_codes(1 if kind == "aa" else 0)
    idx = rng.integers(0, len(lc), size=(families, L))
    rows = np.repeat(idx, members, axis=0)
    n = len(rows)
    subs = rng.integers(0, max_subs + 1, size=n)
    perm = np.argsort(rng.random(size=(n, L)), axis=1)[:, :max_subs]
    shift = rng.integers(1, len(lc), size=(n, max_subs))
    for s in range(max_subs):
        who = np.nonzero(subs > s)[0]
        rows[who, perm[who, s]] = (rows[who, perm[who, s]] + shift[who, s]) % len(lc)
    codes = lc[rows]
    if n_frac > 0:
        mask = np.repeat(rng.random(size=(families, L)) < n_frac, members, axis=0)
        codes[mask] = 4  # the family's N columns: shared by its members
    codes = np.concatenate([codes, codes[rng.integers(0, n, size=copies)]])
    rng.shuffle(codes, axis=0)
    return np.ascontiguousarray(codes, dtype=np.uint8)


def brute_pairs(codes, D, slab=1024):
    """every pair i < j with (codes[i] != codes[j]).sum() <= D as HIT_DTYPE rows ordered (i, dist, j)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, L = codes.shape
    letters = np.unique(codes)
    remap = np.zeros(256, dtype=np.int64)
    remap[letters] = np.arange(len(letters))
    onehot = np.zeros((n, L * len(letters)), dtype=np.float32)
    cols = np.arange(L)[None, :] * len(letters) + remap[codes]
    onehot[np.arange(n)[:, None], cols] = 1.0
    out_i, out_j, out_d = [], [], []
    for a in range(0, n, slab):
        b = min(n, a + slab)
        dist = L - (onehot[a:b] @ onehot[a:].T)  # rows a..b against rows a..n: the upper triangle's share
        ii, jj = np.nonzero(dist <= D)
        ii += a
        jj += a
        keep = ii < jj
        ii, jj = ii[keep], jj[keep]
        literal = (codes[ii] != codes[jj]).sum(axis=1)
        assert (literal == dist[ii - a, jj - a]).all()
        out_i.append(ii)
        out_j.append(jj)
        out_d.append(literal)
    i, j, d = (np.concatenate(x) if x else np.zeros(0, np.int64) for x in (out_i, out_j, out_d))
    order = np.lexsort((j, d, i))
    rows = np.zeros(len(order), dtype=HIT_DTYPE)
    rows["query"], rows["subject"], rows["dist"] = i[order], j[order], d[order]
    return rows


def check_against_oracle(codes, rows, D, sample=64, seed=5):
    """oracle.scan_codes on a sample of the same rows must give the brute-force neighbours"""
    import oracle

    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(len(codes), size=min(sample, len(codes)), replace=False))
    got = oracle.scan_codes(codes, codes[pick], D)
    for k, i in enumerate(pick):
        mine = got[got["query"] == k]
        mine = mine[mine["subject"] != i]
        lo = rows[rows["query"] == i]
        hi = rows[rows["subject"] == i]
        want = sorted([(int(r["subject"]), int(r["dist"])) for r in lo] + [(int(r["query"]), int(r["dist"])) for r in hi])
        assert sorted((int(r["subject"]), int(r["dist"])) for r in mine) == want, i


def sort_rows(rows):
    """device rows (n x 3 uint32: query, subject, dist) -> HIT_DTYPE ordered (query, dist, subject)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 3)
    order = np.lexsort((rows[:, 1], rows[:, 2], rows[:, 0]))
    return np.ascontiguousarray(rows[order]).view(HIT_DTYPE).reshape(-1)


# (name, kind, L, D, n_frac): the shapes of the issue's case 1
SHAPES = [
    ("nt60", "nt", 60, 5, 0.0),     # 2 planes
    ("nt60n", "nt", 60, 5, 0.01),   # N in 1 % of the columns: 3 planes
    ("aa60", "aa", 60, 5, 0.0),
    ("nt9", "nt", 9, 2, 0.0),       # one word
    ("nt130", "nt", 130, 6, 0.0),   # wide kernel
    ("aa60d0", "aa", 60, 0, 0.0),   # copies only
]

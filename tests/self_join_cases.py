"""Stores and expected rows of the self-join tests (tests/test_gpu_self_join.py, tests/self_join_worker.py, and — the second
table, SHAPE_TABLE — tests/test_gpu_self_join_shapes.py with its CPU model tests/test_self_join_shapes_model.py).

The expected pairs never come from the code under test: they are the brute-force distances of the code bytes — the number
of columns whose codes differ.  For a store of n rows that is n^2 / 2 comparisons of L columns; numpy does them
slab by slab as a product of one-hot matrices (matches[a, b] = sum over columns and letters of onehot[a] * onehot[b], small
integers, exact in float32) and every pair that comes out within the bound is then recomputed literally, `(a != b).sum()`,
and asserted equal."""
import functools

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


# ---- the second table: store SHAPES.  What differs between its rows is not what the rows hold but how wide a query record is
# (QS words, transposed through LDS in windows of 32 by store_records_kernel), how many planes the store keeps, and how many
# words a plane has (W: which scan instantiation runs).  tests/test_self_join_shapes_model.py derives the last four columns
# from the layout functions of kernels.hip.h and says what each shape reaches.
# name -> (kind, L, n_frac, planes stored, planes of a query record, W, QS)
SHAPE_TABLE = {
    "aa200": ("aa", 200, 0.0, 5, 5, 7, 36),     # two windows, the last of 4 words
    "aa224": ("aa", 224, 0.0, 5, 5, 7, 36),     # the same, with the last column word full
    "aa250": ("aa", 250, 0.0, 5, 5, 8, 44),     # last window of 12 words
    "aa700": ("aa", 700, 0.0, 5, 5, 22, 112),   # four windows
    "nt330": ("nt", 330, 0.0, 2, 3, 11, 36),    # second window: only slots of the plane the store does not keep
    "nt330n": ("nt", 330, 0.01, 3, 3, 11, 36),  # the same slots now hold stored words
    "nt520": ("nt", 520, 0.0, 2, 3, 17, 52),    # two-plane store with stored words in the second window
    "aa20": ("aa", 20, 0.0, 5, 5, 1, 8),        # one-word amino-acid records
    "nt90": ("nt", 90, 0.0, 2, 3, 3, 12),
    "nt120": ("nt", 120, 0.0, 2, 3, 4, 16),
    "aa90": ("aa", 90, 0.0, 5, 5, 3, 16),
    "aa120": ("aa", 120, 0.0, 5, 5, 4, 24),
    "nt130": ("nt", 130, 0.0, 2, 3, 5, 16),     # the shapes of SHAPES: wide kernel, and the two that are pinned everywhere
    "nt60": ("nt", 60, 0.0, 2, 3, 2, 8),
    "aa60": ("aa", 60, 0.0, 5, 5, 2, 12),
}
REC_WINDOW = 32  # join.hip.h kRecWindow
WIDE_SHAPES = [n for n, s in SHAPE_TABLE.items() if s[4] * s[5] >= REC_WINDOW]  # records of more than one window
NARROW_SHAPES = [n for n, s in SHAPE_TABLE.items() if s[5] <= 4]                 # the per-length scan instantiations
ONE_SPAN_FAMILIES, SPANS_FAMILIES, SORTED_FAMILIES = 100, 150, 500               # 1 020, 1 520 and 5 020 rows
LOOSE_BOUND, LOOSE_SUBS = 20, 10  # members up to 10 columns from their seed: distances up to 20 between members


def shape_bound(name):
    return 2 if name == "aa20" else 5  # (20 columns: level 1 of the prefilter prunes up to bound 3)


# every store of tests/test_gpu_self_join_shapes.py, as the arguments of shape_case: (name, families, D, max_subs)
SHAPE_STORES = ([(n, ONE_SPAN_FAMILIES, 5, 4) for n in WIDE_SHAPES] + [(n, SPANS_FAMILIES, shape_bound(n), 4) for n in SHAPE_TABLE] +
                [(n, SPANS_FAMILIES, LOOSE_BOUND, LOOSE_SUBS) for n in ("aa200", "nt520")] + [("nt330", SORTED_FAMILIES, 3, 4)])
RESEED = {}  # (name, families, D, max_subs) -> seed, for a store whose default seed misses a distance


@functools.lru_cache(maxsize=None)
def shape_case(name, families, D, max_subs=4):
    """-> (codes, expected rows) of a shape of SHAPE_TABLE at `families` x 10 + 20 rows; every distance 0..D occurs"""
    key = (name, families, D, max_subs)
    assert key in SHAPE_STORES, key  # the CPU model checks exactly the stores the GPU tests use
    kind, L, n_frac = SHAPE_TABLE[name][:3]
    seed = RESEED.get(key, 1000 + 37 * list(SHAPE_TABLE).index(name) + families + D)
    codes = planted_store(seed, kind, L, families, n_frac, max_subs=max_subs)
    assert len(codes) == families * 10 + 20 and ((codes == 4).any() == (n_frac > 0) or kind == "aa")
    want = brute_pairs(codes, D)
    assert (want["dist"] == 0).sum() >= 1 and set(np.unique(want["dist"])) == set(range(D + 1)), (key, np.unique(want["dist"]))
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, want


@functools.lru_cache(maxsize=None)
def replaned_case():
    """-> (three pieces of nt330 rows, 1 000 + 20 + 500, expected rows of their concatenation at D = 5): the first N arrives in
    the last piece, so a store that takes them in this order keeps two planes for two appends and three after the third"""
    first = planted_store(71, "nt", 330, 100)
    last = planted_store(72, "nt", 330, 48, n_frac=0.01)
    assert len(first) == 1020 and len(last) == 500 and first.max() == 3 and (last == 4).any()
    pieces = (first[:1000], first[1000:], last)
    want = brute_pairs(np.concatenate(pieces), 5)
    assert (want["dist"] == 0).sum() >= 1 and set(np.unique(want["dist"])) == set(range(6))
    # pairs across the pieces' edges, or the re-planed store could lose the rows in front of the last piece unnoticed
    assert ((want["query"] < 1000) & (want["subject"] >= 1000) & (want["subject"] < 1020)).any()
    for p in pieces:
        p.setflags(write=False)
    want.setflags(write=False)
    return pieces, want


def join_spans(n, block, stride):
    """[(p0, m, S, R)] as join_pass (self_join.hip.h) cuts n positions with SMAFA_JOIN_BLOCK = block, SMAFA_JOIN_STRIDE = stride"""
    block = max(64, block // 64 * 64)
    spans = []
    for p0 in range(0, n, block * stride):
        m = min(n, p0 + block * stride) - p0
        S = (m + block - 1) // block
        spans.append((p0, m, S, (m + S - 1) // S))
    return spans


def join_scans(n, block, stride):
    """the scans of a join whose every block is taken at once: one per block, sum over spans of ceil(m / block)"""
    return sum(S for _, _, S, _ in join_spans(n, block, stride))

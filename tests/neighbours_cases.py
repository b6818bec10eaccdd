"""Expected answers and stores of the neighbours tests (tests/test_neighbours_model.py, tests/test_gpu_neighbours.py,
tests/neighbours_worker.py).

Nothing here comes from the code under test.  brute_neighbours compares every wanted row with every row of the store on the
code bytes — dist = the number of columns whose codes differ — keeps the others within the bound, orders them by (dist,
number) and cuts the list at k.  The store builders are those of tests/self_join_cases.py and tests/peaks_cases.py."""
import numpy as np

from self_join_cases import planted_store  # noqa: F401  (re-exported for the tests)


def brute_neighbours(codes, D, k=None, rows=None):
    """-> (offsets uint64[m + 1], neighbours uint32, dists uint32) of the rows `rows` (default: all, m = n) of the store"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, L = codes.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    slab = max(1, (32 << 20) // max(1, n * L))
    counts, nbs, ds = [], [], []
    for a in range(0, len(rows), slab):
        who = rows[a:a + slab]
        dist = (codes[who][:, None, :] != codes[None, :, :]).sum(axis=2)
        for r, i in enumerate(who):
            near = np.flatnonzero(dist[r] <= D)
            near = near[near != i]
            order = np.lexsort((near, dist[r][near]))
            near = near[order]
            if k is not None:
                near = near[:k]
            counts.append(len(near))
            nbs.append(near)
            ds.append(dist[r][near])
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.array(counts, dtype=np.uint64))
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, dtype=np.uint32)  # noqa: E731
    return offsets, cat(nbs), cat(ds)


def cut_lists(answer, k):
    """the first k entries of every list of a whole answer (k = None: the answer itself) — the definition of the cut"""
    if k is None:
        return answer
    offsets, nb, ds = answer
    deg = np.diff(offsets.astype(np.int64))
    rank = np.arange(len(nb)) - np.repeat(offsets[:-1].astype(np.int64), deg)
    keep = rank < k
    out = np.zeros(len(offsets), dtype=np.uint64)
    out[1:] = np.cumsum(np.minimum(deg, k).astype(np.uint64))
    return out, nb[keep], ds[keep]


def rows_of(answer, rows):
    """the lists of `rows` cut out of a whole answer, in the form brute_neighbours(..., rows=rows) gives"""
    offsets, nb, ds = answer
    counts = [int(offsets[i + 1] - offsets[i]) for i in rows]
    out = np.zeros(len(rows) + 1, dtype=np.uint64)
    out[1:] = np.cumsum(np.array(counts, dtype=np.uint64))
    pick = np.concatenate([np.arange(int(offsets[i]), int(offsets[i + 1])) for i in rows]) if len(rows) else np.zeros(0, dtype=np.int64)
    return out, nb[pick.astype(np.int64)], (None if ds is None else ds[pick.astype(np.int64)])


def same(got, want, dists=True):
    """exact equality of the three arrays, types included"""
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32
    assert got[0].tobytes() == want[0].tobytes(), "offsets"
    assert got[1].tobytes() == want[1].tobytes(), "neighbours"
    if dists:
        assert got[2].dtype == np.uint32 and got[2].tobytes() == want[2].tobytes(), "dists"
    else:
        assert got[2] is None


def planted_ends(n, L=60, seed=3):
    """n random nt rows, no two of them near each other, with rows 0 and n - 1 made neighbours at distance 2 and row n // 2 a
    copy of row 1: the first and the last row number both occur as row and as neighbour"""
    rng = np.random.default_rng(seed + n)
    codes = rng.integers(0, 4, size=(n, L)).astype(np.uint8)
    codes[n - 1] = codes[0]
    codes[n - 1, [5, 17]] = (codes[0, [5, 17]] + 1) % 4
    codes[n // 2] = codes[1]
    return np.ascontiguousarray(codes)


def middle_pair(n=1500, L=60, seed=9):
    """random rows with ONE pair, in the middle of the numbering: rows n // 2 - 3 and n // 2 + 4 at distance 1"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n, L)).astype(np.uint8)
    a, b = n // 2 - 3, n // 2 + 4
    codes[b] = codes[a]
    codes[b, 11] = (codes[a, 11] + 2) % 4
    return np.ascontiguousarray(codes), a, b


def no_pair(n=1200, L=60, seed=10):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.integers(0, 4, size=(n, L)).astype(np.uint8))


def tie_family(L=60, seed=12):
    """40 exact copies of one row and 40 variants of it with one substituted column each (distinct columns), shuffled: a copy
    has 39 neighbours at distance 0 and 40 at distance 1; a variant has 40 at distance 1 and 39 at distance 2"""
    rng = np.random.default_rng(seed)
    row = rng.integers(0, 4, size=L).astype(np.uint8)
    rows = [row] * 40
    for c in rng.choice(L, size=40, replace=False):
        v = row.copy()
        v[c] = (v[c] + 1) % 4
        rows.append(v)
    codes = np.array(rows, dtype=np.uint8)
    perm = rng.permutation(80)
    return np.ascontiguousarray(codes[perm]), (perm < 40)  # (codes, which rows are copies)


def short_store(n=300, seed=14):
    """seq_len 4, nt: at a bound >= 4 every row lists every other, and distance 4 = seq_len occurs"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n, 4)).astype(np.uint8)
    codes[1] = (codes[0] + 1) % 4  # distance 4 for certain
    return np.ascontiguousarray(codes)

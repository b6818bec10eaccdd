"""Expected answers and planted stores of the chimera tests (tests/test_chimera_model.py, tests/test_gpu_chimeras.py,
tests/test_chimera_abi.py, tests/chimera_worker.py).

Nothing here comes from the code under test: the pairs are self_join_cases.brute_pairs — brute force on the code bytes — the
counted weights a bincount over both columns of the pairs within the radius (as peaks_cases.peaks_from_pairs counts them), the
prefix and suffix lengths the first and the last True of `codes[q] != codes[p]`, and the best parents an np.maximum.at on
64-bit keys (length << 32 | 0xFFFFFFFF - parent: the longer side wins, ties go to the smaller number).

The definition (include/smafa_amd.h): p is an eligible parent of q iff p != q, both weights are non-zero, dist(q, p) <= D,
weight[p] > weight[q] and weight[p] >= F * weight[q]; rows that are equal column by column are never each other's parents."""
import collections
import functools
import struct

import numpy as np

from smafa_amd import synth
from self_join_cases import brute_pairs

NONE = 0xFFFFFFFF
Expected = collections.namedtuple("Expected", "flags left_parent left_len right_parent right_len weights n_chimeras")
BREAKPOINTS = (1, 31, 32, 33, 63, 64, 65)  # and L - 1: plane-word edges, and the first and the last column

# The hand-worked store of tests/test_chimera_model.py: eight rows of six columns.  A = 000000 three times (rows 0, 1, 2), B =
# 111111 twice (rows 3, 4), and
#   row 5 = 000111  A's head on B's tail, breakpoint 3
#   row 6 = 002111  the same with column 2 moved: one column short
#   row 7 = 222222  shares no column with anybody: from D = 6 on A is its parent of last resort, at length 0
HAND = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1],
                 [0, 0, 0, 1, 1, 1], [0, 0, 2, 1, 1, 1], [2, 2, 2, 2, 2, 2]], dtype=np.uint8)


def counted_weights(n, pairs, radius):
    near = pairs["dist"].astype(np.int64) <= int(radius)
    q, s = pairs["query"].astype(np.int64)[near], pairs["subject"].astype(np.int64)[near]
    return (1 + np.bincount(q, minlength=n) + np.bincount(s, minlength=n)).astype(np.uint32)


def chimeras_from_pairs(codes, pairs, radius, fold, weights_in=None, slab=1 << 16):
    """pairs (HIT_DTYPE, each unordered pair once, all within the bound) -> Expected"""
    n, L = codes.shape
    weights = counted_weights(n, pairs, radius) if weights_in is None else np.asarray(weights_in, dtype=np.uint32).copy()
    assert weights.shape == (n,)
    w = weights.astype(np.uint64)
    left, right = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    pq, ps = pairs["query"].astype(np.int64), pairs["subject"].astype(np.int64)
    differ = pairs["dist"] > 0
    for cand, par in ((pq, ps), (ps, pq)):  # both orientations: either row may be the candidate
        ok = differ & (w[cand] != 0) & (w[par] != 0) & (w[par] > w[cand]) & (w[par] >= np.uint64(fold) * w[cand])
        q_all, p_all = cand[ok], par[ok]
        for at in range(0, len(q_all), slab):
            q, p = q_all[at: at + slab], p_all[at: at + slab]
            diff = codes[q] != codes[p]
            assert diff.any(axis=1).all()
            pre = diff.argmax(axis=1).astype(np.uint64)               # d_0
            suf = diff[:, ::-1].argmax(axis=1).astype(np.uint64)      # L - 1 - d_{m-1}
            low = np.uint64(NONE) - p.astype(np.uint64)
            np.maximum.at(left, q, (pre << np.uint64(32)) | low)
            np.maximum.at(right, q, (suf << np.uint64(32)) | low)
    has = left != 0
    assert (has == (right != 0)).all()
    mask = np.uint64(NONE)
    left_len, right_len = (left >> np.uint64(32)).astype(np.uint32), (right >> np.uint64(32)).astype(np.uint32)
    left_parent = np.where(has, mask - (left & mask), mask).astype(np.uint32)
    right_parent = np.where(has, mask - (right & mask), mask).astype(np.uint32)
    flags = (has & (left_len.astype(np.int64) + right_len.astype(np.int64) >= L)).astype(np.uint32)
    return Expected(flags, left_parent, left_len, right_parent, right_len, weights, int(flags.sum()))


def brute_chimeras(codes, D, radius, fold, weights_in=None):
    """-> Expected(flags, left_parent, left_len, right_parent, right_len, weights, n_chimeras) of a store at bound D, radius r <=
    D (None: r = D) and fold F >= 1; weights_in: uint32[n] used in place of the counted weights"""
    radius = D if radius is None else radius
    assert radius <= D and fold >= 1
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if len(codes) == 0:
        empty = np.zeros(0, dtype=np.uint32)
        return Expected(empty, empty, empty, empty, empty, empty, 0)
    return chimeras_from_pairs(codes, brute_pairs(codes, D), radius, fold, weights_in)


def rebuilt(codes, answer, q, b):
    """row q as left_parent[:b] + right_parent[b:]"""
    return np.concatenate([codes[answer.left_parent[q]][:b], codes[answer.right_parent[q]][b:]])


def packed_perm(path, L):
    """perm[j] = source column of packed column j, from a packed store file (SubjectStore.save; host/packed.cpp)"""
    raw = open(path, "rb").read()
    off_perm = struct.unpack_from("<Q", raw, 8 + 40)[0]
    return np.frombuffer(raw, dtype="<u4", count=L, offset=off_perm)


# the planted classes: role[i] of chimera_store
FILLER, PARENT, BIMERA, NEAR_MISS, LOW_FOLD, TIE, FAR = range(7)
ROLE_NAMES = ("filler", "parent", "bimera", "near miss", "low fold", "tie", "far parent")


def _substituted(rng, row, cols, letters, avoid=()):
    """row with every column of `cols` moved to another letter (and away from the rows of `avoid` there)"""
    out = row.copy()
    for c in cols:
        taken = {int(row[c])} | {int(a[c]) for a in avoid}
        out[c] = rng.choice([v for v in range(letters) if v not in taken])
    return out


def chimera_store(seed, kind, L, filler=100):
    """A planted store -> (codes, role, info).  kind: "nt", "ntn" (N in 1 % of the filler's cells and one shared column of a
    family) or "aa".  Parents are heavy (20 - 40 copies), the rows made from them light (1 - 3 copies):
      P0 | P1   differ in columns 0, L - 1 and two between: bimeras P0[:b] + P1[b:] at every b of BREAKPOINTS and L - 1 that
                fits (BIMERA, flagged from D = 3 and F <= 3 on: each is within 3 of both parents), and one near miss — the
                bimera at the middle with column b - 1 moved away from both parents, left_len + right_len == L - 1 (NEAR_MISS);
      P4        P0 with one column behind the first differing column of (P0, P1) moved away from both: for the bimera at b = 1,
                whose first difference from P0 lies in front of it, P4 shares exactly P0's prefix — two equally good left
                parents, the tie goes to the smaller number (TIE: that bimera's copies);
      P2 | P3   6 copies each, four columns apart: their bimera has 4 copies — its parents are heavier, but not twice as heavy
                (LOW_FOLD: flagged at F = 1 only);
      P5 | P6   eight columns apart, four on either side of the middle: their bimera at the middle is 4 from both, not flagged at
                D = 3 and flagged at D >= 4 (FAR);
      filler    random rows, a few of them twice.
    info: {"b": breakpoint of every planted row (0: none), "parents": {name: one row number of that parent}}."""
    assert L >= 9
    rng = np.random.default_rng(seed)
    lc = synth.letter_codes(1 if kind == "aa" else 0)
    A = len(lc)
    mid = L // 2
    rows, role, bps, with_n, first = [], [], [], [], {}

    def add(row, copies, r, b=0, name=None, shared_n=False):
        if name:
            first[name] = len(rows)
        for _ in range(copies):
            rows.append(row)
            role.append(r)
            bps.append(b)
            with_n.append(shared_n)

    def pair(cols):
        a = rng.integers(0, A, size=L)
        return a, _substituted(rng, a, cols, A)

    # P0 | P1: columns 0, c1, c2, L - 1 with a free column between c1 and c2
    c1 = int(rng.integers(2, L - 4))
    c2 = int(rng.integers(c1 + 2, L - 2))
    p0, p1 = pair([0, c1, c2, L - 1])
    p4 = _substituted(rng, p0, [c2], A, avoid=(p1,))  # within 3 of the bimera at b = 1, and P0's prefix c1 with it
    add(p0, 40, PARENT, name="P0")
    add(p1, 36, PARENT, name="P1")
    add(p4, 22, PARENT, name="P4")
    made = set()
    for b in sorted({b for b in BREAKPOINTS + (L - 1,) if 1 <= b <= L - 1}):
        # breakpoints with no differing column between them make the same row: 1 - 3 copies of it once, one more per repeat (at
        # most 3 + 7 = 10 <= 36 / 3: light enough for F = 3)
        row = np.concatenate([p0[:b], p1[b:]])
        add(row, 1 if row.tobytes() in made else int(rng.integers(1, 4)), TIE if b == 1 else BIMERA, b)
        made.add(row.tobytes())
    junction = c1 + 2  # c1 < junction <= c2: two of the four columns on either side, and column junction - 1 is free
    near = _substituted(rng, np.concatenate([p0[:junction], p1[junction:]]), [junction - 1], A, avoid=(p0, p1))
    add(near, 1, NEAR_MISS, junction)
    # (column 1 stays alike inside this family: "ntn" puts its shared N there)
    p2, p3 = pair([0, *sorted(rng.choice(np.arange(2, L - 2), size=2, replace=False).tolist()), L - 1])
    add(p2, 6, PARENT, name="P2", shared_n=True)
    add(p3, 6, PARENT, name="P3", shared_n=True)
    add(np.concatenate([p2[:mid], p3[mid:]]), 4, LOW_FOLD, mid, shared_n=True)
    lo = rng.choice(np.arange(0, mid), size=4, replace=False).tolist()
    hi = rng.choice(np.arange(mid, L), size=4, replace=False).tolist()
    p5, p6 = pair(sorted(lo + hi))
    add(p5, 24, PARENT, name="P5")
    add(p6, 21, PARENT, name="P6")
    add(np.concatenate([p5[:mid], p6[mid:]]), 1, FAR, mid)
    codes = lc[np.array(rows, dtype=np.int64)]
    if kind == "ntn":
        codes[np.array(with_n), 1] = 4
    fill = lc[rng.integers(0, A, size=(filler, L))]
    if kind == "ntn":
        fill[rng.random(size=fill.shape) < 0.01] = 4
    fill = np.concatenate([fill, fill[: max(1, filler // 20)]])
    codes = np.concatenate([codes, fill])
    role = np.array(role + [FILLER] * len(fill))
    bps = np.array(bps + [0] * len(fill))
    order = rng.permutation(len(codes))
    new_number = np.argsort(order)
    codes, role, bps = np.ascontiguousarray(codes[order], dtype=np.uint8), role[order], bps[order]
    codes.setflags(write=False)
    return codes, role, {"b": bps, "parents": {name: int(new_number[k]) for name, k in first.items()}}


# every planted store of the GPU tests: key -> (seed, kind, L, filler).  nt60 / ntn60 / aa60: 2, 3 and 5 planes; the lengths
# around the plane-word edges; one wide shape of self_join_cases.SHAPE_TABLE (aa250); nt60big: more than one span at
# SMAFA_JOIN_BLOCK=192 SMAFA_JOIN_STRIDE=3 (576 positions per span).  tests/test_chimera_model.py holds each to its classes; a
# store that misses one gets another seed HERE.
STORES = {
    "nt60": (1, "nt", 60, 100), "ntn60": (2, "ntn", 60, 100), "aa60": (3, "aa", 60, 100),
    "nt9": (4, "nt", 9, 100), "nt31": (5, "nt", 31, 100), "nt32": (6, "nt", 32, 100), "nt33": (7, "nt", 33, 100),
    "nt64": (8, "nt", 64, 100), "nt65": (9, "nt", 65, 100), "nt130": (10, "nt", 130, 100), "aa250": (11, "aa", 250, 100),
    "nt60big": (12, "nt", 60, 1500),
}


@functools.lru_cache(maxsize=None)
def planted(key):
    seed, kind, L, filler = STORES[key]
    return chimera_store(seed, kind, L, filler)


@functools.lru_cache(maxsize=None)
def expected(key, D, radius, fold):
    """brute_chimeras of a planted store with counted weights, computed once and shared"""
    return brute_chimeras(planted(key)[0], D, radius, fold)


def check_classes(codes, role, info, L):
    """The planted store yields at least one row of every class with the intended verdict, on the brute-force answer: a store
    that misses one gets another seed, not a weaker test."""
    at = {f: brute_chimeras(codes, 3, 0, f) for f in (1, 2, 3)}
    wide = brute_chimeras(codes, 6, 0, 2)
    a = at[2]
    n = len(codes)
    same = lambda i, j: (codes[i] == codes[j]).all()  # noqa: E731
    P = info["parents"]
    # bimeras: flagged at D = 3 for every F, with P0's head and P1's tail, and rebuilt at every breakpoint of the interval
    bim = np.flatnonzero((role == BIMERA) | (role == TIE))
    assert len(bim) >= 3
    for f in (1, 2, 3):
        assert at[f].flags[bim].all(), (f, at[f].weights[bim])
    for q in bim:
        # (P4, or a bimera that several breakpoints made heavy, may be as good a parent: what is planted is P0's head, P1's tail)
        b = int(info["b"][q])
        assert (codes[a.left_parent[q]][:b] == codes[P["P0"]][:b]).all() and (codes[a.right_parent[q]][b:] == codes[P["P1"]][b:]).all()
        assert a.left_parent[q] != a.right_parent[q] and L - a.right_len[q] <= b <= a.left_len[q]
        for b in range(L - int(a.right_len[q]), int(a.left_len[q]) + 1):
            assert (rebuilt(codes, a, q, b) == codes[q]).all()
    assert {int(b) for b in info["b"][bim]} == {b for b in BREAKPOINTS + (L - 1,) if 1 <= b <= L - 1}
    # the near miss: parents found, one column short
    near = np.flatnonzero(role == NEAR_MISS)
    assert len(near) == 1 and not a.flags[near[0]] and int(a.left_len[near[0]]) + int(a.right_len[near[0]]) == L - 1
    # (P4, or a bimera that several breakpoints made heavy, may be as good a parent as P0 or P1: the lengths are what is planted)
    assert a.left_len[near[0]] == info["b"][near[0]] - 1 and a.right_len[near[0]] == L - info["b"][near[0]]
    assert a.left_parent[near[0]] != NONE and a.right_parent[near[0]] != NONE
    # heavier, but not twice as heavy
    low = np.flatnonzero(role == LOW_FOLD)
    assert len(low) == 4 and at[1].flags[low].all() and not at[2].flags[low].any() and not at[3].flags[low].any()
    assert (at[2].left_parent[low] == NONE).all() and (at[2].left_len[low] == 0).all()
    # two equally good left parents: the smallest copies of P0 and of P4 share the best prefix, the smaller number is chosen
    tie = np.flatnonzero(role == TIE)
    assert len(tie) >= 1
    q = tie[0]
    firsts = [min(i for i in range(n) if same(i, P[name])) for name in ("P0", "P4")]
    pre = [int((codes[q] != codes[p]).argmax()) for p in firsts]
    assert pre[0] == pre[1] == a.left_len[q] and a.left_parent[q] == min(firsts) and not same(firsts[0], firsts[1])
    # a parent farther than the bound
    far = np.flatnonzero(role == FAR)
    assert len(far) == 1 and not a.flags[far[0]] and wide.flags[far[0]]
    assert same(wide.left_parent[far[0]], P["P5"]) and same(wide.right_parent[far[0]], P["P6"])
    # parents and filler are no chimeras
    assert not a.flags[(role == PARENT) | (role == FILLER)].any()
    return at, wide

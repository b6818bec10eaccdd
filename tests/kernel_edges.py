"""Edge inputs for the kernel census (tests/test_gpu_kernel_census.py).  Test helpers only.

A store is built in two appends: a random first one, which fixes the column layout (host/layout.cpp: columns re-coded one by
one and ordered by how evenly their letters split, so packed column j is source column perm[j]), and a second one that holds
the planted subjects.  Stores have n = 1 or 255 (mod 256) rows, so the last wave tile and the last 1024-subject workgroup
are partial.  A nucleotide store of three planes receives its first N only in the second append.

Queries of a case:
- a homopolymer of every letter in use (N included on nucleotide stores of two planes): far from every subject, so a padding
  slot that passed for a subject would show up as a row;
- for the bound E of the launch, planted pairs at distance exactly E and E + 1, the mismatches placed four ways in PACKED
  columns: (i) all in columns 0-31, which level 1 sees, (ii) all past column 31, (iii) spread over every word, (iv) including
  column L - 1 when L % 32 != 0; the substituted letters cycle over every unordered pair of letters in use, so pairs that
  differ in one plane and pairs that differ in several both occur;
- k modes: queries with k - 1, k and k + 1 subjects tied at distance E (and one more at E + 1);
- fillers: planted pairs at distances spread over [0, spread] (the near-hit ladder then finishes some queries at every step).

Dense stores (Planter(..., dense_bounds=...)) keep all of the above and add a FAMILY: copies of one base row, at least 40 % of
the store, in both appends.  The first append holds only exact copies (the layout is not known before it is fixed); the
second one also holds members 1 .. E + 1 substitutions away for every bound E of the store, their columns placed the four
ways above and their letters cycling over every letter difference.  The dense queries are the base and the base with 1-2
substitutions: 32 of them in every 64-query chunk, then the planted queries and the homopolymers.  So every
workgroup and chunk appends far more rows than its LDS stage parks, and the k modes see ties far past k.
"""
from __future__ import annotations

import itertools

import numpy as np

NT_N = 4
KINDS = {"nt2": (0, 2, 3), "nt3": (0, 3, 3), "aa": (1, 5, 5)}  # kind -> (alphabet, store planes, query planes)
PLACEMENTS = ("low", "high", "spread", "last")


def store_letters(kind):
    return {"nt2": 4, "nt3": 5, "aa": 20}[kind]


def query_letters(kind):
    return {"nt2": 5, "nt3": 5, "aa": 20}[kind]


def packed_columns(alphabet, L, first):
    """perm[j] = source column of packed column j (mirror of compute_layout, host/layout.cpp)"""
    n = len(first)
    S = min(n, 4096)
    rows = first[[k * n // S for k in range(S)]]
    aa = alphabet == 1
    score = []
    for c in range(L):
        cc = np.bincount(rows[:, c] & 31, minlength=32).astype(np.int64)

        def balance(t0, t1):
            a = float(t0 + t1)
            return 2.0 * float(t0) * float(t1) / (a * a) if a > 0 else 0.0

        if not aa:
            pair = ((2, 3), (1, 3), (1, 2))
            sc = []
            for p in pair:
                t1 = int(cc[p[0]] + cc[p[1]])
                t0 = int(cc[0] + cc[1] + cc[2] + cc[3]) - t1
                sc.append(balance(t0, t1))
            top = max(sc)
            best = 0 if not sc[0] < 0.95 * top else (1 if sc[1] >= sc[2] else 2)
            score.append(sc[best])
        else:
            idx = sorted(range(28), key=lambda v: -cc[v])  # (stable, as std::stable_sort)
            tot, num = [0, 0], [0, 0]
            for v in idx:
                side = 0 if tot[0] <= tot[1] else 1
                if num[side] == 16:
                    side ^= 1
                tot[side] += int(cc[v])
                num[side] += 1
            score.append(balance(tot[0], tot[1]))
    return sorted(range(L), key=lambda c: -score[c])


class Planter:
    """rows of one store and the queries planted against it"""

    def __init__(self, kind, L, n, seed, dense_bounds=None):
        self.kind, self.L, self.n = kind, L, n
        self.alphabet, self.planes, _ = KINDS[kind]
        self.rng = np.random.default_rng(seed)
        self.sl, self.ql = store_letters(kind), query_letters(kind)
        first_letters = 4 if kind == "nt3" else self.sl  # the three-plane store: its first N arrives with the second append
        self.first = self.rng.integers(0, first_letters, size=(1024, L), dtype=np.uint8)
        self.dense, self.sealed = dense_bounds is not None, False
        if self.dense:
            self.base = self.rng.integers(0, first_letters, size=L, dtype=np.uint8)  # (no N: it is in the first append too)
            self.first[self.rng.choice(1024, size=620, replace=False)] = self.base
            self.member_d = sorted(set(range(1, 8)) | {d for E in dense_bounds for d in (E, E + 1)})
            self.dense_pool = [self.base]
            while len(self.dense_pool) < 128:  # the base with 1-2 substitutions
                q = self.base.copy()
                for c in self.rng.choice(L, size=min(L, 1 + len(self.dense_pool) % 2), replace=False):
                    q[c] = (int(q[c]) + 1 + int(self.rng.integers(0, self.ql - 1))) % self.ql
                self.dense_pool.append(q)
        self.perm = packed_columns(self.alphabet, L, self.first)
        self.second = self.rng.integers(0, self.sl, size=(n - 1024, L), dtype=np.uint8)
        self.free = list(self.rng.permutation(n - 1024))
        self.free.remove(n - 1025)
        self.free.insert(0, n - 1025)  # the store's last subject is a planted one
        self.pairs = itertools.cycle(list(itertools.combinations(range(self.ql), 2)))
        self.sets = {}

    def subjects(self):
        return np.concatenate([self.first, self.second])

    def _place(self, row):
        assert self.free, "no room left for planted subjects"
        assert not self.sealed, "planted after the family filled the store"
        self.second[self.free.pop(0)] = row

    def _pair(self):
        a, b = next(self.pairs)
        if self.rng.integers(0, 2):
            a, b = b, a
        if a >= self.sl:  # a letter the store cannot hold (N on two planes) goes to the query side
            a, b = b, a
        return a, b

    def columns(self, d, placement):
        L, perm, rng = self.L, self.perm, self.rng
        W = (L + 31) // 32
        if placement == "low":
            pool = range(min(32, L))
            if d > len(pool):
                return None
            packed = rng.choice(pool, size=d, replace=False)
        elif placement == "high":
            pool = range(32, L)
            if d > len(pool) or (d == 0 and L <= 32):
                return None
            packed = rng.choice(pool, size=d, replace=False) if d else []
        elif placement == "spread":
            if d > L:
                return None
            words = [list(rng.permutation(range(32 * w, min(L, 32 * w + 32)))) for w in range(W)]
            packed, w = [], 0
            while len(packed) < d:
                if words[w % W]:
                    packed.append(words[w % W].pop())
                w += 1
        else:
            if L % 32 == 0 or d == 0 or d > L:
                return None
            packed = [L - 1] + list(rng.choice(range(L - 1), size=d - 1, replace=False))
        return [perm[int(j)] for j in packed]

    def pair(self, d, placement):
        """a planted subject and a query at distance exactly d, or None where the placement cannot hold d mismatches"""
        cols = self.columns(d, placement)
        if cols is None:
            return None
        base = self.rng.integers(0, self.sl, size=self.L, dtype=np.uint8)
        s, q = base.copy(), base.copy()
        for c in cols:
            s[c], q[c] = self._pair()
        self._place(s)
        return q

    def tie(self, k_subjects, E):
        """a query with k_subjects subjects at distance exactly E and one at E + 1"""
        q = self.rng.integers(0, self.sl, size=self.L, dtype=np.uint8)
        for d in [E] * k_subjects + [E + 1]:
            s = q.copy()
            for c in self.rng.choice(self.L, size=min(d, self.L), replace=False):
                s[c] = (int(q[c]) + 1 + int(self.rng.integers(0, self.sl - 1))) % self.sl
            self._place(s)
        return q

    def plant(self, E, k=0, spread=0):
        """plant the query set of bound E (once per store and (E, k, spread)); call before subjects() is pushed"""
        key = (E, k, spread)
        if key not in self.sets:
            qs = [q for d in (E, E + 1) for p in PLACEMENTS for q in [self.pair(d, p)] if q is not None]
            if k:
                qs += [self.tie(t, E) for t in (k - 1, k, k + 1)]
            for d in range(0, spread + 1, 2):  # every other distance: enough of them that each ladder step finishes some
                qs.append(self.pair(min(d, self.L), "spread"))
            self.sets[key] = np.array(qs, dtype=np.uint8)
        return self.sets[key]

    def seal(self):
        """dense stores: the family's rows in the second append, in every free row but a fifth (call after every plant())"""
        if not self.dense or self.sealed:
            return
        keep = len(self.free) // 5
        deltas = itertools.cycle(range(1, self.sl))
        dists, places = itertools.cycle(self.member_d), itertools.cycle(PLACEMENTS)
        for i, slot in enumerate(self.free[: len(self.free) - keep]):
            row = self.base.copy()
            if i % 2:  # every other one a member 1 .. E + 1 substitutions away; the rest exact copies
                d = min(next(dists), self.L)
                cols = None
                while cols is None:
                    cols = self.columns(d, next(places))
                for c in cols:
                    row[c] = (int(row[c]) + next(deltas)) % self.sl
            self.second[slot] = row
        self.free = self.free[len(self.free) - keep:]
        self.sealed = True

    def dense_queries(self, E, nq, k=0, spread=0):
        """dense stores: nq queries and the mask of the dense ones (the base and the base with 1-2 substitutions) — 32 of every
        64-query chunk (all of a chunk of fewer than 32), then the planted queries and the homopolymers, repeated as often as
        the chunks need; a single query is the base.
        (The near-hit ladder steps on only while 16 or more queries are open: with the dense queries finished by its first
        step, the planted ones must be that many for the later steps — and their instantiations — to run, as on a sparse store.)"""
        assert self.dense
        if nq == 1:
            return np.ascontiguousarray(self.base[None, :]), np.ones(1, dtype=bool)
        homo = np.repeat(np.arange(self.ql, dtype=np.uint8)[:, None], self.L, axis=1)
        extra = itertools.cycle(list(np.concatenate([self.plant(E, k, spread), homo])))
        pool = itertools.cycle(self.dense_pool)
        qs, mask = [], []
        for lo in range(0, nq, 64):
            size = min(64, nq - lo)
            n_dense = 32 if size >= 32 else size
            qs += [next(pool) for _ in range(n_dense)] + [next(extra) for _ in range(size - n_dense)]
            mask += [True] * n_dense + [False] * (size - n_dense)
        return np.ascontiguousarray(np.array(qs, dtype=np.uint8)), np.array(mask)

    def queries(self, E, nq, k=0, spread=0):
        """nq queries for a launch of bound E: the planted ones first, then homopolymers, then fillers drawn from the store"""
        if self.dense:
            return self.dense_queries(E, nq, k, spread)[0]
        if nq == 1:
            return self.plant(E, k, spread)[:1]
        homo = np.repeat(np.arange(self.ql, dtype=np.uint8)[:, None], self.L, axis=1)
        qs = np.concatenate([self.plant(E, k, spread), homo])
        if len(qs) < nq:
            subj = self.subjects()
            rng = np.random.default_rng(nq * 1000 + E)
            fill = subj[rng.integers(0, len(subj), size=nq - len(qs))].copy()
            for r in fill:  # 0 .. E + 1 substitutions
                for c in rng.choice(self.L, size=int(rng.integers(0, min(E + 2, self.L) + 1)), replace=False):
                    r[c] = rng.integers(0, self.ql)
            qs = np.concatenate([qs, fill])
        assert len(qs) >= nq, (len(qs), nq)
        return np.ascontiguousarray(qs[:nq])

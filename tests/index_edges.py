"""Edge inputs for the block index (smafa_amd/csrc/index.hip.h), planted against the index's own geometry.  Test helpers only.

A store indexed with build_index(D) has B = D + 1 blocks, block b being the PACKED columns [b*L // B, (b+1)*L // B)
(engine.hip index_build: col_begin).  A pair within the bound is found through a probed block it is clean on (no mismatch
in the block) and reported by the first such block of the probe order.  The pairs planted here, by class:

  only_clean(c, v)  distance exactly D, one mismatch in every block but c — at the block's first column (v = 0) or its last
                    (v = 1).  At bound D every block is probed: the pair must be found through block c, wherever c stands
                    in the probe order.
  none_clean        distance D + 1, one mismatch in every block: absent.
  over(c)           distance D + 1, block c clean, two mismatches in one other block and one in each of the rest: a
                    candidate of block c that the full comparison rejects.
  shared(d)         d in 0 .. D - 1, all d mismatches inside one block: clean on at least two probed blocks, reported once.
  rotating(D', s)   D' in 0 .. D - 1, s in 0 .. B - 1: distance exactly D', one mismatch in each of the blocks s, s + 1, ..,
                    s + D' - 1 (mod B).  At bound D' only D' + 1 of the B blocks are probed, chosen by their run statistics:
                    whichever they are, some of these pairs are clean on exactly one of them.
  straddle(j)       where a block holds packed columns 32k - 1 and 32k (k = 1, 2, 3): a single mismatch at column j = 32k - 1,
                    and one at j = 32k — the block's key and its clear test take bits of two words (lo / hi masks).  (The
                    only_clean pairs of that block are planted with every other block's.)
A class that a shape cannot hold is left out: over() needs a second block of two columns, shared(d) a block of d columns.

The store is kernel_edges.Planter's: two appends, the first one fixing the column layout (perm: packed column -> source
column), a three-plane nucleotide store receiving its first N only with the second.  The second append of the smaller store
(n = 1025) is ONE row and a shape with 32 blocks plants over a thousand pairs, so the planted subjects are HOSTS shared by
many queries: `hosts` rows placed with Planter._place (the first one the store's last row), each planted pair a host and a
query that differs from it in the planted columns.  The substituted letters cycle over the unordered letter pairs as
Planter._pair does — the next pair of the cycle that holds the host's letter gives the query's — so pairs that differ in one
plane and in several both occur, and on a two-plane store N is always on the query side (no host holds one).
"""
from __future__ import annotations

import numpy as np

from kernel_edges import Planter

# (kind, L, D): the shapes of tests/test_gpu_index_edges.py
SHAPES = [(kind, L, D) for kind in ("nt2", "nt3", "aa") for L, D in ((31, 5), (60, 5), (60, 6), (90, 7), (120, 5), (128, 3))]
SHAPES += [("aa", 120, 31), ("nt3", 120, 31), ("aa", 20, 19)]
SIZES = (1279, 1025)  # a partial last tile of 255 rows and of one
MIN_QUERIES = 65      # the index answers batches of more than 64 queries


def block_columns(L, B):
    """[(c0, c1)] packed columns of every block (engine.hip index_build: col_begin[b] = b * L / blocks)"""
    return [(b * L // B, (b + 1) * L // B) for b in range(B)]


class IndexPlanter(Planter):
    """the rows of one store and every pair planted against the B = D + 1 blocks of its index"""

    def __init__(self, kind, L, n, D, seed, hosts=48):
        super().__init__(kind, L, n, seed)
        self.D, self.B = D, D + 1
        self.blocks = block_columns(L, self.B)
        assert all(c1 > c0 for c0, c1 in self.blocks)
        self.host_rows = []  # subject numbers of the hosts
        for _ in range(min(hosts, len(self.free))):
            slot = self.free[0]
            self._place(self.rng.integers(0, self.sl, size=L, dtype=np.uint8))
            self.host_rows.append(1024 + int(slot))
        self.planted = []  # dicts: cls, args, subject, query (position in self.planted), cols (packed columns that differ)
        self._plant_all()
        fill = max(0, MIN_QUERIES - len(self.planted))
        homo = np.repeat(np.arange(self.ql, dtype=np.uint8)[:, None], L, axis=1)
        subj = self.subjects()
        noise = subj[self.rng.integers(0, n, size=fill)].copy()
        for r in noise:  # 0 .. D + 1 substitutions
            for c in self.rng.choice(L, size=int(self.rng.integers(0, min(D + 2, L) + 1)), replace=False):
                r[c] = self.rng.integers(0, self.ql)
        self.query_rows = np.ascontiguousarray(np.concatenate([np.array([p["q"] for p in self.planted], dtype=np.uint8).reshape(-1, L),
                                                               homo, noise]))

    def queries(self):
        """the planted queries (query i belongs to self.planted[i]), then a homopolymer of every letter, then noisy copies"""
        return self.query_rows

    def _letter(self, a):
        """the query's letter against the host's letter a: from the next pair of the cycle that holds a"""
        while True:
            x, y = next(self.pairs)
            if a in (x, y):
                return y if a == x else x

    def _plant(self, cls, args, packed):
        packed = [int(j) for j in packed]
        assert len(set(packed)) == len(packed)
        subject = self.host_rows[len(self.planted) % len(self.host_rows)]
        q = self.second[subject - 1024].copy()
        for j in packed:
            c = self.perm[j]
            q[c] = self._letter(int(q[c]))
        self.planted.append(dict(cls=cls, args=args, subject=subject, query=len(self.planted), cols=sorted(packed), q=q))

    def _one_in(self, b, where):
        c0, c1 = self.blocks[b]
        return c0 if where == 0 else c1 - 1 if where == 1 else int(self.rng.integers(c0, c1))

    def _plant_all(self):
        D, B, blocks = self.D, self.B, self.blocks
        width = [c1 - c0 for c0, c1 in blocks]
        for c in range(B):
            for v in (0, 1):
                self._plant("only_clean", (c, v), [self._one_in(b, v) for b in range(B) if b != c])
        self._plant("none_clean", (), [self._one_in(b, 2) for b in range(B)])
        for c in range(B):
            two = next((b % B for b in range(c + 1, c + B) if width[b % B] >= 2), None)
            if two is None:
                continue
            cols = [self._one_in(b, 2) for b in range(B) if b not in (c, two)]
            cols += [int(j) for j in blocks[two][0] + self.rng.choice(width[two], size=2, replace=False)]
            self._plant("over", (c,), cols)
        for d in range(D):
            b = d % B if width[d % B] >= d else int(np.argmax(width))
            if width[b] < d:
                continue
            self._plant("shared", (d,), [int(j) for j in blocks[b][0] + self.rng.choice(width[b], size=d, replace=False)])
        for Dp in range(D):
            for s in range(B):
                self._plant("rotating", (Dp, s), [self._one_in((s + t) % B, (s + t) % 3) for t in range(Dp)])
        for edge in (32, 64, 96):
            if any(c0 < edge < c1 for c0, c1 in blocks):
                self._plant("straddle", (edge - 1,), [edge - 1])
                self._plant("straddle", (edge,), [edge])

    def straddling_blocks(self):
        return [b for b, (c0, c1) in enumerate(self.blocks) if any(c0 < e < c1 for e in (32, 64, 96))]


def observed(p, pair):
    """(distance, mismatches per block) of a planted pair, recomputed from the code bytes and perm alone"""
    s, q = p.subjects()[pair["subject"]], p.queries()[pair["query"]]
    dist = int((s != q).sum())
    per_block = [sum(int(s[p.perm[j]] != q[p.perm[j]]) for j in range(c0, c1)) for c0, c1 in p.blocks]
    return dist, per_block


def small_store(kind, L, n, D, seed, nq=80):
    """a store of one append (fewer than 256 rows or one row past a tile: dir_bits 8) and random queries — no layout is known
    beforehand, so nothing is planted: copies of the rows with 0 .. D + 1 substitutions, and random rows"""
    rng = np.random.default_rng(seed)
    sl = {"nt2": 4, "nt3": 5, "aa": 20}[kind]
    ql = {"nt2": 5, "nt3": 5, "aa": 20}[kind]
    s = rng.integers(0, sl, size=(n, L), dtype=np.uint8)
    if kind == "nt3":
        s[0, L // 2] = 4  # (a store of one row still has its N)
    q = s[rng.integers(0, n, size=nq)].copy()
    for r in q[: nq - 8]:
        for c in rng.choice(L, size=int(rng.integers(0, min(D + 2, L) + 1)), replace=False):
            r[c] = rng.integers(0, ql)
    q[nq - 4:] = rng.integers(0, ql, size=(4, L), dtype=np.uint8)
    return s, np.ascontiguousarray(q)

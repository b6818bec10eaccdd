"""Stores and planted queries for the sampled counting path of the k-th distance modes (scan_host.hip.h scan_kth with
kth_sample_tiles != 0: kth_seed_kernel counting a sample, kth_from_counts_kernel, one counting-and-appending pass over the rest,
the sample's tiles again, filter_rows_kernel).  Used by tests/test_kth_sample_model.py (CPU: the planted structure is what
this text says, by brute force) and tests/test_gpu_kth_sample.py (GPU: rows == the oracle's).  Test helpers only.

Stores are unsorted (SMAFA_SORT=0, SMAFA_RESORT=0): position = subject number, and the sample is subjects [0, S), S = 256 x
sample_tiles.  n = 1 (mod 256): the last wave tile holds one row.  A three-plane nucleotide store (nt3) is pushed in two parts,
an N-free first one of 1024 rows and the rest, so the store that is sampled is the re-planed one.

Every planted query has a base row of its own; its planted subjects are the base with exactly d substituted columns, each set
to a different letter, at positions nothing else is planted at.  E = 3, D = L // 2 (a bound level 1 of the prefilter does not
prune at: level1_prunes), k = the k the case is built for:
  a     k - 1 subjects at E inside the sample, two at E outside it, one at E + 1 outside      -> k-th distance E, k + 1 rows
  b     k at E inside, k at E outside, two at E - 1 outside                                   -> E, 2k + 2 rows
  c     ties at E at subjects 0, S - 1, S and n - 1 (the lone row of the last tile)           -> k = 3: E, all four rows
  d     k - 2 subjects at D, three at D + 1, on both sides of S     -> under the bound D: k - 2 rows; without: D + 1, k + 1 rows
  e     k subjects at D, on both sides of S                         -> D, k rows, bound or not
  twin  (of e) k - 1 subjects at D, two at D + 1                    -> under the bound D: k - 1 rows; without: D + 1, k + 1 rows
  f     k + 3 exact copies of the base in the first, the middle and the last full tile (the last tile's only row is c's)  -> 0
  g     a homopolymer of a letter no subject holds (N on nt2, code 27 on aa): at distance L from every subject, n rows, and
        only where there is no bound.  Left out on nt3, whose store holds N: a filler takes its place there.
  h     k subjects at E + 1 inside the sample, k at E outside it: the true k-th distance (E) is BELOW the sample's (E + 1)
Classes a, b and h come twice: once at the head of the batch and once in its last, partial 32-query chunk.  The rest of the 75
queries are fillers: rows of the store with 0 to 8 substituted columns.  Order: a b c d e f g h, fillers, the twin at 32 (the
lone query of the 33-query batch's second chunk), fillers, a b h at 72..74.

The bases of d, e and the twin have to be farther than D + 1 from every other subject, which random rows are not at L = 31
(unrelated nucleotide rows differ in 3/4 of their columns: two dozen of 10 000 come within 16 of 31).  So the background
never holds, in column c, the letter r[c] of one random reserved row r, and these three bases are r with two columns each
(disjoint) set to another letter; their planted subjects substitute columns outside those six.  Every other base is random
(drawn again while it lies within D + 7 of r).
`inside_steps`: the 4-tile steps of the sample (kth_seed_kernel: step s = tiles 4s .. 4s + 3) the inside subjects of a, b and
h are dealt to in turn; default: every step.
"""
from __future__ import annotations

import zlib

import numpy as np

E = 3
KS = (3, 5, 40)
LENGTHS = (31, 60, 90, 120, 150, 255, 256)
KINDS = ("nt2", "nt3", "aa")
ALPHABET = {"nt2": 0, "nt3": 0, "aa": 1}
PLANES = {"nt2": 2, "nt3": 3, "aa": 5}
STORE_LETTERS = {"nt2": 4, "nt3": 5, "aa": 20}  # as tests/kernel_edges.py: nt3 holds N = 4
ABSENT_LETTER = {"nt2": 4, "aa": 27}
SHAPES = [(kind, L) for kind in KINDS for L in LENGTHS]
N_ROWS = 10241        # 41 tiles, the last one of one row
N_ROWS_WALK = 40961   # 161 tiles: a sample of 80 tiles = 20 steps
WALK_SHAPES = [("aa", 60), ("nt2", 31), ("aa", 150)]
WALK_STEPS = (3, 4, 7, 19)  # under one tile group: the last step before the first bound update, the first after it, the
                            # second update's step, the last step of the sample
N_QUERIES = 75
BATCHES = (75, 33, 1)
FIRST_PART = 1024     # rows of the first append (nt3: N-free)
ENV = {"SMAFA_SORT": "0", "SMAFA_RESORT": "0", "SMAFA_TWO_PHASE": "0", "SMAFA_KTH_SAMPLE_MIN_TILES": "8"}
SEED_BINS = 256       # kernels.hip.h kSeedBins: rows of up to 255 columns are counted in LDS histograms


def seed_kernel(kind, L):
    """the kth_seed_kernel instantiation of a shape (scan_host.hip.h launch_kth_hist), None where the histogram is not used"""
    if L >= SEED_BINS:
        return None
    W = (L + 31) // 32
    ps, pq = {"nt2": (2, 3), "nt3": (3, 3), "aa": (5, 5)}[kind]
    return "smafa::kth_seed_kernel<%d, %d, %d>" % ((ps, pq, W) if W <= 4 else (0, 0, 0))


def level1_prunes(L, bound, prune_p=2e-3):
    """mirror of scan_plan.h prefilter_prunes (kth_plan.h kth_count_first): the k-th modes count first only where this is false"""
    cols = min(32, L)
    if bound >= cols:
        return False
    term, tail = 1.0, 0.0
    for k in range(bound + 1):
        tail += term
        term = term * (cols - k) / (k + 1)
    return tail * 0.5 ** cols <= prune_p


class Case:
    """one store and its 75 queries, planted for one k"""

    def __init__(self, kind, L, k, n=N_ROWS, sample_tiles=20, inside_steps=None):
        assert n % 256 == 1 and n > FIRST_PART
        self.kind, self.L, self.k, self.n = kind, L, k, n
        self.S = 256 * sample_tiles
        self.D = L // 2
        self.n_tiles = (n + 255) // 256
        self.steps = list(range((sample_tiles + 3) // 4)) if inside_steps is None else list(inside_steps)
        assert 0 < self.S < n - 1 and E + 1 <= self.D - 2
        self.rng = rng = np.random.default_rng(zlib.crc32(repr((kind, L, k, n, sample_tiles, self.steps)).encode()))
        self.sl = STORE_LETTERS[kind]
        self.base_letters = 4 if kind != "aa" else 20  # bases hold no N: they are planted in the N-free first part too
        self.reserved = rng.integers(0, self.base_letters, size=L, dtype=np.uint8)
        bg = rng.integers(0, self.sl - 1, size=(n, L), dtype=np.uint8)
        bg += bg >= self.reserved[None, :]  # every letter but the reserved row's, column by column
        if kind == "nt3":  # the first part N-free (there N is drawn again among the other letters)
            head = rng.integers(0, 3, size=(FIRST_PART, L), dtype=np.uint8)
            head += head >= self.reserved[None, :]
            bg[:FIRST_PART] = head
        self.subjects = bg
        self.background = bg.copy()
        self.taken = {}
        self.c_positions = (0, self.S - 1, self.S, n - 1)  # class c's: nobody else's
        self.queries, self.meta = [], []
        self._build()
        self.subjects.setflags(write=False)
        self.queries = np.ascontiguousarray(np.array(self.queries, dtype=np.uint8))
        self.queries.setflags(write=False)
        assert self.queries.shape == (N_QUERIES, L)

    # ---- placing ---------------------------------------------------------------------------------------------
    def parts(self):
        return self.subjects[:FIRST_PART], self.subjects[FIRST_PART:]

    def _free(self, lo, hi):
        for _ in range(10000):
            pos = int(self.rng.integers(lo, hi))
            if pos not in self.taken and pos not in self.c_positions:
                return pos
        raise AssertionError("no room left for planted subjects in [%d, %d)" % (lo, hi))

    def _inside(self, i):
        """a free position inside the sample, in the tiles of the i-th of the steps in turn"""
        s = self.steps[i % len(self.steps)]
        lo, hi = 1024 * s, min(1024 * (s + 1), self.S)
        assert lo < hi, "step %d lies outside the sample" % s
        return self._free(lo, hi)

    def _outside(self):
        return self._free(self.S, self.n - 1)

    def _letters_at(self, pos):
        return 4 if self.kind == "nt3" and pos < FIRST_PART else self.sl

    def _plant(self, pos, base, d, owner, cols=None):
        """subject `pos` = base with exactly d substituted columns (drawn from `cols`), each set to a different letter"""
        assert pos not in self.taken, "planted subject %d would be overwritten" % pos
        pool = np.arange(self.L) if cols is None else np.asarray(cols)
        assert d <= len(pool), "%s L=%d cannot hold %d substitutions" % (self.kind, self.L, d)
        row = base.copy()
        nl = self._letters_at(pos)
        for c in self.rng.choice(pool, size=d, replace=False):
            row[c] = (int(row[c]) + 1 + int(self.rng.integers(0, nl - 1))) % nl
        assert int((row != base).sum()) == d
        self.subjects[pos] = row
        self.taken[pos] = (owner, d)

    def _random_base(self):
        """... farther than D + 7 from the reserved row, so that its subjects (within E + 1 of it) stay out of the neighbourhood
        (D + 1) of d's, e's and the twin's bases (two columns from the reserved row)"""
        while True:
            base = self.rng.integers(0, self.base_letters, size=self.L, dtype=np.uint8)
            if int((base != self.reserved).sum()) >= self.D + 8:
                return base

    def _query(self, cls, base, **expect):
        self.queries.append(base.copy())
        self.meta.append(dict(cls=cls, **expect))
        return len(self.queries) - 1

    # ---- the classes -----------------------------------------------------------------------------------------
    def _a(self):
        k, base = self.k, self._random_base()
        qi = len(self.queries)
        for i in range(k - 1):
            self._plant(self._inside(i), base, E, qi)
        for _ in range(2):
            self._plant(self._outside(), base, E, qi)
        self._plant(self._outside(), base, E + 1, qi)
        self._query("a", base, kth=E, ties_in=k - 1, ties_out=2, rows=k + 1, rows_D=k + 1)

    def _b(self):
        k, base = self.k, self._random_base()
        qi = len(self.queries)
        for i in range(k):
            self._plant(self._inside(i), base, E, qi)
        for _ in range(k):
            self._plant(self._outside(), base, E, qi)
        for _ in range(2):
            self._plant(self._outside(), base, E - 1, qi)
        self._query("b", base, kth=E, ties_in=k, ties_out=k, rows=2 * k + 2, rows_D=2 * k + 2)

    def _c(self):
        base = self._random_base()
        qi = len(self.queries)
        for pos in self.c_positions:
            self._plant(pos, base, E, qi)
        three = self.k == 3  # (a larger k reaches into the background: the oracle says how far)
        self._query("c", base, kth=E if three else None, ties_in=2 if three else None, ties_out=2 if three else None,
                    rows=4 if three else None, rows_D=4 if three else None, at_E=self.c_positions)

    def _reserved_bases(self):
        """three bases = the reserved row with two columns each set to another letter; the columns their subjects may substitute"""
        cols = self.rng.choice(self.L, size=6, replace=False)
        bases = []
        for i in range(3):
            b = self.reserved.copy()
            for c in cols[2 * i: 2 * i + 2]:
                b[c] = (int(b[c]) + 1 + int(self.rng.integers(0, self.base_letters - 1))) % self.base_letters
            bases.append(b)
        return bases, np.setdiff1d(np.arange(self.L), cols)

    def _side(self, i):
        return self._inside(i // 2) if i % 2 == 0 else self._outside()

    def _d(self, base, cols):
        k, D, qi = self.k, self.D, len(self.queries)
        for i in range(k - 2):
            self._plant(self._side(i), base, D, qi, cols)
        for i in range(3):
            self._plant(self._side(i + 1), base, D + 1, qi, cols)
        self._query("d", base, kth=D + 1, rows=k + 1, rows_D=k - 2)

    def _e(self, base, cols):
        k, D, qi = self.k, self.D, len(self.queries)
        for i in range(k):
            self._plant(self._side(i), base, D, qi, cols)
        self._query("e", base, kth=D, rows=k, rows_D=k)

    def _twin(self, base, cols):
        k, D, qi = self.k, self.D, len(self.queries)
        for i in range(k - 1):
            self._plant(self._side(i + 1), base, D, qi, cols)
        for i in range(2):
            self._plant(self._side(i), base, D + 1, qi, cols)
        self._query("twin", base, kth=D + 1, rows=k + 1, rows_D=k - 1)

    def _f(self):
        k, base = self.k, self._random_base()
        qi = len(self.queries)
        tiles = (0, self.n_tiles // 2, self.n_tiles - 2)  # (the last tile's only row belongs to c)
        for i in range(k + 3):
            t = tiles[i % 3]
            self._plant(self._free(256 * t, 256 * (t + 1)), base, 0, qi)
        S = self.S
        inside = sum(1 for i in range(k + 3) if 256 * tiles[i % 3] < S)
        self._query("f", base, kth=0, ties_in=inside, ties_out=k + 3 - inside, rows=k + 3, rows_D=k + 3)

    def _g(self):
        if self.kind == "nt3":
            return self._filler()
        base = np.full(self.L, ABSENT_LETTER[self.kind], dtype=np.uint8)
        self._query("g", base, kth=self.L, ties_in=self.S, ties_out=self.n - self.S, rows=self.n, rows_D=0)

    def _h(self):
        k, base = self.k, self._random_base()
        qi = len(self.queries)
        for i in range(k):
            self._plant(self._inside(i), base, E + 1, qi)
        for _ in range(k):
            self._plant(self._outside(), base, E, qi)
        self._query("h", base, kth=E, ties_in=0, ties_out=k, rows=k, rows_D=k)

    def _filler(self):
        while True:
            pos = int(self.rng.integers(0, self.n))
            if pos not in self.taken and pos not in self.c_positions:
                break
        q = self.background[pos].copy()  # (a background row stays what it is: plants go to other positions)
        self.taken.setdefault(pos, ("filler", 0))
        ql = 5 if self.kind != "aa" else 20
        for c in self.rng.choice(self.L, size=int(self.rng.integers(0, 9)), replace=False):
            q[c] = (int(q[c]) + 1 + int(self.rng.integers(0, ql - 1))) % ql
        self._query("filler", q)

    def _build(self):
        (bd, be, bt), cols = self._reserved_bases()
        self._a()
        self._b()
        self._c()
        self._d(bd, cols)
        self._e(be, cols)
        self._f()
        self._g()
        self._h()
        while len(self.queries) < 32:
            self._filler()
        self._twin(bt, cols)
        while len(self.queries) < N_QUERIES - 3:
            self._filler()
        self._a()
        self._b()
        self._h()

    # ---- what the tests ask ----------------------------------------------------------------------------------
    def planted_steps(self, qi, d):
        """the sample's 4-tile steps that hold a subject planted for query qi at distance d"""
        return sorted({pos // 1024 for pos, (owner, dd) in self.taken.items() if owner == qi and dd == d and pos < self.S})


_cases = {}


def case(kind, L, k, n=N_ROWS, sample_tiles=20, inside_steps=None):
    """built once per process and shared (read-only arrays)"""
    key = (kind, L, k, n, sample_tiles, None if inside_steps is None else tuple(inside_steps))
    if key not in _cases:
        if len(_cases) >= 8:  # (a few at a time: the walk-length stores are 6 MB each)
            _cases.pop(next(iter(_cases)))
        _cases[key] = Case(kind, L, k, n, sample_tiles, inside_steps)
    return _cases[key]


def walk_case(kind, L, k):
    return case(kind, L, k, n=N_ROWS_WALK, sample_tiles=80, inside_steps=WALK_STEPS)

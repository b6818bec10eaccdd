"""Stores of about 70 000 rows whose exact answer to every resident-store call is known by construction
(tests/test_big_store_model.py on the CPU, tests/test_gpu_big_store.py on the device).

The brute-force models beside this file compare all pairs: 2.4 G pair tests at 70 000 rows.  Here a store is made of FAMILIES
that cannot see each other, so the answer of the whole store is the answer of each family, moved to where its rows are.

  templates    A family is one of a dozen TEMPLATES: a small matrix of substitutions, member k changes these slots by these
               offsets (mod the alphabet size).  Offsets are 1 .. 3, so two members differ in a slot exactly where their offsets
               differ, under base 4 and base 20 alike: the in-family distances are those of the offset matrix itself, whatever
               the seed, the alphabet or the columns the slots land on.  No member changes more than S_MAX = 3 slots.
  seeds        Family f's seed spells f in base 4 (nt, 7 digits) or base 20 (aa, 3 digits), every digit repeated r times (16, 20)
               over consecutive columns; the columns left over (8 of nt120) are filled alike in every family.  Two seeds differ in
               at least r columns, a member differs from its seed in at most S_MAX, so two rows of different families are at least
               r - 2 S_MAX apart: 10 (nt120) and 14 (aa60), above the bound D = 5 of every call.  (bound_of asserts this from the
               construction; nothing here asks the engine.)
  interleaving Rows are a seeded shuffle of a list that holds family f size(f) times; its k-th occurrence is member k.  A
               family's local numbers map to global row numbers INCREASINGLY, so every "the smaller number wins" rule of
               include/smafa_amd.h — labels, parents, nearest, the order of a neighbour list — chooses the same row locally and
               globally.
  expectation  Every existing model runs once per template on its few rows (brute_pairs, density_from_pairs, peaks_from_pairs,
               brute_neighbours, expected_levels, expected_reach, expected_stable) and the result is scattered through the
               families' position arrays with vectorised numpy: no step is O(n^2), and no Python loop runs over rows or families.
               tests/test_big_store_model.py holds the scatter to the whole-store brute-force models on a 3 000-row instance.

What does not decompose by family is the consensus under a labelling that ignores the families; consensus_of is the definition
of include/smafa_amd.h as one bincount per column over (group, code), held to consensus_cases.expected_consensus on the CPU.

Inside a family every row is within S_MAX slots of the seed.  Two rows more than D = 5 apart therefore change disjoint triples of
slots, and a third row within 5 of the one is within 5 of every row that changes the same triple: a chain row between two dense
groups is never sparse, and DBSCAN at D = 5 cannot split what single linkage joins through it.  The `bridge` template (two groups
of twelve copies 6 apart, three chain rows between) is where the PEAKS differ from single linkage (two peaks, one component);
`late` (two groups 5 apart that meet only at the last level) is where the STABLE clusters do (two clusters, one component), and
`spokes`, `pair5` and the small families are where DENSITY does (border and noise rows inside a component)."""
import functools

import numpy as np

from smafa_amd import HIT_DTYPE, synth
from components_cases import labels_from_pairs_numpy
from density_cases import density_from_pairs
from forest_cases import expected_levels
from neighbours_cases import brute_neighbours, cut_lists
from peaks_cases import peaks_from_pairs
from reach_cases import expected_reach
from self_join_cases import brute_pairs
from stable_cases import expected_stable

NONE = 0xFFFFFFFF
D = 5
SLOTS = 9     # slots a template may change
S_MAX = 3     # ... of which a member changes at most three
DEFAULT_BLOCK, DEFAULT_STRIDE = 65536, 16  # engine.hip: join_block, join_stride
WINDOW = 4096                              # engine.hip: consensus_chunk


def members(*rows):
    """dicts {slot: offset} -> the template's offset matrix (members x SLOTS, uint8)"""
    out = np.zeros((len(rows), SLOTS), dtype=np.uint8)
    for k, row in enumerate(rows):
        for slot, off in row.items():
            out[k, slot] = off
    return out


def _random_members(seed, count, slots):
    """`count` members that change up to S_MAX of the first `slots` slots; every fourth one repeats an earlier member"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(count):
        if k % 4 == 3:
            rows.append(dict(rows[int(rng.integers(0, k))]))
            continue
        where = rng.choice(slots, size=int(rng.integers(0, S_MAX + 1)), replace=False)
        rows.append({int(c): int(rng.integers(1, 4)) for c in where})
    return members(*rows)


A3, B3, B2 = {0: 1, 1: 1, 2: 1}, {3: 1, 4: 1, 5: 1}, {3: 1, 4: 1}
# name -> (offset matrix, families of it in a full-size store)
TEMPLATES = {
    "single": (members({}), 1000),
    "twins": (members({}, {}), 800),                                                   # an exact copy
    "copies6": (members({}, {}, {0: 1}, {}, {}, {}, {}), 700),
    "star": (members({}, *[{k: 1} for k in range(8)]), 700),                           # distances 1 and 2
    "spokes": (members(A3, {}, B3, {6: 1, 7: 1, 8: 1}), 500),                           # a centre of degree 3, three leaves 6 apart
    "ladder": (members(A3, {3: 1}, B2, {0: 2, 1: 1, 2: 1}, {0: 2, 1: 2, 2: 1}, {3: 2, 4: 1}), 500),  # distances 1 .. 5
    # two groups of twelve copies, 6 apart, and the chain {0: 1} - {} - {3: 1} between them (steps of 1), dealt alternately
    "bridge": (members(*([A3, B3] * 6 + [{0: 1}, {}, {3: 1}] + [B3, A3] * 6)), 520),
    "late": (members(*([B2, A3] * 10)), 400),                                          # two groups of ten copies, 5 apart
    "big40": (_random_members(40, 40, 6), 350),
    "copies20": (members(*([{4: 2}] * 20)), 250),
    "pair5": (members(A3, B2), 400),                                                   # one pair, at the bound
    "pair6": (members(B3, A3), 300),                                                   # two rows just past the bound: no pair
    "offsets": (members({0: 1}, {0: 2}, {0: 3}, {0: 1, 1: 2}, {0: 1, 1: 3}), 500),     # one slot, every offset
    "random12": (_random_members(12, 12, 9), 500),
}
NAMES = list(TEMPLATES)
SIZES = np.array([len(TEMPLATES[t][0]) for t in NAMES])

# name -> (kind, L, digits of a seed, r = columns per digit, N in one spare column)
STORES = {
    "nt120": ("nt", 120, 7, 16, False),   # 2 planes, W = 4
    "aa60": ("aa", 60, 3, 20, False),     # 5 planes, W = 2
    "nt120n": ("nt", 120, 7, 16, True),   # 3 planes: column 116, one of the eight spare ones (about 1 % of a row), holds N everywhere
}
N_COLUMN = 116


def bound_of(name):
    """the least distance between rows of two families, from the construction: r - 2 s"""
    r = STORES[name][3]
    s = max(int((TEMPLATES[t][0] != 0).sum(axis=1).max()) for t in NAMES)
    assert s == S_MAX and r - 2 * s > D, (name, r, s)
    return r - 2 * s


@functools.lru_cache(maxsize=None)
def local(t):
    """the existing models on template t's own rows (the offset matrix: see the module docstring), each once"""
    codes = np.ascontiguousarray(TEMPLATES[NAMES[t]][0])
    m = len(codes)
    pairs = brute_pairs(codes, D)
    out = {"m": m, "pairs": pairs, "levels": expected_levels(codes, D)[:2], "neighbours": brute_neighbours(codes, D)}
    for M in (2, 4):
        out["density", M] = density_from_pairs(m, pairs, M)
    for radius in (0, 2):
        out["peaks", radius] = peaks_from_pairs(m, pairs, radius)
    out["reach"] = expected_reach(codes, D, 3)
    out["stable"] = expected_stable(codes, D, 3, 0)
    return out


def in_family_distances():
    return sorted(set(int(d) for t in range(len(NAMES)) for d in np.unique(local(t)["pairs"]["dist"])))


def greatest_in_family_distance():
    return max(int((a[:, None, :] != a[None, :, :]).sum(axis=2).max()) for a, _ in TEMPLATES.values())


class BigStore:
    """One store and the scatter of the templates' answers.  scale: every template's family count is divided by it (at least one
    family stays), so that scale = 23 gives the 3 000-row instance of the CPU cross-check."""

    def __init__(self, name, scale=1, seed=2024):
        kind, L, digits, r, with_n = STORES[name]
        self.name, self.kind, self.L, self.r, self.bound = name, kind, L, r, bound_of(name)
        rng = np.random.default_rng(seed + 7 * list(STORES).index(name) + scale)
        lc = synth.letter_codes(1 if kind == "aa" else 0)
        base = len(lc)
        assert base == (20 if kind == "aa" else 4) and digits * r <= L
        counts = np.array([max(1, TEMPLATES[t][1] // scale) for t in NAMES])
        # ---- families: template of each, in a seeded order, so that a family's number says nothing about its template
        self.tmpl = rng.permutation(np.repeat(np.arange(len(NAMES)), counts))
        F = self.F = len(self.tmpl)
        assert F <= base ** digits, (F, base, digits)  # every family number has its own spelling
        size = SIZES[self.tmpl]
        # ---- interleaving: the k-th occurrence of f is member k of family f
        fam = np.repeat(np.arange(F), size)
        rng.shuffle(fam)
        n = self.n = len(fam)
        self.fam = fam
        self.row_of = np.argsort(fam, kind="stable")         # row_of[start[f] + k] = the row of member k of family f: increasing in k
        self.start = np.concatenate([[0], np.cumsum(size)[:-1]])
        self.member = np.empty(n, dtype=np.int64)
        self.member[self.row_of] = np.arange(n) - self.start[fam[self.row_of]]
        self.trow = self.tmpl[fam]                           # template of every row
        self.toff = np.concatenate([[0], np.cumsum(SIZES)[:-1]])  # where a template's members begin in a table of all members
        self.key = self.toff[self.trow] + self.member        # every row's place in such a table
        # ---- seeds: digit j of f over the columns j r .. (j + 1) r - 1; the spare columns alike in every family
        seed_idx = np.empty((F, L), dtype=np.int64)
        seed_idx[:] = (np.arange(L) * 7 + 3) % base
        f = np.arange(F)
        for j in range(digits):
            seed_idx[:, j * r:(j + 1) * r] = ((f // base ** j) % base)[:, None]
        # ---- members: the template's slots land on SLOTS distinct columns of the family's own choice (never the N column)
        allowed = np.array([c for c in range(L) if not (with_n and c == N_COLUMN)])
        colmap = allowed[np.argsort(rng.random(size=(F, len(allowed))), axis=1)[:, :SLOTS]]
        table = np.concatenate([TEMPLATES[t][0] for t in NAMES]).astype(np.int64)
        idx = seed_idx[fam]
        cols = colmap[fam]
        at = np.arange(n)[:, None]
        idx[at, cols] = (idx[at, cols] + table[self.key]) % base
        codes = lc[idx]
        if with_n:
            codes[:, N_COLUMN] = 4
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.codes.setflags(write=False)
        self._cache = {}

    def _once(self, key, make):
        if key not in self._cache:
            value = make()
            for part in value if isinstance(value, tuple) else (value,):
                if isinstance(part, np.ndarray):
                    part.setflags(write=False)
            self._cache[key] = value
        return self._cache[key]

    # ---- the two scatters
    def per_member(self, pick, dtype=np.uint32):
        """pick(local(t)) = one value per member -> one value per row"""
        return np.concatenate([np.asarray(pick(local(t))) for t in range(len(NAMES))]).astype(dtype)[self.key]

    def to_rows(self, pick):
        """pick(local(t)) = per member a LOCAL member number or NONE -> per row the global row number or NONE"""
        loc = self.per_member(pick, np.int64)
        none = loc == NONE
        out = self.row_of[self.start[self.fam] + np.where(none, 0, loc)]
        return np.where(none, NONE, out).astype(np.uint32)

    def summed(self, pick):
        """pick(local(t)) = one number per template -> its sum over the families"""
        per_template = np.bincount(self.tmpl, minlength=len(NAMES))
        return int(sum(int(per_template[t]) * int(pick(local(t))) for t in range(len(NAMES))))

    # ---- the calls
    def pairs(self, bound=D):
        def make():
            q, s, d = [], [], []
            for t in range(len(NAMES)):
                loc = local(t)["pairs"]
                base = self.start[np.flatnonzero(self.tmpl == t)][:, None]
                q.append(self.row_of[base + loc["query"].astype(np.int64)[None, :]].ravel())
                s.append(self.row_of[base + loc["subject"].astype(np.int64)[None, :]].ravel())
                d.append(np.tile(loc["dist"], len(base)))
            q, s, d = np.concatenate(q), np.concatenate(s), np.concatenate(d)
            assert (q < s).all()  # the maps are increasing
            order = np.lexsort((s, d, q))
            rows = np.zeros(len(order), dtype=HIT_DTYPE)
            rows["query"], rows["subject"], rows["dist"] = q[order], s[order], d[order]
            return rows
        full = self._once("pairs", make)
        return full if bound == D else np.ascontiguousarray(full[full["dist"] <= bound])

    def pair_count_by_templates(self):
        return self.summed(lambda loc: len(loc["pairs"]))

    def components(self):
        """(labels, count)"""
        return self.levels()[0][D], self.levels()[1][D]

    def levels(self):
        """(labels (D + 1, n), counts)"""
        def make():
            labels = np.stack([self.to_rows(lambda loc, t=t: loc["levels"][0][t]) for t in range(D + 1)])
            counts = [self.summed(lambda loc, t=t: loc["levels"][1][t]) for t in range(D + 1)]
            return np.ascontiguousarray(labels), counts
        return self._once("levels", make)

    def density(self, M):
        def make():
            counts = {k: self.summed(lambda loc: loc["density", M][2][k]) for k in ("clusters", "core", "noise")}
            return self.to_rows(lambda loc: loc["density", M][0]), self.per_member(lambda loc: loc["density", M][1]), counts
        return self._once(("density", M), make)

    def peaks(self, radius):
        """(labels, parents, weights, n_peaks)"""
        def make():
            return (self.to_rows(lambda loc: loc["peaks", radius][0]), self.to_rows(lambda loc: loc["peaks", radius][1]),
                    self.per_member(lambda loc: loc["peaks", radius][2]), self.summed(lambda loc: loc["peaks", radius][3]))
        return self._once(("peaks", radius), make)

    def neighbours(self, k=None):
        """(offsets, neighbours, dists); k: every list cut to its first k (neighbours_cases.cut_lists)"""
        def make():
            locs = [local(t)["neighbours"] for t in range(len(NAMES))]
            begin = np.concatenate([loc[0][:-1].astype(np.int64) for loc in locs])  # per member: where its list begins in its template's
            degree = np.concatenate([np.diff(loc[0].astype(np.int64)) for loc in locs])
            lists = np.concatenate([[0], np.cumsum([len(loc[1]) for loc in locs])[:-1]])  # where a template's lists begin in all lists
            nb = np.concatenate([loc[1] for loc in locs]).astype(np.int64)
            ds = np.concatenate([loc[2] for loc in locs]).astype(np.uint32)
            deg = degree[self.key]
            offsets = np.zeros(self.n + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum(deg)
            first = lists[self.trow] + begin[self.key]
            rank = np.arange(int(deg.sum())) - np.repeat(offsets[:-1].astype(np.int64), deg)
            at = np.repeat(first, deg) + rank
            rows = self.row_of[np.repeat(self.start[self.fam], deg) + nb[at]]
            return offsets, rows.astype(np.uint32), np.ascontiguousarray(ds[at])
        whole = self._once("neighbours", make)
        return whole if k is None else self._once(("neighbours", k), lambda: cut_lists(whole, k))

    def reach(self):
        """(cores, labels (D + 1, n), counts) at min_pts = 3"""
        def make():
            labels = np.stack([self.to_rows(lambda loc, t=t: loc["reach"][1][t]) for t in range(D + 1)])
            counts = [self.summed(lambda loc, t=t: loc["reach"][2][t]) for t in range(D + 1)]
            return self.per_member(lambda loc: loc["reach"][0]), np.ascontiguousarray(labels), counts
        return self._once("reach", make)

    def stable(self):
        """(labels, joined, n_clusters, cores) of self_stable_clusters(D, 3, 0)"""
        def make():
            return (self.to_rows(lambda loc: loc["stable"][0]), self.per_member(lambda loc: loc["stable"][1]),
                    self.summed(lambda loc: loc["stable"][2]), self.per_member(lambda loc: loc["stable"][3]))
        return self._once("stable", make)

    def since(self, mark):
        rows = self.pairs()
        return np.ascontiguousarray(rows[rows["subject"] >= mark])

    def labels_before(self, mark):
        """the component labels of the first `mark` rows alone: what self_components_update is seeded with"""
        rows = self.pairs()
        return self._once(("before", mark), lambda: labels_from_pairs_numpy(mark, rows[rows["subject"] < mark]))

    def window_labels(self, rows=20000):
        """one label over `rows` rows scattered over the store (its value: the smallest of them), the components elsewhere: a
        group that crosses at least four edges of full 4 096-entry windows however the entries are ordered"""
        def make():
            rng = np.random.default_rng(self.n)
            who = np.sort(rng.choice(self.n, size=min(rows, self.n // 3), replace=False))
            labels = self.components()[0].copy()
            labels[who] = who[0]
            return labels
        return self._once(("window", rows), make)

    # ---- the forests: held to their contract, as forest_cases.check_forest and reach_cases.check_reach_forest hold them
    def check_forest(self, edges, level_ends, want_labels, want_counts, cores=None):
        """edges a < b of one family at their true weight (distance; under `cores`, max(distance, core[a], core[b])), ordered by
        weight, level_ends their counts per level and n - the sets of the expected partition, and for every t the edges up to t
        unite exactly the expected sets (as many edges as sets they remove: acyclic)"""
        n = self.n
        assert edges.dtype == HIT_DTYPE and edges.ndim == 1 and level_ends.dtype == np.uint64 and level_ends.shape == (D + 1,)
        assert len(edges) == int(level_ends[-1]) <= n - 1
        a, b, w = (edges[k].astype(np.int64) for k in ("query", "subject", "dist"))
        assert (a < b).all() and (b < n).all()
        assert (self.fam[a] == self.fam[b]).all(), "an edge joins two families"
        true = (self.codes[a] != self.codes[b]).sum(axis=1)
        if cores is not None:
            big = cores.astype(np.int64)
            true = np.maximum(true, np.maximum(big[a], big[b]))
        assert (w == true).all(), "an edge's dist is not its weight"
        assert (w <= D).all() and (np.diff(w) >= 0).all()
        for t in range(D + 1):
            end = int(level_ends[t])
            assert end == int((w <= t).sum()) == n - want_counts[t], (t, level_ends.tolist(), want_counts)
            got = labels_from_pairs_numpy(n, edges[:end])
            assert got.tobytes() == want_labels[t].tobytes(), "level %d: the edges up to it do not unite the expected sets" % t


@functools.lru_cache(maxsize=None)
def big_store(name, scale=1):
    return BigStore(name, scale)


def consensus_of(codes, labels):
    """-> (ids, sizes, consensus[K, L] uint8, nearest, div): consensus_cases.expected_consensus without its loop over groups —
    one bincount per COLUMN over (group, code), argmax (the first maximum: the smallest code), the divergences literally, and
    the first row of every group in the order (group, div, number)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    labels = np.asarray(labels, dtype=np.uint32)
    n, L = codes.shape
    inside = np.flatnonzero(labels != NONE)
    ids, group = np.unique(labels[inside], return_inverse=True)
    K = len(ids)
    cons = np.zeros((K, L), dtype=np.uint8)
    for c in range(L):
        cons[:, c] = np.bincount(group * 32 + codes[inside, c], minlength=K * 32).reshape(K, 32).argmax(axis=1)
    d = (codes[inside] != cons[group]).sum(axis=1)
    div = np.full(n, NONE, dtype=np.uint32)
    div[inside] = d
    order = np.lexsort((inside, d, group))
    first = np.concatenate([[True], np.diff(group[order]) != 0]) if K else np.zeros(0, dtype=bool)
    return (ids.astype(np.uint32), np.bincount(group, minlength=K).astype(np.uint32), cons, inside[order][first].astype(np.uint32), div)

"""Steps, stores and walks of the sequence tests (tests/test_sequence_model.py on the CPU, tests/test_gpu_sequence.py on the
device): every kind of call a resident store handle serves — twenty kinds, 27 steps — interleaved on ONE handle, each answer
held against brute force.

Nothing here calls the library.  A step is a triple (call(store, ctx), check(answer, ctx), verb): `call` is what the GPU test
runs on its handle, `check` holds the answer against an expectation that only composes the brute-force modules beside this one —
self_join_cases.brute_pairs on the code bytes and what components_cases, levels_cases, density_cases, peaks_cases,
neighbours_cases, forest_cases, reach_cases, delta_cases, stable_cases, consensus_cases, chimera_cases, assign_cases and
classify_cases make of those pairs and bytes — and, for the scans, the CPU oracle as tests/test_gpu_parity.py uses it.  Every
expectation is computed once per store (Ctx caches them) and never written again.

Stage A walks the 24 steps a fresh store has (576 ordered pairs, 577 steps run), stage B the 17 verbs of a grown store, the two
delta calls among them (289 ordered pairs, 290 steps run).

circuit(names) orders the steps: a closed walk over the complete directed graph on the names, self-loops included, that has
every ordered pair (a, b) as consecutive steps exactly once — what a consumer leaves on the handle is then seen by every other
consumer, and by itself."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from smafa_amd import _lib, synth
from assign_cases import expected_assign, planted_reads, random_samples, random_weights
from chimera_cases import chimeras_from_pairs
from classify_cases import distances, expected_classify, tree_lineage
from components_cases import labels_from_pairs, n_components
from consensus_cases import expected_consensus
from delta_cases import since
from density_cases import density_from_pairs
from forest_cases import check_forest, expected_levels
from levels_cases import check_nesting
from neighbours_cases import brute_neighbours, cut_lists, same
from peaks_cases import peaks_from_pairs
from reach_cases import check_reach_forest
from stable_cases import expected_stable
from self_join_cases import ONE_SPAN_FAMILIES, SHAPE_TABLE, SHAPES, brute_pairs, planted_store, shape_case

WIDE = "nt330"  # of self_join_cases.WIDE_SHAPES: records of two windows, a two-plane store whose queries have three
STORES = ("nt60", "aa60", WIDE)
# min_pts: at the bound D a family of 10 has degrees up to 9, so 11 asks for a planted copy; at D - 2, 3 splits the thinned families
M_HI, M_LO = 11, 3
REACH_M = M_LO     # (at 11 only the rows beside a copy are not sparse: a forest of a few dozen edges)
CUT = 3            # the neighbours cut
K_MODE = 5         # max_num_hits of the k-mode scan
GROWTH_SEED, GROWTH_FAMILIES = 77, 49  # planted_store(77, kind, L, 49): 510 rows
LATE_ROWS = 36
# planted_bimeras: 8 per base store and 8 per growth piece, 9 rows each; the first parent of a base store is ABUNDANT
BIMERAS, BIMERA_ROWS, BIMERA_SEED, ABUNDANT = 8, 9, 311, 120
READS, N_SAMPLES, RANKS, SLACK = 300, 3, 7, 1  # the reads of the table and classify steps: READS planted on the store at large ...
# ... and per planted bimera 4 and 3 reads of weight 3 that equal parent A and parent B, one of weight 2 that equals the bimera and one of weight 1
# that equals the one-sided row: the table model's subject counts then make the parents 6 and 4.5 times as heavy as the bimera
BIMERA_READS = ((0, 4, 3), (1, 3, 3), (2, 1, 2), (3, 1, 1))  # (which of the four planted rows, reads, the weight of each)
NONE = 0xFFFFFFFF


def late_members(codes, kind, D, rows=LATE_ROWS):
    """`rows` late members of the store's own families: row i of the store with i mod (D + 1) columns substituted (distinct
    columns, each to a different letter of the generator's set).  planted_store(77, ...) shares no family with the store — two
    random rows of 60 columns are never within 5 — so without these an append would add no pair between an old and a new row,
    and a delta call that lost the old rows altogether would pass."""
    rng = np.random.default_rng(GROWTH_SEED + len(codes))
    lc = synth.letter_codes(1 if kind == "aa" else 0)
    inv = np.zeros(256, dtype=np.int64)
    inv[lc] = np.arange(len(lc))
    out = codes[:rows].copy()
    for i in range(rows):
        cols = rng.choice(codes.shape[1], size=i % (D + 1), replace=False)
        out[i, cols] = lc[(inv[out[i, cols]] + rng.integers(1, len(lc), size=len(cols))) % len(lc)]
    return out


def planted_bimeras(pools, kind, seed, abundant=0):
    """BIMERAS two-parent bimeras and what makes them ones, BIMERA_ROWS rows each (the first: abundant - 3 more), shuffled.  The
    planted families hold no bimera: their members are a few columns from ONE seed.  Here A is a row of `pools` (taken from them in
    turn), B = A with four columns moved, two in front of a breakpoint b and two behind it — a seed within 4 of A — and the rows
    added are 3 copies of A (`abundant` copies for the first, a cluster of 100 rows and more for the consensus step), 4 copies
    of B, the bimera A[:b] + B[b:] once — two columns from either parent, each of which is 4 times as heavy at radius 0 — and
    A with its last (or, every second time, first) column moved, once: a row whose parents share no column with it on that
    side.  b: 2, L - 2, the middle and the edges of the first plane word.
    -> (the rows, the distinct ones (BIMERAS, 4, L): A, B, the bimera, the one-sided row)"""
    rng = np.random.default_rng(seed)
    lc = synth.letter_codes(1 if kind == "aa" else 0)
    inv = np.zeros(256, dtype=np.int64)
    inv[lc] = np.arange(len(lc))
    L = pools[0].shape[1]

    def moved(row, cols):
        out = row.copy()
        out[cols] = lc[(inv[out[cols]] + rng.integers(1, len(lc), size=len(cols))) % len(lc)]
        return out

    rows, distinct = [], []
    for k, b in enumerate((2, 31, 32, 33, L // 2, L - 2, 17, L - 15)[:BIMERAS]):
        pool = pools[k % len(pools)]
        a = pool[rng.integers(0, len(pool))]
        head, tail = rng.choice(b, size=2, replace=False), b + rng.choice(L - b, size=2, replace=False)
        other = moved(a, np.concatenate([head, tail]))
        rows += [a] * (abundant if k == 0 and abundant else 3) + [other] * 4
        distinct.append([a, other, np.concatenate([a[:b], other[b:]]), moved(a, np.array([L - 1 if k % 2 == 0 else 0]))])
        rows += distinct[-1][2:]
    rows = np.array(rows, dtype=np.uint8)
    return rows[rng.permutation(len(rows))], np.array(distinct, dtype=np.uint8)


def expected_with_k(all_hits, k):
    """"dist <= the k-th smallest distance of the query" applied to an ordered complete hit list (the rule of
    tests/test_gpu_parity.py)"""
    n = len(all_hits)
    if n == 0:
        return all_hits[:0]
    q = all_hits["query"]
    starts = np.r_[0, np.nonzero(q[1:] != q[:-1])[0] + 1]
    sizes = np.diff(np.r_[starts, n])
    kth = np.where(sizes >= k, all_hits["dist"][np.minimum(starts + k - 1, n - 1)], np.uint32(0xFFFFFFFF))
    return all_hits[all_hits["dist"] <= np.repeat(kth, sizes)]


class Ctx:
    """One store — as pushed (grown = False) or after the growth stage — and its expectations, each computed once."""

    def __init__(self, name, grown):
        if name == WIDE:
            kind, L, n_frac = SHAPE_TABLE[name][:3]
            D = 5
            base = shape_case(name, ONE_SPAN_FAMILIES, D, 4)[0]
        else:
            _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
            base = planted_store(11 + 300 + len(name), kind, L, 300, n_frac)  # the seeds of test_gpu_density.case
        self.name, self.grown, self.kind, self.L, self.D, self.D2 = name, grown, kind, L, D, D - 2
        self.alphabet = 1 if kind == "aa" else 0
        seed = BIMERA_SEED + len(name)
        planted, self.planted = planted_bimeras([base], kind, seed, ABUNDANT)
        self.base = np.ascontiguousarray(np.concatenate([base, planted]))
        piece = planted_store(GROWTH_SEED, kind, L, GROWTH_FAMILIES)
        # (the growth's bimeras: every second one has a parent among the OLD rows, whose new copies make it heavy enough)
        planted, later = planted_bimeras([base, piece], kind, seed + 1)
        self.growth = np.concatenate([piece, late_members(self.base, kind, D), planted])
        if grown:
            self.planted = np.concatenate([self.planted, later])
        self.first_row = len(self.base) if grown else None
        self.codes = np.ascontiguousarray(np.concatenate([self.base, self.growth])) if grown else self.base
        self.codes.setflags(write=False)
        self.n = len(self.codes)
        # 64 queries drawn from the store's families, 0 .. 6 columns away, and 8 unrelated ones
        near = synth.queries(self.base, 64, self.alphabet, seed=5 + len(name), max_subs=6)[0]
        far = synth.subjects(8, L, self.alphabet, seed=6 + len(name), dup_frac=0.0)
        self.queries = np.ascontiguousarray(np.concatenate([near, far]), dtype=np.uint8)
        self._cache = {}

    def _once(self, key, make):
        if key not in self._cache:
            value = make()
            for part in value if isinstance(value, tuple) else (value,):
                if isinstance(part, np.ndarray):
                    part.setflags(write=False)
            self._cache[key] = value
        return self._cache[key]

    def pairs(self, bound):
        """brute-force pairs within `bound` <= D, ordered (query, dist, subject): one brute force per store, at D"""
        assert bound <= self.D
        full = self._once("pairs", lambda: brute_pairs(self.codes, self.D))
        return full if bound == self.D else self._once(("pairs", bound), lambda: np.ascontiguousarray(full[full["dist"] <= bound]))

    def labels(self):
        return self._once("labels", lambda: labels_from_pairs(self.n, self.pairs(self.D)))

    def levels(self):
        """(labels (D + 1, n), counts): forest_cases.expected_levels, which check_forest reads too"""
        return expected_levels(self.codes, self.D)[:2]

    def density(self, bound, min_pts):
        return self._once(("density", bound, min_pts), lambda: density_from_pairs(self.n, self.pairs(bound), min_pts))

    def peaks(self, radius):
        return self._once(("peaks", radius), lambda: peaks_from_pairs(self.n, self.pairs(self.D), radius))

    def neighbours(self, k):
        whole = self._once("neighbours", lambda: brute_neighbours(self.codes, self.D))
        return whole if k is None else self._once(("neighbours", k), lambda: cut_lists(whole, k))

    def scan(self, mode):
        import oracle

        if mode == "fixed":
            return self._once("scan fixed", lambda: oracle.scan_codes(self.codes, self.queries, self.D))
        everything = self._once("scan all", lambda: oracle.scan_codes(self.codes, self.queries, self.L))
        return self._once(("scan", mode), lambda: expected_with_k(everything, K_MODE if mode == "k" else 1))

    def since(self):
        return self._once("since", lambda: since(self.pairs(self.D), self.first_row))

    def stable(self, min_pts=REACH_M):
        return self._once(("stable", min_pts), lambda: expected_stable(self.codes, self.D, min_pts, 0))

    def consensus_labels(self):
        """the brute peak labels with a seeded tenth of the rows unlabelled"""
        def make():
            labels = self.peaks(0)[0].copy()
            labels[np.random.default_rng(21 + self.n).random(self.n) < 0.1] = NONE
            return labels
        return self._once("consensus labels", make)

    def consensus(self):
        return self._once("consensus", lambda: expected_consensus(self.codes, self.consensus_labels()))

    def reads(self):
        """(reads, samples, weights): READS reads planted on the store, strangers among them, at weights 0 .. 5, and the reads of
        BIMERA_READS for every planted bimera of the store, shuffled among them; sample numbers below N_SAMPLES (the host forms
        refuse a read whose sample number is not: only a launch form counts one, in totals[3])"""
        def make():
            reads, weights = [planted_reads(self.codes, self.D, READS, 31 + self.n)], [random_weights(READS, 33 + self.n)]
            for which, count, weight in BIMERA_READS:
                reads.append(np.repeat(self.planted[:, which], count, axis=0))
                weights.append(np.full(len(reads[-1]), weight, dtype=np.uint32))
            reads, weights = np.concatenate(reads), np.concatenate(weights)
            order = np.random.default_rng(35 + self.n).permutation(len(reads))
            return np.ascontiguousarray(reads[order]), random_samples(len(reads), N_SAMPLES, 32 + self.n), np.ascontiguousarray(weights[order])
        return self._once("reads", make)

    def read_distances(self):
        return self._once("read distances", lambda: distances(self.codes, self.reads()[0]))

    def lineage(self):
        return self._once("lineage", lambda: tree_lineage(self.n, RANKS, 34 + self.n))

    def table(self):
        reads, samples, weights = self.reads()
        return self._once("table", lambda: expected_assign(self.codes, reads, self.D, self.peaks(0)[0], samples, N_SAMPLES, weights))

    def classify(self, slack=SLACK):
        reads, samples, weights = self.reads()
        return self._once(("classify", slack), lambda: expected_classify(self.codes, reads, self.D, self.lineage(), slack, samples, N_SAMPLES, weights,
                                                                         dmat=self.read_distances()))

    def given_weights(self):
        """the table model's subject counts, as the weights the second chimera step is given"""
        return self._once("given weights", lambda: self.table()[3].astype(np.uint32))

    def chimeras(self, given):
        """the two chimera steps: counted weights at radius 0 and fold 2; given weights (radius 1) and fold 1"""
        pairs = self.pairs(self.D)
        if given:
            return self._once("chimeras given", lambda: chimeras_from_pairs(self.codes, pairs, 1, 1, self.given_weights()))
        return self._once("chimeras", lambda: chimeras_from_pairs(self.codes, pairs, 0, 2))

    def keep(self):
        """the subset step's mask: a seeded tenth of the rows dropped, the last row among them"""
        def make():
            keep = np.random.default_rng(41 + self.n).random(self.n) >= 0.1
            keep[-1] = False
            return keep
        return self._once("keep", make)

    def subset(self):
        """(old_of_new, rows, pairs at D - 2, scan rows at D) of the store of the kept rows"""
        import oracle

        def make():
            keep = self.keep()
            new_of_old = np.cumsum(keep) - 1
            lower = self.pairs(self.D2)
            pairs = lower[keep[lower["query"]] & keep[lower["subject"]]].copy()  # (renumbering keeps the order: it is monotone)
            pairs["query"], pairs["subject"] = new_of_old[pairs["query"]], new_of_old[pairs["subject"]]
            rows = np.ascontiguousarray(self.codes[keep])
            return np.flatnonzero(keep).astype(np.uint32), rows, pairs, oracle.scan_codes(rows, self.queries, self.D)
        return self._once("subset", make)

    def listed(self):
        """(subject numbers, their rows): descending with every fifth one twice, then row n - 1"""
        def make():
            down = np.arange(self.n - 2, -1, -7)
            listed = np.concatenate([np.sort(np.concatenate([down, down[::5]]))[::-1], [self.n - 1]]).astype(np.uint32)
            return listed, np.ascontiguousarray(self.codes[listed])
        return self._once("listed", make)

    def old_labels(self):
        """brute labels of the first first_row rows alone: what the update is seeded with"""
        old = self.pairs(self.D)
        return self._once("old labels", lambda: labels_from_pairs(self.first_row, old[old["subject"] < self.first_row]))


@functools.lru_cache(maxsize=None)
def context(name, grown=False):
    return Ctx(name, grown)


# ---- the steps
def eq(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, getattr(got, "dtype", None),
                                                                                                  getattr(got, "shape", None), want.shape)
    assert got.tobytes() == want.tobytes(), "%s differs from brute force at %s" % (what, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8])


def check_rows(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype, what
    assert len(got) == len(want), "%s: %d rows, brute force has %d" % (what, len(got), len(want))
    assert got.tobytes() == want.tobytes(), "%s differ from brute force" % what


def call_count_only(store, ctx):
    count = C.c_uint64(0)
    rc = _lib.lib().smafa_db_self_hits(store._h, ctx.D, None, 0, C.byref(count))
    return rc, int(count.value)


def check_count_only(answer, ctx):
    rc, count = answer
    want = len(ctx.pairs(ctx.D))
    assert count == want, "the count-only call counted %d pairs, brute force has %d" % (count, want)
    assert rc == (_lib.ERR_CAPACITY if want else _lib.OK), rc


def check_components(answer, ctx):
    labels, count = answer
    eq(labels, ctx.labels(), "labels")
    assert count == n_components(ctx.labels()), (count, n_components(ctx.labels()))


def check_levels(answer, ctx):
    labels, counts = answer
    want, want_counts = ctx.levels()
    eq(labels, want, "level labels")
    assert list(counts) == list(want_counts), (counts, want_counts)
    check_nesting(labels, counts)


def check_density(bound, min_pts, degrees):
    def check(answer, ctx):
        labels, degs, counts = answer
        want = ctx.density(bound(ctx), min_pts)
        eq(labels, want[0], "density labels")
        if degrees:
            eq(degs, want[1], "degrees")
        else:
            assert degs is None
        assert counts == want[2], (counts, want[2])
    return check


def check_peaks(radius):
    def check(answer, ctx):
        labels, parents, weights, n_peaks = answer
        want = ctx.peaks(radius)
        eq(weights, want[2], "weights")
        eq(parents, want[1], "parents")
        eq(labels, want[0], "peak labels")
        assert n_peaks == want[3], (n_peaks, want[3])
    return check


def check_forest_step(answer, ctx):
    edges, level_ends = answer
    check_forest(ctx.codes, edges, level_ends, ctx.D)


def check_reach_step(answer, ctx):
    edges, level_ends, cores = answer
    check_reach_forest(ctx.codes, edges, level_ends, cores, ctx.D, REACH_M)


INDEX_MAX_COLUMNS = 128  # include/smafa_amd.h, smafa_db_build_index: "Rows of up to 128 columns"


def call_index(store, ctx):
    from smafa_amd import SmafaError

    try:
        return store.build_index(ctx.D)
    except SmafaError as e:  # (the refusal of a wider store is an answer like any other: the scan behind it must still be exact)
        return e


def check_index(answer, ctx):
    """a dict — or, for a store wider than the index takes, the documented refusal; the scan behind it is the check"""
    if ctx.L > INDEX_MAX_COLUMNS:
        assert isinstance(answer, Exception) and answer.code == _lib.ERR_INVALID and "columns" in str(answer), answer
    else:
        assert isinstance(answer, dict) and "max_div_served" in answer, answer


def call_update(store, ctx):
    seed = np.zeros(ctx.n, dtype=np.uint32)
    seed[: ctx.first_row] = ctx.old_labels()
    return store.self_components_update(ctx.first_row, ctx.D, seed)


def check_fields(names, want_of):
    """every part of the answer, by position, byte for byte against want_of(ctx); a trailing count as a number"""
    def check(answer, ctx):
        want = want_of(ctx)
        assert len(answer) >= len(want), (len(answer), len(want))
        for name, g, w in zip(names, answer, want):
            if isinstance(w, np.ndarray):
                eq(g, w, name)
            else:
                assert g == w, (name, g, w)
    return check


STABLE_FIELDS = ("stable labels", "n_clusters", "joined", "cores")  # the order SubjectStore.self_stable_clusters returns them in
CONSENSUS_FIELDS = ("ids", "sizes", "codes", "nearest", "div")  # consensus_cases.check_consensus, against the Ctx's one model answer
CHIMERA_FIELDS = ("flags", "left_parent", "left_len", "right_parent", "right_len", "weights", "n_chimeras")
TABLE_FIELDS = ("entries", "subject", "dist", "subject_counts", "totals")
CLASSIFY_FIELDS = ("entries", "subject", "dist", "taxon", "depth", "ties", "totals")
SUBSET_FIELDS = ("old_of_new", "rows of the subset", "pairs of the subset", "scan rows of the subset")


def call_table(store, ctx):
    reads, samples, weights = ctx.reads()
    return store.assign(reads, ctx.D, labels=ctx.peaks(0)[0], samples=samples, n_samples=N_SAMPLES, weights=weights, subject_counts=True)


def call_classify(store, ctx):
    reads, samples, weights = ctx.reads()
    return store.classify(reads, ctx.D, ctx.lineage(), slack=SLACK, samples=samples, n_samples=N_SAMPLES, weights=weights)


def call_subset(store, ctx):
    """a child store made, asked and destroyed: the step behind this one proves that the parent is as it was"""
    sub, old_of_new = store.subset(ctx.keep())
    try:
        return old_of_new, sub.rows(), sub.self_pairs(ctx.D2), sub.scan(ctx.queries, max_divergence=ctx.D)
    finally:
        sub.close()


def call_rows(store, ctx):
    """-> (every row, the listed rows, the kernels of the first of the two calls: the one that may have to build pos_of[])"""
    whole = store.rows()
    first = store.last_call_kernels()
    return whole, store.rows(ctx.listed()[0]), first


# verb: whose kernels the call may launch (None: a scan, or the index)
Step = namedtuple("Step", "call check verb")
D_OF, D2_OF = (lambda ctx: ctx.D), (lambda ctx: ctx.D2)
STEPS = {
    "pairs": Step(lambda s, c: s.self_pairs(c.D), lambda a, c: check_rows(a, c.pairs(c.D), "pairs"), "pairs"),
    "pairs_count_only": Step(call_count_only, check_count_only, "pairs"),
    "components": Step(lambda s, c: s.self_components(c.D), check_components, "components"),
    "levels": Step(lambda s, c: s.self_component_levels(c.D), check_levels, "levels"),
    "density": Step(lambda s, c: s.self_density(c.D, M_HI), check_density(D_OF, M_HI, True), "density"),
    "density_lower": Step(lambda s, c: s.self_density(c.D2, M_LO, degrees=False), check_density(D2_OF, M_LO, False), "density"),
    "peaks_r0": Step(lambda s, c: s.self_peaks(c.D, 0), check_peaks(0), "peaks"),
    "peaks_r1": Step(lambda s, c: s.self_peaks(c.D, 1), check_peaks(1), "peaks"),
    "neighbours": Step(lambda s, c: s.self_neighbours(c.D), lambda a, c: same(a, c.neighbours(None)), "neighbours"),
    "neighbours_k3": Step(lambda s, c: s.self_neighbours(c.D, k=CUT), lambda a, c: same(a, c.neighbours(CUT)), "neighbours"),
    "forest": Step(lambda s, c: s.self_forest(c.D), check_forest_step, "forest"),
    "reach_forest": Step(lambda s, c: s.self_reach_forest(c.D, REACH_M), check_reach_step, "reach_forest"),
    "scan_fixed": Step(lambda s, c: s.scan(c.queries, max_divergence=c.D), lambda a, c: check_rows(a, c.scan("fixed"), "scan rows"), None),
    "scan_k5": Step(lambda s, c: s.scan(c.queries, max_num_hits=K_MODE), lambda a, c: check_rows(a, c.scan("k"), "k-mode rows"), None),
    "scan_best": Step(lambda s, c: s.scan(c.queries, max_num_hits=1), lambda a, c: check_rows(a, c.scan("best"), "best-hit rows"), None),
    "build_index": Step(call_index, check_index, None),
    # (every output and the count against the Ctx's one stable_cases.expected_stable, as stable_cases.check_stable compares them)
    "stable": Step(lambda s, c: s.self_stable_clusters(c.D, REACH_M, joined=True, cores=True),
                   check_fields(STABLE_FIELDS, lambda c: tuple(c.stable()[k] for k in (0, 2, 1, 3))), "stable"),
    "consensus": Step(lambda s, c: s.cluster_consensus(c.consensus_labels()), check_fields(CONSENSUS_FIELDS, lambda c: c.consensus()), "consensus"),
    "chimeras": Step(lambda s, c: s.self_chimeras(c.D, 2, 0), check_fields(CHIMERA_FIELDS, lambda c: c.chimeras(False)), "chimeras"),
    "chimeras_weights": Step(lambda s, c: s.self_chimeras(c.D, 1, 1, weights=c.given_weights()), check_fields(CHIMERA_FIELDS, lambda c: c.chimeras(True)),
                             "chimeras"),
    "table": Step(call_table, check_fields(TABLE_FIELDS, lambda c: c.table()), "table"),
    "classify": Step(call_classify, check_fields(CLASSIFY_FIELDS, lambda c: c.classify()), "classify"),
    "subset": Step(call_subset, check_fields(SUBSET_FIELDS, lambda c: c.subset()), "subset"),
    "rows": Step(call_rows, check_fields(("rows", "listed rows"), lambda c: (c.codes, c.listed()[1])), "rows"),
    # at the other min_pts: its answer is worth checking (6 to 13 clusters, nine rows in ten noise), but the circuits stay at the 24 and
    # 17 steps the walk is specified with, so it runs in STAGE_B_MIN_PTS alone
    "stable_hi": Step(lambda s, c: s.self_stable_clusters(c.D, M_HI, joined=True, cores=True),
                      check_fields(STABLE_FIELDS, lambda c: tuple(c.stable(M_HI)[k] for k in (0, 2, 1, 3))), "stable"),
    # once the store has grown
    "pairs_since": Step(lambda s, c: s.self_pairs_since(c.first_row, c.D), lambda a, c: check_rows(a, c.since(), "delta pairs"), "pairs_since"),
    "components_update": Step(call_update, check_components, "components_update"),
}
SCANS = ("scan_fixed", "scan_k5", "scan_best")
DELTA = ("pairs_since", "components_update")
STAGE_A = tuple(n for n in STEPS if n not in DELTA + ("stable_hi",))  # 24 steps: 576 ordered pairs
# one step per verb, the delta steps included: 17 steps, 289 ordered pairs.  The density step is the one at the smaller bound and
# the neighbours step the one with the cut (row bounds and cut degrees in J.parent): both follow every call at D
STAGE_B = (("pairs", "components", "levels", "density_lower", "peaks_r0", "neighbours_k3", "forest", "reach_forest") + DELTA +
           ("stable", "consensus", "chimeras", "table", "classify", "subset", "rows"))
# the three scans directly behind the two consumers that leave the sort buffers and the scratch list in their largest state, and
# behind the table call, which trims hits, scratch and J.parent on its way out
STAGE_B_SCANS = tuple(n for after in ("components_update", "neighbours", "table") for scan in SCANS for n in (after, scan))
# the reach forest at REACH_M and the stable clusters at M_HI and at REACH_M, each directly behind each: a stable call that took the
# forest, the cores or the kept list another min_pts left would show
STAGE_B_MIN_PTS = ("reach_forest", "stable_hi", "stable", "stable_hi", "reach_forest", "stable")
# step -> its bound.  The chimera steps keep as the peaks call does and the stable step as the reach forest does (join_chimeras,
# reach_passes in self_join.hip.h: one join where kept_plan finds every pair in the list, the store joined again where not)
KEEPING = {"density": D_OF, "density_lower": D2_OF, "peaks_r0": D_OF, "peaks_r1": D_OF, "forest": D_OF, "reach_forest": D_OF,
           "chimeras": D_OF, "chimeras_weights": D_OF, "stable": D_OF, "stable_hi": D_OF}

# ---- whose kernels a call may launch: every name of last_call_kernels() is a scan (smafa::), the join's own (smafa_join::) or one
# of the verb's — the sets the per-verb tests assert (CC, LV, DN, PK, NB, SF, MR and HEAD, GATHER / FILTER / SEED there; ST, FULL,
# ASSIGN_KERNELS, CLASSIFY_KERNELS, SUBSET_CALL and the unpack kernel for the seven newer verbs), prefixes as tests/kernel_namespaces.py
CONSUMER_NAMESPACES = ("smafa_cc::", "smafa_lv::", "smafa_dn::", "smafa_pk::", "smafa_nb::", "smafa_sf::", "smafa_mr::", "smafa_dl::",
                       "smafa_st::", "consensus::", "chimera::", "assign::", "classify::", "subset::")
INVERSE = "smafa_join::inverse_order_kernel"
OWN_KERNELS = {  # verb -> (prefixes it may launch, one kernel it always launches at these stores; "...<": whatever the planes)
    "pairs": ((), "smafa_join::join_filter_kernel"),
    "components": (("smafa_cc::",), "smafa_cc::flatten_labels_kernel"),
    "levels": (("smafa_lv::",), "smafa_lv::flatten_levels_kernel"),
    "density": (("smafa_dn::",), "smafa_dn::flatten_density_kernel"),
    "peaks": (("smafa_pk::",), "smafa_pk::settle_kernel"),
    "neighbours": (("smafa_nb::",), "smafa_nb::emit_kernel"),
    "forest": (("smafa_sf::",), "smafa_sf::span_edges_kernel"),
    "reach_forest": (("smafa_mr::", "smafa_sf::init_forest_kernel", "smafa_sf::star_roots_kernel"), "smafa_mr::core_dist_kernel"),
    "pairs_since": (("smafa_dl::gather_records_kernel", "smafa_dl::delta_filter_kernel"), "smafa_dl::delta_filter_kernel"),
    "components_update": (("smafa_dl::gather_records_kernel", "smafa_dl::seed_parents_kernel", "smafa_cc::link_rows_kernel",
                           "smafa_cc::flatten_labels_kernel"), "smafa_dl::seed_parents_kernel"),
    # the reach forest's passes in front of its own; the peaks call's first phase in front of its own
    "stable": (("smafa_st::", "smafa_mr::", "smafa_sf::init_forest_kernel", "smafa_sf::star_roots_kernel"), "smafa_st::assign_kernel"),
    "chimeras": (("chimera::", "smafa_pk::init_peaks_kernel", "smafa_pk::weigh_keep_kernel"), "chimera::verdict_kernel"),
    "consensus": (("consensus::",), "consensus::finish_groups_kernel"),
    "table": (("assign::",), "assign::fold_kernel"),
    "classify": (("classify::", "assign::best_kernel", "assign::heads_kernel", "assign::fold_kernel"), "classify::key_kernel"),
    "subset": (("subset::keep_flags_kernel", "subset::run_ends_kernel", "subset::move_rows_kernel"), "subset::move_rows_kernel"),
    "rows": (("subset::unpack_rows_kernel<",), "subset::unpack_rows_kernel<"),
}
# verb -> what it may launch of smafa:: and smafa_join:: where that is not "the scans and the join's own": the consensus scans
# nothing, the read tables scan and never join (no record kernel, no pos_of[]), the subset fills the child's zone words, the rows
# call brings pos_of[] up to date and launches nothing else
SHARED_KERNELS = {"consensus": (), "table": ("smafa::",), "classify": ("smafa::",), "subset": ("smafa::zone_kernel",), "rows": (INVERSE,)}
JOINING = tuple(v for v in OWN_KERNELS if v not in SHARED_KERNELS)  # the verbs that join the store: every one scans it block by block
# the verbs whose join needs pos_of[] (join_positions in self_join.hip.h: every joining verb but the two that link whole lists)
POSITIONED = tuple(v for v in JOINING if v not in ("components", "levels")) + ("rows",)


def check_kernels(verb, kernels):
    """the kernels of a call: the verb's own, and none of another verb's"""
    own, always = OWN_KERNELS[verb]
    assert any(k.startswith(always) for k in kernels) if always.endswith("<") else always in kernels, \
        "%s is not among the call's kernels %s" % (always, kernels)
    delta = verb in ("pairs_since", "components_update")
    shared = SHARED_KERNELS.get(verb, ("smafa::", "smafa_join::"))
    for k in kernels:
        assert k.startswith(("smafa::", "smafa_join::") + CONSUMER_NAMESPACES), "%s in %s" % (k, kernels)
        if k.startswith(CONSUMER_NAMESPACES):
            assert own and k.startswith(own), "%s is no kernel of a %s call: %s" % (k, verb, kernels)
        else:
            assert shared and k.startswith(shared), "%s in a %s call: %s" % (k, verb, kernels)
        # of the join's own kernels the filter is the plain pairs call's, and a delta call's records are gathered, not stored
        assert k != "smafa_join::join_filter_kernel" or verb == "pairs", "%s in a %s call: %s" % (k, verb, kernels)
        assert k != "smafa_join::store_records_kernel" or not delta, "%s in a %s call: %s" % (k, verb, kernels)


# ---- the configs of the GPU test
KNOBS = ("SMAFA_DENSITY_KEEP_MAX", "SMAFA_JOIN_BLOCK", "SMAFA_JOIN_STRIDE", "SMAFA_JOIN_SCRATCH_MAX")
# kept_overflow: the kept list holds half the pairs at D.  At these stores more than half the pairs lie within D - 2 too, so there
# every keeping call overflows; kept_alternating puts the capacity between the pairs within D - 2 of the grown store and the pairs
# within D of the store as pushed: the calls at D overflow, the density call at D - 2 fits, before the growth and after it, and the
# walk alternates the two paths on one handle.
CONFIGS = ("default", "kept_overflow", "kept_alternating", "small_blocks")


def knobs(config, ctx):
    """the environment of a config, read when the handle is made; ctx: the store as pushed"""
    at_D, below = len(ctx.pairs(ctx.D)), len(context(ctx.name, True).pairs(ctx.D2))  # (below: after the growth, the larger count)
    return {"default": {}, "kept_overflow": {"SMAFA_DENSITY_KEEP_MAX": at_D // 2},
            "kept_alternating": {"SMAFA_DENSITY_KEEP_MAX": (at_D + below) // 2},
            # the values of tests/test_gpu_neighbours.py and tests/test_gpu_forest.py: many spans, cut pieces, a scratch list and an
            # entry list that grow in the middle of a call
            "small_blocks": {"SMAFA_JOIN_BLOCK": 192, "SMAFA_JOIN_STRIDE": 3, "SMAFA_JOIN_SCRATCH_MAX": 4096}}[config]



# ---- the walk
def circuit(names):
    """A closed walk over the complete directed graph on `names`, self-loops included, as its k * k steps: every ordered pair
    (a, b) is two consecutive steps exactly once, the last step and the first being consecutive too.  Hierholzer with an
    explicit stack; every vertex tries its successors in the order of `names`, so the walk depends on that order alone."""
    names = list(names)
    k = len(names)
    assert k and len(set(names)) == k, names
    tried = {a: 0 for a in names}  # the successors of a already used: names[: tried[a]]
    stack, walk = [names[0]], []
    while stack:
        a = stack[-1]
        if tried[a] < k:
            tried[a] += 1
            stack.append(names[tried[a] - 1])
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == k * k + 1 and walk[0] == walk[-1]
    return walk[:-1]


def closed(walk):
    """the steps to run: the circuit and its first step once more, so that every ordered pair is RUN as consecutive steps"""
    return list(walk) + [walk[0]]


def consecutive_pairs(steps):
    return list(zip(steps[:-1], steps[1:]))

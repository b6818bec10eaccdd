"""The model and the fixtures of the classification tests (tests/test_classify_model.py, tests/test_gpu_classify.py,
tests/test_classify_abi.py).

The expected answer never comes from the library: it is the header's definition worked in numpy from the code bytes.  The distance
of a read and a subject is the number of columns whose codes differ; d(q) is the smallest within the bound, the anchor the first
subject at it (numpy's argmin), B(q) the subjects within min(d(q) + slack, bound), cp(anchor, s) the number of leading ranks at
which the two lineage rows hold the same id that is not NONE, depth the minimum of cp over B(q), the taxon the anchor's id at rank
depth - 1 (ROOT at depth 0, NONE without an anchor), and the table np.unique over the (taxon, sample) keys of the reads of weight
> 0 with their weights summed."""
import functools

import numpy as np

from assign_cases import NONE, TABLE_DTYPE, shape_reads

ROOT = 0xFFFFFFFE
CLASSIFY_KERNELS = ["classify::start_kernel", "assign::best_kernel", "classify::agree_kernel", "classify::key_kernel", "assign::heads_kernel",
                    "assign::fold_kernel"]
FIELDS = ("entries", "subject", "dist", "taxon", "depth", "ties", "totals")


def distances(subject_codes, read_codes, slab=64):
    """(m, n) int32: the number of differing columns of every read and subject"""
    subjects = np.ascontiguousarray(subject_codes, dtype=np.uint8)
    reads = np.ascontiguousarray(read_codes, dtype=np.uint8).reshape(-1, subjects.shape[1])
    out = np.zeros((len(reads), len(subjects)), dtype=np.int32)
    for a in range(0, len(reads), slab):
        out[a:a + slab] = (reads[a:a + slab, None, :] != subjects[None, :, :]).sum(-1)
    return out


def common_prefix(lineage, a, members):
    """cp(a, s) for every s of members: the leading ranks r with lineage[a][r] == lineage[s][r] != NONE"""
    same = (lineage[members] == lineage[a][None, :]) & (lineage[a][None, :] != NONE)
    return np.cumprod(same, axis=1).sum(axis=1)


def members_of(d_row, D, slack):
    """-> (anchor, d, members) of one read's distances; (None, None, []) without a subject within D"""
    if len(d_row) == 0 or d_row.min() > D:
        return None, None, np.zeros(0, dtype=np.int64)
    anchor = int(d_row.argmin())
    low = int(d_row[anchor])
    return anchor, low, np.flatnonzero(d_row <= min(low + slack, D))


def expected_classify(subject_codes, read_codes, D, lineage, slack=0, samples=None, n_samples=None, weights=None, dmat=None):
    """-> (entries, subject, dist, taxon, depth, ties, totals) as the contract of include/smafa_amd.h defines them"""
    lineage = np.asarray(lineage, dtype=np.uint32)
    assert lineage.ndim == 2 and len(lineage) == len(subject_codes)
    d_all = distances(subject_codes, read_codes) if dmat is None else dmat
    m = len(d_all)
    subject, dist, taxon, depth = (np.full(m, NONE, dtype=np.uint32) for _ in range(4))
    ties = np.zeros(m, dtype=np.uint32)
    for q in range(m):
        anchor, low, members = members_of(d_all[q], D, slack)
        if anchor is None:
            continue
        deep = int(common_prefix(lineage, anchor, members).min())
        subject[q], dist[q], depth[q], ties[q] = anchor, low, deep, len(members)
        taxon[q] = lineage[anchor][deep - 1] if deep else ROOT
    samples = np.zeros(m, dtype=np.uint32) if samples is None else np.asarray(samples, dtype=np.uint32)
    weights = np.ones(m, dtype=np.uint32) if weights is None else np.asarray(weights, dtype=np.uint32)
    if n_samples is None:
        n_samples = int(samples.max()) + 1 if m else 1
    found = subject != NONE
    stray = samples >= n_samples  # such a read takes no part in anything but totals[3]
    w = np.where(stray, 0, weights).astype(np.uint64)
    live = w > 0
    keys = (taxon[live].astype(np.uint64) << np.uint64(32)) | samples[live].astype(np.uint64)
    uniq, inverse = np.unique(keys, return_inverse=True)
    entries = np.zeros(len(uniq), dtype=TABLE_DTYPE)
    entries["label"] = (uniq >> np.uint64(32)).astype(np.uint32)
    entries["sample"] = (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    np.add.at(entries["count"], inverse, w[live])
    totals = np.array([len(entries), w[found].sum(), w[~found].sum(), stray.sum(), w[found & (depth == 0)].sum(), (~stray & (ties > 1)).sum()],
                      dtype=np.uint64)
    return entries, subject, dist, taxon, depth, ties, totals


# ---- the fixtures of the every-shape test: a store of self_join_cases.SHAPE_STORES with TIE FAMILIES appended, so that ties are
# the rule.  A tie family is a centre row far from everything, an exact copy of it (the twin: a tie at slack 0) and three siblings
# that each differ from the centre in one column (members from slack 1 on).  The reads are assign_cases.shape_reads' with
# TIE_READS reads that equal a centre.
TIE_READS = 140
SIBLINGS = 3


def tie_plan(R):
    """[(twin_rank, sibling_rank, cut, who)] per tie family: the twin's lineage leaves the centre's at twin_rank, the siblings' at
    sibling_rank (R: never); cut / who: the lineage of `who` ("centre", "twin", "sibling" or None) ends behind `cut` ranks.  The
    centre comes first in the store, so it is the anchor.  Families 0 .. R give every depth 0 .. R at every slack; the last four
    hold the NONE tails: the anchor's row the shortest, the twin's the shortest, a sibling's shorter than the anchor's (it counts
    from slack 1 on), and a sibling with no lineage at all."""
    plan = [(f, f, None, None) for f in range(R + 1)]
    half = R // 2
    return plan + [(R, R, half, "centre"), (R, R, half, "twin"), (R, R, half, "sibling"), (R, R, 0, "sibling")]


def tree_lineage(n, R, seed):
    """a lineage row per store row from a binary tree of five forking ranks (one child per node below them): ids are unique per
    node; a quarter of the rows end early, some at once"""
    rng = np.random.default_rng(seed)
    leaf = rng.integers(0, 32, size=n)
    rows = np.zeros((n, R), dtype=np.uint32)
    for r in range(R):
        rows[:, r] = (r << 8) | (leaf >> max(0, 4 - r)) if r < 5 else (r << 8) | leaf
    rows += 1
    length = np.where(rng.random(n) < 0.25, rng.integers(0, R + 1, size=n), R)
    rows[np.arange(R)[None, :] >= length[:, None]] = NONE
    return rows


@functools.lru_cache(maxsize=None)
def tie_case(name, families, D, max_subs=4):
    """-> (store codes, reads, distance matrix): the shape's store with the rows of the largest plan's tie families appended (the
    same rows serve every R), and shape_reads' reads with TIE_READS centre reads, shuffled"""
    codes, reads, _, _ = shape_reads(name, families, D, max_subs)
    rng = np.random.default_rng(9000 + families + D + len(name))
    L = codes.shape[1]
    letters = np.unique(codes[codes != 4]) if codes.max() <= 4 else np.unique(codes)
    F = len(tie_plan(16))
    extra, centres = [], []
    for _ in range(F):
        centre = letters[rng.integers(0, len(letters), size=L)]
        centres.append(centre)
        extra += [centre, centre]  # the centre, then its twin
        for k in range(SIBLINGS):
            sibling = centre.copy()
            sibling[k % L] = letters[letters != centre[k % L]][0]
            extra.append(sibling)
    store = np.ascontiguousarray(np.concatenate([codes, np.array(extra, dtype=np.uint8)]), dtype=np.uint8)
    tie_reads = np.array([centres[i % F] for i in range(TIE_READS)], dtype=np.uint8)
    all_reads = np.concatenate([reads, tie_reads])
    all_reads = np.ascontiguousarray(all_reads[rng.permutation(len(all_reads))], dtype=np.uint8)
    dmat = distances(store, all_reads)
    for a in (store, all_reads, dmat):
        a.setflags(write=False)
    return store, all_reads, dmat


def tie_lineage(name, families, D, max_subs, R):
    """the lineage rows of tie_case's store for R ranks: tree_lineage for the shape's rows, tie_plan(R) for the tie families (the
    families behind the plan's repeat it)"""
    store, _, _ = tie_case(name, families, D, max_subs)
    per = 2 + SIBLINGS
    F = len(tie_plan(16))
    n0 = len(store) - F * per
    rows = np.full((len(store), R), NONE, dtype=np.uint32)
    rows[:n0] = tree_lineage(n0, R, 77 + R)
    plan = tie_plan(R)
    for f in range(F):
        twin_rank, sibling_rank, cut, who = plan[f % len(plan)]
        at = n0 + f * per
        base = 0x10000 + f * 0x100  # ids of this family: the centre's path, the twin's and each sibling's behind their forks
        centre = base + np.arange(R, dtype=np.uint32)
        rows[at] = centre
        rows[at + 1] = np.where(np.arange(R) < twin_rank, centre, base + 0x20 + np.arange(R))
        for k in range(SIBLINGS):
            rows[at + 2 + k] = np.where(np.arange(R) < sibling_rank, centre, base + 0x40 + 0x20 * k + np.arange(R))
        if who is not None:
            row = {"centre": at, "twin": at + 1, "sibling": at + 2}[who]
            rows[row, cut:] = NONE
    return rows


def coverage(store, dmat, D, lineage, slack):
    """what the every-shape test must not pass without, from the MODEL's view of the inputs: -> (share of the assigned reads with
    ties > 1, the set of depths, anchor's row the shortest, another member's the shortest, some read unassigned)"""
    length = (np.cumprod(lineage != NONE, axis=1)).sum(axis=1)
    tied = assigned = 0
    depths, anchor_shortest, other_shortest, unassigned = set(), False, False, False
    for q in range(len(dmat)):
        anchor, _, members = members_of(dmat[q], D, slack)
        if anchor is None:
            unassigned = True
            continue
        assigned += 1
        tied += len(members) > 1
        deep = int(common_prefix(lineage, anchor, members).min())
        depths.add(deep)
        others = members[members != anchor]
        if len(others):
            low = int(length[others].min())
            anchor_shortest |= length[anchor] < low and deep == length[anchor]
            other_shortest |= low < length[anchor] and deep == low
    return tied / max(assigned, 1), depths, anchor_shortest, other_shortest, unassigned


# ---- the taxonomy file of `smafa classify`: ids interned by (parent id, name) in order of first appearance
def intern_taxonomy(n, lines):
    """lines: [(i, [name, ...])] in file order -> (lineage (n, R) uint32, names per id, parent per id)"""
    ids, names, parents, rows = {}, [], [], {}
    for i, path in lines:
        up, row = NONE, []
        for name in path:
            if (up, name) not in ids:
                ids[(up, name)] = len(names)
                names.append(name)
                parents.append(up)
            up = ids[(up, name)]
            row.append(up)
        rows[i] = row
    R = max([len(r) for r in rows.values()] + [1])
    lineage = np.full((n, R), NONE, dtype=np.uint32)
    for i, row in rows.items():
        lineage[i, :len(row)] = row
    return lineage, names, parents


def lineage_text(taxon, names, parents):
    if taxon == NONE:
        return "unassigned"
    if taxon == ROOT:
        return "root"
    path = []
    while taxon != NONE:
        path.append(names[taxon])
        taxon = parents[taxon]
    return ";".join(reversed(path))


def entry_lines(entries, names, parents):
    return "".join("%s\t%d\t%d\n" % (lineage_text(int(e["label"]), names, parents), e["sample"], e["count"]) for e in entries).encode()


def per_read_lines(subject, dist, ties, depth, taxon, names, parents):
    show = lambda v: -1 if v == NONE else int(v)  # noqa: E731
    return "".join("%d\t%d\t%d\t%d\t%d\t%s\n" % (q, show(subject[q]), show(dist[q]), ties[q], show(depth[q]),
                                                 lineage_text(int(taxon[q]), names, parents)) for q in range(len(subject))).encode()

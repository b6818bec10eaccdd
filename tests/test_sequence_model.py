"""CPU model of the sequence tests (tests/sequence_cases.py, run on the device by tests/test_gpu_sequence.py): the walk has
every ordered pair of steps exactly once — 576 pairs of the 24 steps of stage A, 289 pairs of the 17 of stage B —, every store
gives every step an answer worth checking, and every checker refuses an answer with one element off.

The answers the checkers are fed are made here from brute force — for the two forests by a plain Kruskal over the brute-force
pairs, for the seven newer verbs by the models of their own case modules — never by the library: this file passes without a GPU."""
import collections

import numpy as np
import pytest

from smafa_amd import HIT_DTYPE, SmafaError, _lib
from classify_cases import ROOT
from components_cases import n_components
from consensus_cases import tied_columns
from delta_cases import has_both_kinds
from density_cases import kinds
from peaks_cases import moved_and_multi_step
from reach_cases import NONE, weighted_pairs
from sequence_cases import (ABUNDANT, BIMERA_ROWS, BIMERAS, CONFIGS, CUT, DELTA, INDEX_MAX_COLUMNS, INVERSE, JOINING, KEEPING, M_HI, M_LO, OWN_KERNELS, POSITIONED,
                            REACH_M, SCANS, SHARED_KERNELS, STAGE_A, STAGE_B, STAGE_B_MIN_PTS, STAGE_B_SCANS, STEPS, STORES, check_kernels, circuit, closed,
                            consecutive_pairs, context, knobs)


# ---- the walk
@pytest.mark.parametrize("names", [("a",), ("a", "b"), ("a", "b", "c"), STAGE_A, STAGE_B], ids=["k1", "k2", "k3", "stage_a", "stage_b"])
def test_circuit_has_every_ordered_pair_once(names):
    k = len(names)
    walk = circuit(names)
    assert len(walk) == k * k and set(walk) == set(names)
    pairs = collections.Counter(consecutive_pairs(closed(walk)))  # (closed: the last step is followed by the first)
    assert len(pairs) == k * k and set(pairs.values()) == {1}
    assert set(pairs) == {(a, b) for a in names for b in names}
    assert circuit(list(names)) == walk  # no seed, no set or dict order: the same walk every time
    if k > 1:
        assert circuit(tuple(reversed(names))) != walk  # (the order of the names is what decides)


def test_the_stages_cover_the_steps():
    assert len(STAGE_A) == 24 and len(STAGE_B) == 17 and set(DELTA) <= set(STAGE_B) and not set(DELTA) & set(STAGE_A)
    assert set(STAGE_A) | set(STAGE_B) == set(STEPS) - {"stable_hi"} and len(STEPS) == 27
    # the one step outside the circuits: behind and in front of the reach forest and the stable step at the other min_pts
    assert {("reach_forest", "stable_hi"), ("stable_hi", "stable"), ("stable", "stable_hi"), ("stable_hi", "reach_forest")} <= set(consecutive_pairs(list(STAGE_B_MIN_PTS)))
    assert STEPS["stable_hi"].verb == "stable" and M_HI != REACH_M
    # what a small_blocks walk of stage A finds outside the verbs that join the store
    assert {STEPS[n].verb for n in STAGE_A} - set(JOINING) == {None, "consensus", "table", "classify", "subset", "rows"}
    assert len(closed(circuit(STAGE_A))) == 577 and len(closed(circuit(STAGE_B))) == 290
    verbs = {STEPS[n].verb for n in STAGE_B}
    assert verbs == set(OWN_KERNELS) and len(verbs) == 17 and len(STAGE_B) == len(verbs)  # one step per verb
    assert {STEPS[n].verb for n in STAGE_A} == set(OWN_KERNELS) - {"pairs_since", "components_update"} | {None}
    # each scan once directly behind components_update, once directly behind neighbours and once directly behind table
    assert sorted(consecutive_pairs(list(STAGE_B_SCANS))[::2]) == sorted((a, s) for a in ("components_update", "neighbours", "table") for s in SCANS)
    assert set(KEEPING) == {n for n in STEPS if STEPS[n].verb in ("density", "peaks", "forest", "reach_forest", "chimeras", "stable")}
    # the verbs that join the store, and of them the ones whose join needs pos_of[]; the other five each have their own rule
    assert set(JOINING) | set(SHARED_KERNELS) == set(OWN_KERNELS) and len(JOINING) == 12 and not set(JOINING) & set(SHARED_KERNELS)
    assert set(POSITIONED) == set(JOINING) - {"components", "levels"} | {"rows"}


# ---- the stores
@pytest.mark.parametrize("name", STORES)
def test_every_step_has_an_answer_worth_checking(name):
    for grown in (False, True):
        ctx = context(name, grown)
        n, D, D2 = ctx.n, ctx.D, ctx.D2
        # (the planted families, the growth piece and the late members as before; BIMERAS x BIMERA_ROWS planted rows in each of the
        # two pieces, and the abundant parent's further copies in the first)
        planted = BIMERAS * BIMERA_ROWS
        assert planted == 72 and ABUNDANT - 3 == 117
        assert n == {False: {"nt60": 3209, "aa60": 3209}.get(name, 1209), True: {"nt60": 3827, "aa60": 3827}.get(name, 1827)}[grown]
        assert n == {"nt60": 3020, "aa60": 3020}.get(name, 1020) + planted + ABUNDANT - 3 + (546 + planted if grown else 0)
        pairs, lower = ctx.pairs(D), ctx.pairs(D2)
        assert len(pairs) > 2000 and 0 < len(lower) < len(pairs)
        assert set(np.unique(pairs["dist"])) == set(range(D + 1)) and int(lower["dist"].max()) == D2
        _, counts = ctx.levels()
        assert any(counts[t + 1] < counts[t] for t in range(D)) and counts[D] == n_components(ctx.labels())
        for bound, m in ((D, M_HI), (D2, M_LO)):  # the two density steps: core, border and noise rows in each
            labels, degrees, _ = ctx.density(bound, m)
            assert all(bool(k.any()) for k in kinds(labels, degrees, m)), (name, grown, bound, m)
        for radius in (0, 1):
            moved, multi = moved_and_multi_step(ctx.peaks(radius))
            assert moved > 0 and multi > 0, (name, radius)
        assert ctx.peaks(0)[2].tobytes() != ctx.peaks(1)[2].tobytes()  # (the radius matters)
        offsets = ctx.neighbours(None)[0]
        assert int(np.diff(offsets.astype(np.int64)).max()) > CUT and len(ctx.neighbours(CUT)[1]) < len(ctx.neighbours(None)[1])
        edges, ends = forest_of(ctx)
        assert len(set(edges["dist"].tolist())) >= 2 and 0 < int(ends[0]) < int(ends[-1])
        cores = weighted_pairs(ctx.codes, D, REACH_M)[0]
        assert (cores == NONE).any() and (cores != NONE).any() and len(set(cores.tolist())) > 2
        for mode in ("fixed", "k", "best"):
            rows = ctx.scan(mode)
            answered = len(set(rows["query"].tolist()))  # (no bound: every query has rows; at D the unrelated ones have none)
            assert len(rows) >= 64 and (32 <= answered <= 64 if mode == "fixed" else answered == 72), (name, mode, answered)
        assert len(ctx.scan("best")) < len(ctx.scan("k"))
        worth_checking_the_newer_steps(ctx)
        if grown:
            assert ctx.first_row == context(name).n and has_both_kinds(ctx.since(), ctx.first_row, D)
            # the update has work to do: new rows that join a set of old rows, and new rows that make sets of their own
            new = ctx.labels()[ctx.first_row:]
            assert (new < ctx.first_row).any() and (new >= ctx.first_row).any() and ctx.labels()[: ctx.first_row].tobytes() == ctx.old_labels().tobytes()


def worth_checking_the_newer_steps(ctx):
    """the conditions on the brute-force answers of the eight newer steps: a step whose right answer is trivial tests nothing"""
    n, D = ctx.n, ctx.D
    where = (ctx.name, ctx.grown)
    # ---- the chimera steps.  (A row has both parents or none: "a parent on one side only" is a row whose parents share a column
    # with it on one side only — one length is 0, the other is not.)
    counted, given = ctx.chimeras(False), ctx.chimeras(True)
    has = counted.left_parent != NONE
    assert (has == (counted.right_parent != NONE)).all()
    one_side = has & ((counted.left_len == 0) != (counted.right_len == 0))
    assert counted.n_chimeras >= 8 and int(one_side.sum()) >= 8, (where, counted.n_chimeras, int(one_side.sum()))
    assert (has & (counted.flags == 0)).any() and (~has).any() and (has & (counted.left_parent != counted.right_parent)).any(), where
    assert counted.weights.tobytes() != given.weights.tobytes() and (given.weights == 0).any() and (given.weights > 1).any()
    assert (counted.left_parent != given.left_parent).any() or (counted.right_parent != given.right_parent).any()
    # the step with the weights given is held to what the counted one is: the reads planted on the bimeras' rows (BIMERA_READS)
    # make the table model's subject counts flag them
    has = given.left_parent != NONE
    assert (has == (given.right_parent != NONE)).all()
    one_side = has & ((given.left_len == 0) != (given.right_len == 0))
    assert given.n_chimeras >= 8 and int(one_side.sum()) >= 8, (where, given.n_chimeras, int(one_side.sum()))
    assert (has & (given.flags == 0)).any() and (~has).any() and (has & (given.left_parent != given.right_parent)).any(), where
    # ---- stable, at REACH_M and — outside the circuits — at M_HI, where nine rows in ten are noise
    for m in (REACH_M, M_HI):
        labels, joined, count, cores = ctx.stable(m)
        assert count >= 3 and (labels == NONE).any() and (labels != NONE).any() and len(set(joined[joined != NONE].tolist())) >= 2, (where, m, count)
        assert labels.tobytes() != ctx.density(D, m)[0].tobytes()
    assert ctx.stable()[0].tobytes() != ctx.stable(M_HI)[0].tobytes() and ctx.stable()[3].tobytes() != ctx.stable(M_HI)[3].tobytes()
    # ---- consensus
    given_labels = ctx.consensus_labels()
    assert (given_labels == NONE).any() and given_labels.tobytes() != ctx.peaks(0)[0].tobytes()
    ids, sizes, cons, nearest, div = ctx.consensus()
    assert (sizes == 1).any() and int(sizes.max()) >= 100, (where, int(sizes.max()))
    assert tied_columns(ctx.codes, given_labels) >= 1 and int(div[div != NONE].max()) > 0
    # ---- table and classify
    reads = ctx.reads()[0]
    assert len(reads) >= 200 and len(reads) > len(ctx.queries)
    entries, subject, dist, subject_counts, totals = ctx.table()
    d = ctx.read_distances()
    low = d.min(axis=1)
    assert (subject == NONE).any() and (low[subject == NONE] > D).all() and (low[subject != NONE] <= D).all()
    assert set(dist[subject != NONE].tolist()) == set(range(D + 1))
    assert (((d == low[:, None]).sum(axis=1) >= 2) & (low <= D)).any(), where  # two or more equally best subjects: the copies
    # (totals[3], the reads with a sample number out of range, is 0 whenever a host form answers: it refuses such a read)
    assert (totals[:3] > 0).all() and totals[3] == 0 and len(set(entries["sample"].tolist())) == 3 and (entries["label"] == NONE).any(), (where, totals)
    assert (subject_counts > 0).any() and (subject_counts == 0).any()
    with_slack, without = ctx.classify(), ctx.classify(0)
    assert (with_slack[5] > without[5]).any(), where  # slack = 1 lets further subjects in
    taxon, depth = with_slack[3], with_slack[4]
    assert len(set(depth[depth != NONE].tolist())) >= 3 and (taxon == ROOT).any() and (taxon == NONE).any(), where
    assert all((t[[0, 1, 2, 4, 5]] > 0).all() and t[3] == 0 for t in (with_slack[6], without[6])), (where, with_slack[6])
    # ---- subset: a child that kept a dropped row's planes, or lost a kept one's, would show
    keep = ctx.keep()
    old_of_new, rows, pairs, scan_rows = ctx.subset()
    whole = ctx.pairs(D)
    assert not keep[-1] and 0.85 * n < len(old_of_new) < 0.95 * n and len(pairs) >= 500 and len(scan_rows) >= 64
    assert int((~keep[whole["query"]] | ~keep[whole["subject"]]).sum()) >= 100
    assert len(scan_rows) < len(ctx.scan("fixed"))
    # ---- rows: descending, with repeats, the last row at the end
    listed = ctx.listed()[0].astype(np.int64)
    assert listed[-1] == n - 1 and (np.diff(listed[:-1]) <= 0).all() and (np.diff(listed[:-1]) == 0).any() and listed.min() < 7
    assert len(listed) > 200 and ctx.listed()[1].tobytes() == ctx.codes[listed].tobytes()


@pytest.mark.parametrize("name", STORES)
def test_the_kept_list_configs_do_what_they_are_for(name):
    """kept_overflow: half the pairs at D — less than the pairs at D - 2 too, so every keeping call overflows there, before and
    after the growth; kept_alternating: the calls at D overflow, the density call at D - 2 fits, before and after the growth"""
    ctx, grown = context(name), context(name, True)
    assert set(CONFIGS) == {"default", "kept_overflow", "kept_alternating", "small_blocks"} and knobs("default", ctx) == {}
    half = knobs("kept_overflow", ctx)["SMAFA_DENSITY_KEEP_MAX"]
    between = knobs("kept_alternating", ctx)["SMAFA_DENSITY_KEEP_MAX"]
    assert half == len(ctx.pairs(ctx.D)) // 2
    for c in (ctx, grown):
        at_D, below = len(c.pairs(c.D)), len(c.pairs(c.D2))
        assert half < below < at_D and below <= between < at_D, (name, c.grown, half, between, below, at_D)
        kept = {step: len(c.pairs(bound(c))) for step, bound in KEEPING.items()}
        assert [s for s, pairs in kept.items() if pairs <= between] == ["density_lower"] and not [s for s, pairs in kept.items() if pairs <= half]


# ---- the checkers have teeth
def kruskal(n, pairs, weights, D):
    """a minimum spanning forest of (pairs, weights) -> (edges HIT_DTYPE with dist = weight, ordered (w, a, b); level_ends)"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    order = np.lexsort((pairs["subject"], pairs["query"], weights))
    rows = []
    for a, b, w in zip(pairs["query"][order].tolist(), pairs["subject"][order].tolist(), np.asarray(weights)[order].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            rows.append((a, b, w))
    edges = np.array(rows, dtype=np.uint32).reshape(-1, 3).view(HIT_DTYPE).reshape(-1)
    ends = np.array([(edges["dist"] <= t).sum() for t in range(D + 1)], dtype=np.uint64)
    return edges, ends


def forest_of(ctx):
    pairs = ctx.pairs(ctx.D)
    return kruskal(ctx.n, pairs, pairs["dist"].astype(np.int64), ctx.D)


def model_answer(name, ctx):
    """what a correct library returns for the step, made of brute force"""
    D, D2 = ctx.D, ctx.D2
    cp = lambda *xs: tuple(x.copy() if isinstance(x, np.ndarray) else x for x in xs)  # noqa: E731
    if name == "pairs":
        return ctx.pairs(D).copy()
    if name == "pairs_count_only":
        return _lib.ERR_CAPACITY, len(ctx.pairs(D))
    if name in ("components", "components_update"):
        return ctx.labels().copy(), n_components(ctx.labels())
    if name == "levels":
        labels, counts = ctx.levels()
        return labels.copy(), list(counts)
    if name == "density":
        labels, degrees, counts = ctx.density(D, M_HI)
        return labels.copy(), degrees.copy(), dict(counts)
    if name == "density_lower":
        labels, _, counts = ctx.density(D2, M_LO)
        return labels.copy(), None, dict(counts)
    if name in ("peaks_r0", "peaks_r1"):
        return cp(*ctx.peaks(int(name[-1])))
    if name in ("neighbours", "neighbours_k3"):
        return cp(*ctx.neighbours(None if name == "neighbours" else CUT))
    if name == "forest":
        return forest_of(ctx)
    if name == "reach_forest":
        cores, pairs, w = weighted_pairs(ctx.codes, D, REACH_M)
        return kruskal(ctx.n, pairs, w, D) + (cores.copy(),)
    if name in SCANS:
        return ctx.scan({"scan_fixed": "fixed", "scan_k5": "k", "scan_best": "best"}[name]).copy()
    if name == "build_index":
        if ctx.L > INDEX_MAX_COLUMNS:
            return SmafaError(_lib.ERR_INVALID, "the block index takes rows of up to 128 columns (this store: %d)" % ctx.L)
        return {"max_div_served": D, "current": 1}
    if name in ("stable", "stable_hi"):
        labels, joined, count, cores = ctx.stable(REACH_M if name == "stable" else M_HI)
        return labels.copy(), count, joined.copy(), cores.copy()  # (the order SubjectStore.self_stable_clusters returns them in)
    if name == "consensus":
        return cp(*ctx.consensus())
    if name in ("chimeras", "chimeras_weights"):
        return cp(*ctx.chimeras(name == "chimeras_weights"))
    if name == "table":
        return cp(*ctx.table())
    if name == "classify":
        return cp(*ctx.classify())
    if name == "subset":
        return cp(*ctx.subset())
    if name == "rows":
        return ctx.codes.copy(), ctx.listed()[1].copy(), []
    assert name == "pairs_since", name
    return ctx.since().copy()


def edit(answer, part, how):
    """the answer with element `part` of its tuple replaced by how(a copy of it)"""
    parts = list(answer)
    parts[part] = how(parts[part].copy() if isinstance(parts[part], np.ndarray) else parts[part])
    return tuple(parts)


def off_by_one(field=None, at=None):
    def how(a):
        flat = a.reshape(-1)
        i = len(flat) // 2 if at is None else at
        cell = flat[field] if field else flat
        cell[i] = cell[i] - 1 if cell[i] == np.iinfo(cell.dtype).max else cell[i] + 1  # (NONE: one down)
        return a
    return how


def swap_two_neighbours(answer):
    offsets, nb, ds = (x.copy() for x in answer)
    i = int(np.flatnonzero(np.diff(offsets.astype(np.int64)) >= 2)[0])  # the first list of two entries or more
    a = int(offsets[i])
    nb[a], nb[a + 1] = nb[a + 1], nb[a]
    return offsets, nb, ds


def wrong_answers(name, answer):
    """[(what is off, the answer with that one thing off)]"""
    if name in ("pairs", "pairs_since") or name in SCANS:
        return [("one dist", off_by_one("dist")(answer.copy())), ("one subject", off_by_one("subject")(answer.copy())),
                ("the last row missing", answer[:-1].copy()), ("two rows swapped", np.concatenate([answer[1:2], answer[:1], answer[2:]]))]
    if name == "pairs_count_only":
        return [("the count", (answer[0], answer[1] + 1)), ("the code", (_lib.OK, answer[1]))]
    if name in ("components", "components_update"):
        return [("one label", edit(answer, 0, off_by_one())), ("the count", (answer[0], answer[1] + 1))]
    if name == "levels":
        return [("one label of one level", edit(answer, 0, off_by_one())), ("one count", (answer[0], [answer[1][0] + 1] + answer[1][1:]))]
    if name == "density":
        return [("one label", edit(answer, 0, off_by_one())), ("one degree", edit(answer, 1, off_by_one())),
                ("the noise count", (answer[0], answer[1], dict(answer[2], noise=answer[2]["noise"] + 1)))]
    if name == "density_lower":
        return [("one label", edit(answer, 0, off_by_one())), ("degrees given", (answer[0], np.zeros(len(answer[0]), np.uint32), answer[2]))]
    if name in ("peaks_r0", "peaks_r1"):
        return [("one label", edit(answer, 0, off_by_one())), ("one parent", edit(answer, 1, off_by_one())),
                ("one weight", edit(answer, 2, off_by_one())), ("the count", answer[:3] + (answer[3] + 1,))]
    if name in ("neighbours", "neighbours_k3"):
        return [("two neighbours swapped", swap_two_neighbours(answer)), ("one dist", edit(answer, 2, off_by_one())),
                ("one offset", edit(answer, 0, off_by_one()))]
    if name == "forest":
        edges, ends = answer
        light = int(np.flatnonzero(edges["dist"] < edges["dist"].max())[-1])  # the last edge of a class below the top one
        return [("one edge weight", (off_by_one("dist", light)(edges.copy()), ends)), ("one edge missing", (edges[:-1].copy(), ends)),
                ("one level end", (edges, off_by_one(at=0)(ends.copy()))),
                ("one edge twice", (np.concatenate([edges[:1], edges[:-1]]), ends))]
    if name == "reach_forest":
        edges, ends, cores = answer
        finite = int(np.flatnonzero(cores != NONE)[0])
        return [("one core", (edges, ends, off_by_one(at=finite)(cores.copy()))), ("one edge weight", (off_by_one("dist", 0)(edges.copy()), ends, cores)),
                ("one edge missing", (edges[:-1].copy(), ends, cores))]
    if name in ("stable", "stable_hi"):
        core = int(np.flatnonzero(answer[3] != NONE)[0])
        return [("one label", edit(answer, 0, off_by_one())), ("one joined level", edit(answer, 2, off_by_one())),
                ("one core", edit(answer, 3, off_by_one(at=core))), ("the cluster count", (answer[0], answer[1] + 1) + answer[2:])]
    if name == "consensus":
        worst = int(np.where(answer[4] == NONE, 0, answer[4]).argmax())  # a row that sets its cluster's max_div
        return [("one consensus letter", edit(answer, 2, off_by_one())), ("one size", edit(answer, 1, off_by_one())),
                ("one nearest", edit(answer, 3, off_by_one())), ("one max_div", edit(answer, 4, off_by_one(at=worst)))]
    if name in ("chimeras", "chimeras_weights"):
        return [("one flag", edit(answer, 0, off_by_one())), ("one parent", edit(answer, 1, off_by_one())), ("one length", edit(answer, 2, off_by_one())),
                ("one parent on the other side", edit(answer, 3, off_by_one())), ("one weight", edit(answer, 5, off_by_one())),
                ("the count", tuple(answer[:6]) + (answer[6] + 1,))]
    if name == "table":
        return [("one subject", edit(answer, 1, off_by_one())), ("one dist", edit(answer, 2, off_by_one())),
                ("one entry count", edit(answer, 0, off_by_one("count"))), ("one entry missing", (answer[0][:-1].copy(),) + tuple(answer[1:])),
                ("one subject count", edit(answer, 3, off_by_one())), ("one total", edit(answer, 4, off_by_one()))]
    if name == "classify":
        return [("one taxon", edit(answer, 3, off_by_one())), ("one depth", edit(answer, 4, off_by_one())), ("one ties", edit(answer, 5, off_by_one())),
                ("one entry", edit(answer, 0, off_by_one("label"))), ("one total", edit(answer, 6, off_by_one()))]
    if name == "subset":
        return [("one old_of_new entry", edit(answer, 0, off_by_one())), ("one row byte", edit(answer, 1, off_by_one())),
                ("one pair", edit(answer, 2, off_by_one("subject"))), ("one scan row", edit(answer, 3, off_by_one("dist"))),
                ("the last kept row missing", (answer[0][:-1].copy(), answer[1][:-1].copy()) + tuple(answer[2:]))]
    if name == "rows":
        return [("one byte", edit(answer, 0, off_by_one())), ("one byte of a listed row", edit(answer, 1, off_by_one(at=answer[1].size - 1)))]
    assert name == "build_index", name
    return [("no answer", None), ("the other kind of answer", {"max_div_served": 5} if isinstance(answer, Exception) else SmafaError(_lib.ERR_INVALID, "columns"))]


# how many kinds of wrong answer each newer step is fed, at the least
WRONG_AT_LEAST = {"stable": 4, "stable_hi": 4, "consensus": 4, "chimeras": 5, "chimeras_weights": 5, "table": 5, "classify": 4, "subset": 4, "rows": 1}


@pytest.mark.parametrize("name", STORES)
def test_every_checker_refuses_one_wrong_element(name):
    """a checker that accepts a wrong answer is the first way the sequence test could be worthless"""
    for grown in (False, True):
        ctx = context(name, grown)
        for step in (STAGE_B if grown else STAGE_A) + ("stable_hi",):
            answer = model_answer(step, ctx)
            STEPS[step].check(answer, ctx)  # (the model's answer itself is accepted)
            wrong = wrong_answers(step, answer)
            assert wrong and len(wrong) >= WRONG_AT_LEAST.get(step, 1), (step, len(wrong))
            for what, bad in wrong:
                with pytest.raises(AssertionError):
                    STEPS[step].check(bad, ctx)
                    pytest.fail("%s, %s%s: the checker accepted an answer with %s off" % (step, name, " grown" if grown else "", what))


def test_kernel_lists_are_held_to_the_verb():
    join_head = ["smafa::scan_kernel<2,1>", "smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel"]
    delta_head = ["smafa::scan_kernel<2,1>", "smafa_dl::gather_records_kernel", "smafa_join::inverse_order_kernel"]
    mine = {"pairs": ["smafa_join::join_filter_kernel"],
            "components": ["smafa_cc::init_labels_kernel", "smafa_cc::link_rows_kernel", "smafa_cc::flatten_labels_kernel"],
            "levels": ["smafa_lv::init_levels_kernel", "smafa_lv::hook_levels_kernel", "smafa_lv::flatten_levels_kernel"],
            "density": ["smafa_dn::init_density_kernel", "smafa_dn::count_keep_kernel", "smafa_dn::link_cores_kernel", "smafa_dn::flatten_density_kernel"],
            "peaks": ["smafa_pk::init_peaks_kernel", "smafa_pk::weigh_keep_kernel", "smafa_pk::climb_kernel", "smafa_pk::settle_kernel", "smafa_pk::jump_kernel"],
            "neighbours": ["smafa_nb::mirror_pack_kernel", "smafa_nb::row_bounds_kernel", "smafa_nb::cut_degrees_kernel", "smafa_nb::emit_kernel"],
            "forest": ["smafa_sf::init_forest_kernel", "smafa_sf::keep_pairs_kernel", "smafa_sf::span_edges_kernel"],
            "reach_forest": ["smafa_sf::init_forest_kernel", "smafa_mr::tally_keep_kernel", "smafa_mr::core_dist_kernel", "smafa_mr::span_reach_kernel"],
            "pairs_since": ["smafa_dl::delta_filter_kernel"],
            "components_update": ["smafa_dl::seed_parents_kernel", "smafa_cc::link_rows_kernel", "smafa_cc::flatten_labels_kernel"],
            # the lists of the seven newer verbs' own kernel-name tests
            "stable": ["smafa_sf::init_forest_kernel", "smafa_mr::tally_keep_kernel", "smafa_mr::core_dist_kernel", "smafa_mr::span_reach_kernel",
                       "smafa_st::unite_class_kernel", "smafa_st::snapshot_kernel", "smafa_st::census_kernel", "smafa_st::adopt_kernel",
                       "smafa_st::excess_kernel", "smafa_st::choose_kernel", "smafa_st::assign_kernel"],
            "chimeras": ["smafa_pk::init_peaks_kernel", "smafa_pk::weigh_keep_kernel", "chimera::init_sides_kernel", "chimera::offer_sides_kernel",
                         "chimera::verdict_kernel"],
            "consensus": ["consensus::mark_groups_kernel", "consensus::group_ids_kernel", "consensus::group_keys_kernel",
                          "consensus::segment_bounds_kernel", "consensus::tally_vote_kernel<5>", "consensus::measure_kernel",
                          "consensus::finish_groups_kernel"],
            "table": ["assign::init_kernel", "assign::best_kernel", "assign::bin_kernel", "assign::heads_kernel", "assign::fold_kernel"],
            "classify": ["classify::start_kernel", "assign::best_kernel", "classify::agree_kernel", "classify::key_kernel", "assign::heads_kernel",
                         "assign::fold_kernel"],
            "subset": ["subset::keep_flags_kernel", "subset::run_ends_kernel", "subset::move_rows_kernel"],
            "rows": ["subset::unpack_rows_kernel<2>"]}
    assert set(mine) == set(OWN_KERNELS)
    heads = {"consensus": [], "table": join_head[:1], "classify": join_head[:1], "subset": ["smafa::zone_kernel"], "rows": [INVERSE]}
    for verb, own in mine.items():
        scans = heads[verb] if verb in heads else delta_head if verb in DELTA else join_head  # what the call launches in front of its own
        check_kernels(verb, scans + own)
        if verb in heads:  # what the five verbs outside the join may not launch of the scans and the join's own
            for k in ("smafa::scan_kernel<2,1>", "smafa::zone_kernel", "smafa_join::store_records_kernel", INVERSE):
                if not k.startswith(SHARED_KERNELS[verb] or ("-",)):
                    with pytest.raises(AssertionError):
                        check_kernels(verb, scans + own + [k])
        for other, theirs in mine.items():  # the list another verb left behind, and one stray kernel of another verb
            if other != verb:
                with pytest.raises(AssertionError):
                    check_kernels(verb, scans + theirs)
            stray = [k for k in theirs if k not in own and not k.startswith(OWN_KERNELS[verb][0] or ("-",))]
            if stray:
                with pytest.raises(AssertionError):
                    check_kernels(verb, scans + own + stray[:1])
        with pytest.raises(AssertionError):
            check_kernels(verb, scans + own + ["somewhere::else_kernel"])

"""CPU model of the sequence tests (tests/sequence_cases.py, run on the device by tests/test_gpu_sequence.py): the walk has
every ordered pair of steps exactly once, every store gives every step an answer worth checking, and every checker refuses an
answer with one element off.

The answers the checkers are fed are made here from brute force — for the two forests by a plain Kruskal over the brute-force
pairs — never by the library: this file passes without a GPU."""
import collections

import numpy as np
import pytest

from smafa_amd import HIT_DTYPE, SmafaError, _lib
from components_cases import n_components
from delta_cases import has_both_kinds
from density_cases import kinds
from peaks_cases import moved_and_multi_step
from reach_cases import NONE, weighted_pairs
from sequence_cases import (CONFIGS, CUT, DELTA, INDEX_MAX_COLUMNS, KEEPING, M_HI, M_LO, OWN_KERNELS, REACH_M, SCANS, STAGE_A, STAGE_B, STAGE_B_SCANS, STEPS, STORES,
                            check_kernels, circuit, closed, consecutive_pairs, context, knobs)


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
    assert len(STAGE_A) == 16 and len(STAGE_B) == 10 and set(DELTA) <= set(STAGE_B) and not set(DELTA) & set(STAGE_A)
    assert set(STAGE_A) | set(STAGE_B) == set(STEPS)
    verbs = {STEPS[n].verb for n in STAGE_B}
    assert verbs == set(OWN_KERNELS) and len(verbs) == 10  # one step per self-join consumer
    assert {STEPS[n].verb for n in STAGE_A} == set(OWN_KERNELS) - {"pairs_since", "components_update"} | {None}
    # each scan once directly behind components_update and once directly behind neighbours
    assert sorted(consecutive_pairs(list(STAGE_B_SCANS))[::2]) == sorted((a, s) for a in ("components_update", "neighbours") for s in SCANS)
    assert set(KEEPING) == {n for n in STEPS if STEPS[n].verb in ("density", "peaks", "forest", "reach_forest")}


# ---- the stores
@pytest.mark.parametrize("name", STORES)
def test_every_step_has_an_answer_worth_checking(name):
    for grown in (False, True):
        ctx = context(name, grown)
        n, D, D2 = ctx.n, ctx.D, ctx.D2
        assert n == {False: {"nt60": 3020, "aa60": 3020}.get(name, 1020), True: {"nt60": 3566, "aa60": 3566}.get(name, 1566)}[grown]
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
        if grown:
            assert ctx.first_row == context(name).n and has_both_kinds(ctx.since(), ctx.first_row, D)
            # the update has work to do: new rows that join a set of old rows, and new rows that make sets of their own
            new = ctx.labels()[ctx.first_row:]
            assert (new < ctx.first_row).any() and (new >= ctx.first_row).any() and ctx.labels()[: ctx.first_row].tobytes() == ctx.old_labels().tobytes()


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
    assert name == "build_index", name
    return [("no answer", None), ("the other kind of answer", {"max_div_served": 5} if isinstance(answer, Exception) else SmafaError(_lib.ERR_INVALID, "columns"))]


@pytest.mark.parametrize("name", STORES)
def test_every_checker_refuses_one_wrong_element(name):
    """a checker that accepts a wrong answer is the first way the sequence test could be worthless"""
    for grown in (False, True):
        ctx = context(name, grown)
        for step in (STAGE_B if grown else STAGE_A):
            answer = model_answer(step, ctx)
            STEPS[step].check(answer, ctx)  # (the model's answer itself is accepted)
            wrong = wrong_answers(step, answer)
            assert wrong
            for what, bad in wrong:
                with pytest.raises(AssertionError):
                    STEPS[step].check(bad, ctx)
                    pytest.fail("%s, %s%s: the checker accepted an answer with %s off" % (step, name, " grown" if grown else "", what))


def test_kernel_lists_are_held_to_the_verb():
    scans = ["smafa::scan_kernel<2,1>", "smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel"]
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
            "components_update": ["smafa_dl::seed_parents_kernel", "smafa_cc::link_rows_kernel", "smafa_cc::flatten_labels_kernel"]}
    assert set(mine) == set(OWN_KERNELS)
    for verb, own in mine.items():
        scans = delta_head if verb in DELTA else scans[:1] + ["smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel"]
        check_kernels(verb, scans + own)
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

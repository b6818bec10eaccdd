"""Every kind of call of a resident store, interleaved on ONE handle (tests/sequence_cases.py): twenty kinds of call share the
handle's device buffers and host flags — J.parent in its many layouts (the read tables carve it into best[] and their word arrays
and trim it on their way out), the words of J.ctl, the kept pair list, the entry list, pos_of[], the scratch list, the sort
buffers, the block index — and each per-verb test calls one verb on a handle of its own.  Here a handle is walked so that every
step follows every step, itself included, exactly once (circuit): stage A over the 24 steps a fresh store has (576 ordered pairs,
577 steps run); and, on a second handle that has answered a few calls, an append that makes pos_of[] and the block index stale,
then stage B over the 17 verbs, the two delta calls among them (289 ordered pairs, 290 steps run), and the scans behind the three
calls that leave the largest buffers or trim them, and the stable clusters at the other min_pts behind and in front of the reach
forest (STAGE_B_MIN_PTS).
The subset step makes, asks and destroys a child store; the step behind it proves that the walked handle is as it was.  Every
answer is held against brute force as it is produced, and a failure says which step behind which, and whether a fresh handle
gives the same step the right answer.  Besides the answers the walk holds every call to its own kernels, and pos_of[] to its
rule: built at most once per state of the store, by the first call that needs it — the rows call included — and never by a read
table.

Expected answers never come from the code under test, nor from another handle (tests/test_sequence_model.py holds the
checkers to that on the CPU)."""
import ctypes as C
import time

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib
from sequence_cases import (CONFIGS, DELTA, INVERSE, JOINING, KEEPING, KNOBS, N_SAMPLES, POSITIONED, RANKS, STAGE_A, STAGE_B, STAGE_B_MIN_PTS, STAGE_B_SCANS, STEPS, STORES,
                            check_kernels, circuit, closed, consecutive_pairs, context, knobs)

pytestmark = pytest.mark.gpu


def set_knobs(monkeypatch, env):
    for var in KNOBS:
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, str(value))  # (stays set for the test: a fresh handle made on a failure sees the same)


def new_store(ctx):
    return smafa_amd.SubjectStore(ctx.L, smafa_amd.ALPHABET_AA if ctx.kind == "aa" else smafa_amd.ALPHABET_NT)


def run_step(store, name, ctx, state=None):
    """state: {"positions": some earlier call of this state of the store has built pos_of[]} — the walk's; None: not followed"""
    step = STEPS[name]
    rows = len(store)
    answer = step.call(store, ctx)
    step.check(answer, ctx)
    if step.verb:
        calls = [store.last_call_kernels()]
        if step.verb == "rows":  # two calls: the first one's kernels came with the answer
            calls.insert(0, answer[2])
        for kernels in calls:
            check_kernels(step.verb, kernels)
        built = sum(INVERSE in kernels for kernels in calls)
        assert built <= 1 and (step.verb != "rows" or INVERSE not in calls[1]), calls
        if state is not None:
            # pos_of[] is built once per state of the store, by the first call that needs it and by no call that does not
            assert not (built and state["positions"]), "%s built pos_of[] again: %s" % (name, calls)
            if step.verb in POSITIONED:
                assert built or state["positions"], "%s ran without building pos_of[]: %s" % (name, calls)
                state["positions"] = True
            else:
                assert not built, "%s built pos_of[]: %s" % (name, calls)
    assert len(store) == rows == ctx.n, "the call changed the store: %d rows, %d before it" % (len(store), rows)


def on_a_fresh_handle(name, ctx):
    """the one step on a handle of its own over the same rows, under the same environment: is the failure the state's?"""
    store = new_store(ctx)
    try:
        store.push(ctx.codes)
        run_step(store, name, ctx)
        return "fresh handle: passes"
    except (AssertionError, smafa_amd.SmafaError) as e:
        return "fresh handle: fails too (%s)" % str(e)[:200]
    finally:
        store.close()


def walk(store, steps, ctx, config, before, done, log, state):
    """runs `steps` on the handle, each held against brute force; -> the last step.  log: (step, scans of the call)"""
    for name in steps:
        where = "step %d, %s after %s, store %s%s, config %s" % (done + len(log), name, before, ctx.name, " grown" if ctx.grown else "", config)
        try:
            run_step(store, name, ctx, state)
        except (AssertionError, smafa_amd.SmafaError) as e:
            raise AssertionError("%s: %s; %s" % (where, e, on_a_fresh_handle(name, ctx))) from e
        log.append((name, store.last_call_stats()["scans"]))
        before = name
    return before


def kept_paths(log, ctx, keep_max):
    """-> (keeping calls that joined once, that joined again), each held to what the capacity says: a call whose pairs fit the
    kept list scans as often as the components call of the same handle and store, one whose pairs do not at least twice as often"""
    once = {scans for name, scans in log if name == "components"}
    assert len(once) == 1, once
    once = once.pop()
    fast = slow = 0
    for name, scans in log:
        if name in KEEPING:
            fits = len(ctx.pairs(KEEPING[name](ctx))) <= keep_max
            assert (scans == once) if fits else (scans >= 2 * once), (name, scans, once, fits)
            fast, slow = fast + fits, slow + (not fits)
    return fast, slow


def held_to_the_kept_list(name, config, stage, log, ctx, env):
    """the keeping calls of one stage, each held to what the capacity says of it (kept_paths)"""
    if "SMAFA_DENSITY_KEEP_MAX" not in env:
        return
    fast, slow = kept_paths(log, ctx, env["SMAFA_DENSITY_KEEP_MAX"])
    print("%s, %s, stage %s: kept list of %d rows: %d keeping calls joined once, %d joined again" % (name, config, stage, env["SMAFA_DENSITY_KEEP_MAX"], fast, slow))
    assert slow, "the kept list never overflowed"
    if config == "kept_alternating":
        assert fast, "the kept list never held every pair"


# The walk is two tests, each on a handle of its own: with the seven newer verbs in it one handle's walk took more than its share
# of the suite's time at the widest store (profiles/r31_sequence_walk.txt).  Neither circuit is thinned.
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", STORES)
def test_every_call_after_every_call(name, config, monkeypatch):
    """stage A: the 24 steps of a store as pushed, 576 ordered pairs"""
    ctx = context(name)
    env = knobs(config, ctx)
    set_knobs(monkeypatch, env)
    t0 = time.time()
    store = new_store(ctx)
    try:
        store.push(ctx.codes)
        steps_a, log_a, state = closed(circuit(STAGE_A)), [], {"positions": False}
        walk(store, steps_a, ctx, config, "push", 0, log_a, state)
        assert state["positions"]
    finally:
        store.close()
    pairs_a = set(consecutive_pairs(steps_a))
    print("%s, %s: %d steps in %.1f s; stage A %d steps, %d distinct consecutive pairs" % (name, config, len(log_a), time.time() - t0, len(steps_a), len(pairs_a)))
    assert len(pairs_a) == len(STAGE_A) ** 2 == len(steps_a) - 1 == 576
    held_to_the_kept_list(name, config, "A", log_a, ctx, env)
    if config == "small_blocks":  # 3 209 rows in blocks of 192: many scans per join
        assert min(scans for step, scans in log_a if STEPS[step].verb in JOINING) >= ctx.n // 192, log_a[:20]


# what the handle of stage B has served before it grows: an index, pos_of[] and the rows call's inverse table, a kept list, the read
# tables' carving of J.parent — all made for the store as pushed, all stale or trimmed when the growth arrives
BEFORE_THE_GROWTH = ("build_index", "pairs", "rows", "chimeras", "table", "scan_fixed")


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", STORES)
def test_every_call_after_every_call_of_a_grown_store(name, config, monkeypatch):
    """stage B: a handle that has answered calls, then an append that makes pos_of[] and the block index stale, then the 17 verbs
    of the grown store, 289 ordered pairs, and the scans behind the three calls that leave the largest buffers or trim them"""
    ctx, grown = context(name), context(name, True)
    env = knobs(config, ctx)
    set_knobs(monkeypatch, env)
    t0 = time.time()
    store = new_store(ctx)
    try:
        store.push(ctx.codes)
        log_a, state = [], {"positions": False}
        last = walk(store, list(BEFORE_THE_GROWTH), ctx, config, "push", 0, log_a, state)
        assert state["positions"]
        # ---- growth: every expectation now is the grown store's; pos_of[] and the index are stale
        store.push(ctx.growth)
        state["positions"] = False
        assert len(store) == grown.n and grown.first_row == ctx.n
        # ---- stage B
        steps_b, log_b = closed(circuit(STAGE_B)), []
        last = walk(store, steps_b, grown, config, "push after " + last, len(log_a), log_b, state)
        scans_b = list(STAGE_B_SCANS)
        last = walk(store, scans_b, grown, config, last, len(log_a), log_b, state)
        last = walk(store, list(STAGE_B_MIN_PTS), grown, config, last, len(log_a), log_b, state)
        walk(store, ["pairs"], grown, config, last, len(log_a), log_b, state)  # after everything: the plain join, bytes
    finally:
        store.close()
    pairs_b = set(consecutive_pairs(steps_b))
    print("%s, %s: %d steps in %.1f s; %d steps before the growth; stage B %d + %d steps, %d distinct consecutive pairs"
          % (name, config, len(log_a) + len(log_b), time.time() - t0, len(log_a), len(steps_b), len(scans_b) + len(STAGE_B_MIN_PTS) + 1, len(pairs_b)))
    assert len(pairs_b) == len(STAGE_B) ** 2 == len(steps_b) - 1 == 289
    held_to_the_kept_list(name, config, "B", log_b, grown, env)
    if config == "small_blocks":  # blocks of 192: a join of the grown store scans it many times, a delta join the new rows
        joins = [(step, scans) for step, scans in log_b if STEPS[step].verb in JOINING]
        assert min(scans for step, scans in joins if step not in DELTA) >= grown.n // 192, log_b[:20]
        assert min(scans for step, scans in joins if step in DELTA) >= (grown.n - grown.first_row) // 192, log_b[:20]


# ---- calls the ABI refuses, between valid calls
def refused_calls(store, ctx):
    """[(what, call -> code[, the code])]: every call include/smafa_amd.h documents as SMAFA_ERR_INVALID for a live handle of n
    rows — or, where a third element says so, as another code.  (A bound of 2^31 and min_pts = 0 are no errors there: the one
    refused bound is SMAFA_NONE, and min_pts <= 1 makes every row core.)  The cases of the seven newer entry points are the ones
    their tests/test_*_abi.py list: no bound, NULL outputs, short capacities, arguments out of range."""
    l, h, n, D, NONE = _lib.lib(), store._h, ctx.n, ctx.D, _lib.NONE
    u32 = np.zeros((D + 1) * n, dtype=np.uint32)
    u32b, u32c = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    rows = np.zeros(n, dtype=smafa_amd.HIT_DTYPE)
    u64 = np.zeros(n + 1, dtype=np.uint64)
    cnt = (C.c_uint64 * (D + 1))()
    bad_labels = np.arange(n, dtype=np.uint32)
    bad_labels[0] = 1  # a label above its row's number
    p = lambda a: a.ctypes.data  # noqa: E731
    # ---- the seven newer entry points
    L = ctx.L
    reads, samples, weights = ctx.reads()
    m = len(reads)
    in_range, samples = samples, samples.copy()
    samples[5] = N_SAMPLES  # one read with a sample number that is out of range
    lineage = np.ascontiguousarray(ctx.lineage())
    root_inside, id_behind_none = lineage.copy(), lineage.copy()
    root_inside[3, 2] = 0xFFFFFFFE
    id_behind_none[3] = [1, NONE, NONE, NONE, 4, NONE, NONE]
    bad_read = reads.copy()
    bad_read[3, 3] = 28
    labels = np.ascontiguousarray(ctx.consensus_labels())
    label_too_large = labels.copy()
    label_too_large[n // 2] = n
    u8 = np.zeros((n, L), dtype=np.uint8)
    per_read = [np.zeros(m, dtype=np.uint32) for _ in range(5)]
    entries, totals, counts = np.zeros(m, dtype=smafa_amd.TABLE_DTYPE), np.zeros(6, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    six = [np.zeros(n, dtype=np.uint32) for _ in range(6)]
    keep = np.ascontiguousarray(ctx.keep(), dtype=np.uint32)
    listed = np.array([0, n, 1], dtype=np.uint32)
    out = C.c_void_p()

    def chimeras(D_, radius, fold, arrays=six, cap=n, count=cnt, given=None):
        return l.smafa_db_self_chimeras(h, D_, radius, fold, given, *(p(a) if a is not None else None for a in arrays), cap, count)

    def assign(q=reads, D_=D, s_=in_range, n_samples=N_SAMPLES, e=entries, cap=m, t=totals):
        return l.smafa_db_assign(h, p(q) if q is not None else None, m, D_, p(labels), p(s_), n_samples, p(weights), p(per_read[0]), p(per_read[1]),
                                 p(counts), p(e) if e is not None else None, cap, p(t) if t is not None else None)

    def classify(q=reads, D_=D, tax=lineage, ranks=RANKS, s_=in_range, n_samples=N_SAMPLES, e=entries, cap=m, t=totals):
        return l.smafa_db_classify(h, p(q) if q is not None else None, m, D_, 1, p(tax) if tax is not None else None, ranks, p(s_), n_samples,
                                   p(weights), *(p(a) for a in per_read), p(e) if e is not None else None, cap, p(t) if t is not None else None)

    def subset(k=keep, o=out, old=u32b, cap=n, kept=cnt):
        rc = l.smafa_db_subset(h, p(k) if k is not None else None, 0, C.byref(o) if o is not None else None, p(old), cap, kept)
        assert o is None or not o.value, "a refused subset call left a handle behind"
        return rc

    newer = [
        ("stable, no bound", lambda: l.smafa_db_self_stable(h, NONE, 3, 0, p(u32), p(u32b), p(u32c), n, cnt)),
        ("stable, NULL labels", lambda: l.smafa_db_self_stable(h, D, 3, 0, None, p(u32b), p(u32c), n, cnt)),
        ("stable, NULL n_clusters", lambda: l.smafa_db_self_stable(h, D, 3, 0, p(u32), p(u32b), p(u32c), n, None)),
        ("stable, cap < n", lambda: l.smafa_db_self_stable(h, D, 3, 0, p(u32), p(u32b), p(u32c), n - 1, cnt)),
        ("consensus, NULL labels", lambda: l.smafa_db_consensus(h, None, p(u32), p(u32b), p(u8), p(u32c), p(six[0]), n, cnt)),
        ("consensus, NULL n_clusters", lambda: l.smafa_db_consensus(h, p(labels), p(u32), p(u32b), p(u8), p(u32c), p(six[0]), n, None)),
        ("consensus, NULL ids with a capacity", lambda: l.smafa_db_consensus(h, p(labels), None, p(u32b), p(u8), p(u32c), p(six[0]), n, cnt)),
        ("consensus, NULL sizes with a capacity", lambda: l.smafa_db_consensus(h, p(labels), p(u32), None, p(u8), p(u32c), p(six[0]), n, cnt)),
        ("consensus, NULL codes with a capacity", lambda: l.smafa_db_consensus(h, p(labels), p(u32), p(u32b), None, p(u32c), p(six[0]), n, cnt)),
        # (refused on the device, behind the marking pass: it has touched J.parent)
        ("consensus, a label that is no subject", lambda: l.smafa_db_consensus(h, p(label_too_large), p(u32), p(u32b), p(u8), p(u32c), p(six[0]), n, cnt)),
        ("consensus, asked for K", lambda: l.smafa_db_consensus(h, p(labels), None, None, None, None, None, 0, cnt), _lib.ERR_CAPACITY),
        ("chimeras, NULL flags", lambda: chimeras(D, 0, 2, arrays=[None] + six[1:])),
        ("chimeras, NULL n_chimeras", lambda: chimeras(D, 0, 2, count=None)),
        ("chimeras, no bound", lambda: chimeras(NONE, 0, 2)),
        ("chimeras, radius > max_div", lambda: chimeras(D, D + 1, 2)),
        ("chimeras, min_fold 0", lambda: chimeras(D, 0, 0)),
        ("chimeras, cap < n", lambda: chimeras(D, 0, 2, cap=n - 1)),
        ("table, NULL reads", lambda: assign(q=None)),
        ("table, NULL totals", lambda: assign(t=None)),
        ("table, no bound", lambda: assign(D_=NONE)),
        ("table, n_samples 0", lambda: assign(n_samples=0)),
        ("table, NULL entries with a capacity", lambda: assign(e=None)),
        ("table, a sample number out of range", lambda: assign(s_=samples)),
        ("table, a code outside the alphabet", lambda: assign(q=bad_read)),
        ("table, asked for the count", lambda: assign(e=None, cap=0), _lib.ERR_CAPACITY),
        ("classify, NULL reads", lambda: classify(q=None)),
        ("classify, NULL totals", lambda: classify(t=None)),
        ("classify, no bound", lambda: classify(D_=NONE)),
        ("classify, n_samples 0", lambda: classify(n_samples=0)),
        ("classify, NULL entries with a capacity", lambda: classify(e=None)),
        ("classify, n_ranks 0", lambda: classify(ranks=0)),
        ("classify, n_ranks 17", lambda: classify(ranks=17)),
        ("classify, NULL lineage", lambda: classify(tax=None)),
        ("classify, a sample number out of range", lambda: classify(s_=samples)),
        ("classify, a code outside the alphabet", lambda: classify(q=bad_read)),
        ("classify, the root inside a lineage", lambda: classify(tax=root_inside)),
        ("classify, an id behind a NONE", lambda: classify(tax=id_behind_none)),
        ("classify, asked for the count", lambda: classify(e=None, cap=0), _lib.ERR_CAPACITY),
        ("subset, NULL out", lambda: subset(o=None)),
        ("subset, NULL n_kept", lambda: subset(kept=None)),
        ("subset, NULL keep", lambda: subset(k=None)),
        # (refused behind the flags and their sums, once k is known: it has run on the handle's stream)
        ("subset, old_of_new too small", lambda: subset(cap=n // 2), _lib.ERR_CAPACITY),
        ("rows, NULL codes", lambda: l.smafa_db_rows(h, None, 0, n, None)),
        ("rows, a range past the end", lambda: l.smafa_db_rows(h, None, 1, n, p(u8))),
        ("rows, a first row past the end", lambda: l.smafa_db_rows(h, None, n + 1, 1, p(u8))),
        ("rows, a listed number that is no subject", lambda: l.smafa_db_rows(h, p(listed), 0, 3, p(u8))),
    ]
    return newer + [
        ("pairs, no bound", lambda: l.smafa_db_self_hits(h, NONE, p(rows), n, cnt)),
        ("components, no bound", lambda: l.smafa_db_self_components(h, NONE, p(u32), n, cnt)),
        ("components, NULL labels", lambda: l.smafa_db_self_components(h, D, None, n, cnt)),
        ("components, NULL count", lambda: l.smafa_db_self_components(h, D, p(u32), n, None)),
        ("components, cap < n", lambda: l.smafa_db_self_components(h, D, p(u32), n - 1, cnt)),
        ("levels, no bound", lambda: l.smafa_db_self_levels(h, NONE, p(u32), len(u32), cnt)),
        ("levels, NULL labels", lambda: l.smafa_db_self_levels(h, D, None, len(u32), cnt)),
        ("levels, NULL count", lambda: l.smafa_db_self_levels(h, D, p(u32), len(u32), None)),
        ("levels, cap < levels x n", lambda: l.smafa_db_self_levels(h, D, p(u32), len(u32) - 1, cnt)),
        ("forest, no bound", lambda: l.smafa_db_self_forest(h, NONE, p(rows), n, cnt)),
        ("forest, NULL edges", lambda: l.smafa_db_self_forest(h, D, None, n, cnt)),
        ("forest, NULL level_ends", lambda: l.smafa_db_self_forest(h, D, p(rows), n, None)),
        ("forest, cap < n - 1", lambda: l.smafa_db_self_forest(h, D, p(rows), n - 2, cnt)),
        ("reach forest, no bound", lambda: l.smafa_db_self_reach_forest(h, NONE, 3, p(rows), n, cnt, p(u32b))),
        ("reach forest, NULL edges", lambda: l.smafa_db_self_reach_forest(h, D, 3, None, n, cnt, p(u32b))),
        ("reach forest, NULL level_ends", lambda: l.smafa_db_self_reach_forest(h, D, 3, p(rows), n, None, p(u32b))),
        ("reach forest, cap < n - 1", lambda: l.smafa_db_self_reach_forest(h, D, 3, p(rows), n - 2, cnt, p(u32b))),
        ("density, no bound", lambda: l.smafa_db_self_density(h, NONE, 3, p(u32), p(u32b), n, cnt)),
        ("density, NULL labels", lambda: l.smafa_db_self_density(h, D, 3, None, p(u32b), n, cnt)),
        ("density, NULL counts", lambda: l.smafa_db_self_density(h, D, 3, p(u32), p(u32b), n, None)),
        ("density, cap < n", lambda: l.smafa_db_self_density(h, D, 3, p(u32), p(u32b), n - 1, cnt)),
        ("peaks, no bound", lambda: l.smafa_db_self_peaks(h, NONE, 0, p(u32), p(u32b), p(u32c), n, cnt)),
        ("peaks, NULL labels", lambda: l.smafa_db_self_peaks(h, D, 0, None, p(u32b), p(u32c), n, cnt)),
        ("peaks, NULL n_peaks", lambda: l.smafa_db_self_peaks(h, D, 0, p(u32), p(u32b), p(u32c), n, None)),
        ("peaks, radius > max_div", lambda: l.smafa_db_self_peaks(h, D, D + 1, p(u32), p(u32b), p(u32c), n, cnt)),
        ("peaks, cap < n", lambda: l.smafa_db_self_peaks(h, D, 0, p(u32), p(u32b), p(u32c), n - 1, cnt)),
        ("neighbours, no bound", lambda: l.smafa_db_self_neighbours(h, NONE, NONE, p(u64), p(u32), p(u32b), n, cnt)),
        ("neighbours, NULL offsets", lambda: l.smafa_db_self_neighbours(h, D, NONE, None, p(u32), p(u32b), n, cnt)),
        ("neighbours, NULL n_out", lambda: l.smafa_db_self_neighbours(h, D, NONE, p(u64), p(u32), p(u32b), n, None)),
        ("neighbours, NULL neighbours with a capacity", lambda: l.smafa_db_self_neighbours(h, D, NONE, p(u64), None, None, n, cnt)),
        ("neighbours, max_num_hits 0", lambda: l.smafa_db_self_neighbours(h, D, 0, p(u64), p(u32), p(u32b), n, cnt)),
        ("delta pairs, no bound", lambda: l.smafa_db_self_hits_since(h, n // 2, NONE, p(rows), n, cnt)),
        ("delta pairs, NULL count", lambda: l.smafa_db_self_hits_since(h, n // 2, D, p(rows), n, None)),
        ("delta pairs, NULL rows with a capacity", lambda: l.smafa_db_self_hits_since(h, n // 2, D, None, n, cnt)),
        ("delta pairs, first_row > n", lambda: l.smafa_db_self_hits_since(h, n + 1, D, p(rows), n, cnt)),
        ("components update, no bound", lambda: l.smafa_db_self_components_update(h, n // 2, NONE, p(u32), n, cnt)),
        ("components update, NULL labels", lambda: l.smafa_db_self_components_update(h, n // 2, D, None, n, cnt)),
        ("components update, NULL count", lambda: l.smafa_db_self_components_update(h, n // 2, D, p(u32), n, None)),
        ("components update, first_row > n", lambda: l.smafa_db_self_components_update(h, n + 1, D, p(u32), n, cnt)),
        ("components update, cap < n", lambda: l.smafa_db_self_components_update(h, n // 2, D, p(u32), n - 1, cnt)),
        # (refused on the device, behind the seed pass: the one refusal that has touched J.parent and J.ctl)
        ("components update, a label above its row", lambda: l.smafa_db_self_components_update(h, n // 2, D, p(bad_labels), n, cnt)),
    ]


def test_a_refused_call_leaves_the_next_answer_exact(monkeypatch):
    """a failure here is no state bug of the walk above: the aa60 store, the default config, one refused call — or the
    count-only pairs call — between two valid ones"""
    set_knobs(monkeypatch, {})
    ctx = context("aa60")
    following = ("density", "peaks_r0", "reach_forest", "neighbours", "chimeras", "table", "stable", "rows")
    store = new_store(ctx)
    try:
        store.push(ctx.codes)
        refused = refused_calls(store, ctx)
        before = "push"
        for after in following:
            for what, call, *code in refused + [("pairs_count_only", None)]:
                if call is None:
                    run_step(store, "pairs_count_only", ctx)
                else:
                    rc = call()
                    assert rc == (code[0] if code else _lib.ERR_INVALID), "%s after %s: code %d, %s" % (what, before, rc, _lib.lib().smafa_last_error())
                try:
                    run_step(store, after, ctx)
                except (AssertionError, smafa_amd.SmafaError) as e:
                    raise AssertionError("%s after (%s) after %s: %s; %s" % (after, what, before, e, on_a_fresh_handle(after, ctx))) from e
                before = after
    finally:
        store.close()
    print("%d refused calls and the count-only call, each in front of each of %s" % (len(refused), ", ".join(following)))
    assert len(refused) == 41 + 46

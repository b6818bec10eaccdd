"""Every kind of call of a resident store, interleaved on ONE handle (tests/sequence_cases.py): thirteen kinds of call share the
handle's device buffers and host flags — J.parent in six layouts, the words of J.ctl, the kept pair list, the entry list, pos_of[],
the scratch list, the sort buffers — and each per-verb test calls one verb on a handle of its own.  Here a handle is walked so
that every step follows every step, itself included, exactly once (circuit): stage A over the sixteen steps a fresh store
has, then an append that makes pos_of[] and the block index stale, then stage B over the ten self-join consumers, the two delta
calls among them, and the scans behind the two calls that leave the largest buffers.  Every answer is held against brute force
as it is produced, and a failure says which step behind which, and whether a fresh handle gives the same step the right answer.

Expected answers never come from the code under test, nor from another handle (tests/test_sequence_model.py holds the
checkers to that on the CPU)."""
import ctypes as C
import time

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib
from sequence_cases import (CONFIGS, KEEPING, KNOBS, STAGE_A, STAGE_B, STAGE_B_SCANS, STEPS, STORES, check_kernels, circuit, closed, consecutive_pairs,
                            context, knobs)

pytestmark = pytest.mark.gpu


def set_knobs(monkeypatch, env):
    for var in KNOBS:
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, str(value))  # (stays set for the test: a fresh handle made on a failure sees the same)


def new_store(ctx):
    return smafa_amd.SubjectStore(ctx.L, smafa_amd.ALPHABET_AA if ctx.kind == "aa" else smafa_amd.ALPHABET_NT)


def run_step(store, name, ctx):
    step = STEPS[name]
    rows = len(store)
    answer = step.call(store, ctx)
    step.check(answer, ctx)
    if step.verb:
        check_kernels(step.verb, store.last_call_kernels())
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


def walk(store, steps, ctx, config, before, done, log):
    """runs `steps` on the handle, each held against brute force; -> the last step.  log: (step, scans of the call)"""
    for name in steps:
        where = "step %d, %s after %s, store %s%s, config %s" % (done + len(log), name, before, ctx.name, " grown" if ctx.grown else "", config)
        try:
            run_step(store, name, ctx)
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


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", STORES)
def test_every_call_after_every_call(name, config, monkeypatch):
    ctx, grown = context(name), context(name, True)
    env = knobs(config, ctx)
    set_knobs(monkeypatch, env)
    t0 = time.time()
    store = new_store(ctx)
    try:
        # ---- stage A
        store.push(ctx.codes)
        steps_a, log_a = closed(circuit(STAGE_A)), []
        last = walk(store, steps_a, ctx, config, "push", 0, log_a)
        # ---- growth: every expectation now is the grown store's; pos_of[] and the index are stale
        store.push(ctx.growth)
        assert len(store) == grown.n and grown.first_row == ctx.n
        # ---- stage B
        steps_b, log_b = closed(circuit(STAGE_B)), []
        last = walk(store, steps_b, grown, config, "push after " + last, len(log_a), log_b)
        scans_b = list(STAGE_B_SCANS)
        last = walk(store, scans_b, grown, config, last, len(log_a), log_b)
        walk(store, ["pairs"], grown, config, last, len(log_a), log_b)  # after everything: the plain join, bytes
    finally:
        store.close()
    pairs_a, pairs_b = set(consecutive_pairs(steps_a)), set(consecutive_pairs(steps_b))
    print("%s, %s: %d steps in %.1f s; stage A %d steps, %d distinct consecutive pairs; stage B %d + %d steps, %d distinct consecutive pairs"
          % (name, config, len(log_a) + len(log_b), time.time() - t0, len(steps_a), len(pairs_a), len(steps_b), len(scans_b) + 1, len(pairs_b)))
    assert len(pairs_a) == len(STAGE_A) ** 2 == len(steps_a) - 1 and len(pairs_b) == len(STAGE_B) ** 2 == len(steps_b) - 1
    if "SMAFA_DENSITY_KEEP_MAX" in env:
        fast_a, slow_a = kept_paths(log_a, ctx, env["SMAFA_DENSITY_KEEP_MAX"])
        fast_b, slow_b = kept_paths(log_b, grown, env["SMAFA_DENSITY_KEEP_MAX"])
        print("%s, %s: kept list of %d rows: %d keeping calls joined once, %d joined again"
              % (name, config, env["SMAFA_DENSITY_KEEP_MAX"], fast_a + fast_b, slow_a + slow_b))
        assert slow_a and slow_b, "the kept list never overflowed"
        if config == "kept_alternating":
            assert fast_a and fast_b, "the kept list never held every pair"
    if config == "small_blocks":  # 3 020 rows in blocks of 192: many scans per join
        assert min(scans for step, scans in log_a if STEPS[step].verb) >= ctx.n // 192, log_a[:20]


# ---- calls the ABI refuses, between valid calls
def refused_calls(store, ctx):
    """[(what, call -> code)]: every call include/smafa_amd.h documents as SMAFA_ERR_INVALID for a live handle of n rows.  (A
    bound of 2^31 and min_pts = 0 are no errors there: the one refused bound is SMAFA_NONE, and min_pts <= 1 makes every row core.)"""
    l, h, n, D, NONE = _lib.lib(), store._h, ctx.n, ctx.D, _lib.NONE
    u32 = np.zeros((D + 1) * n, dtype=np.uint32)
    u32b, u32c = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    rows = np.zeros(n, dtype=smafa_amd.HIT_DTYPE)
    u64 = np.zeros(n + 1, dtype=np.uint64)
    cnt = (C.c_uint64 * (D + 1))()
    bad_labels = np.arange(n, dtype=np.uint32)
    bad_labels[0] = 1  # a label above its row's number
    p = lambda a: a.ctypes.data  # noqa: E731
    return [
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
    following = ("density", "peaks_r0", "reach_forest", "neighbours")
    store = new_store(ctx)
    try:
        store.push(ctx.codes)
        refused = refused_calls(store, ctx)
        before = "push"
        for after in following:
            for what, call in refused + [("pairs_count_only", None)]:
                if call is None:
                    run_step(store, "pairs_count_only", ctx)
                else:
                    rc = call()
                    assert rc == _lib.ERR_INVALID, "%s after %s: code %d, %s" % (what, before, rc, _lib.lib().smafa_last_error())
                try:
                    run_step(store, after, ctx)
                except (AssertionError, smafa_amd.SmafaError) as e:
                    raise AssertionError("%s after (%s) after %s: %s; %s" % (after, what, before, e, on_a_fresh_handle(after, ctx))) from e
                before = after
    finally:
        store.close()
    print("%d refused calls and the count-only call, each in front of each of %s" % (len(refused), ", ".join(following)))

"""The planted stores of tests/kth_sample_cases.py hold what that module says (CPU, brute force on the code bytes): for every
shape and k the k-th distance of every planted query, its ties on each side of the sample's edge S, the row counts of the
classes, and that no background subject comes within E + 1 of a planted base.  A shape that cannot hold a class fails here —
the builder asserts — and is not skipped on the GPU (tests/test_gpu_kth_sample.py)."""
import numpy as np
import pytest

import kth_sample_cases as cases
from kth_sample_cases import E, KS, SHAPES, WALK_SHAPES, WALK_STEPS


def _distances(subjects, q):
    return (subjects != q[None, :]).sum(axis=1)


def _answer(d, k, bound):
    """(k-th distance or None, rows) of the k mode under a bound, from every subject's distance"""
    within = np.sort(d[d <= bound])
    if len(within) < k:
        return None, len(within)
    return int(within[k - 1]), int((within <= within[k - 1]).sum())


def _check(c):
    k, S, D, L = c.k, c.S, c.D, c.L
    planted = np.zeros(c.n, dtype=bool)
    planted[[p for p, (owner, _) in c.taken.items() if owner != "filler"]] = True
    # a planted subject sits where it was put, d columns from its owner's base, and the fillers' rows were left alone
    for pos, (owner, d) in c.taken.items():
        if owner == "filler":
            assert (c.subjects[pos] == c.background[pos]).all()
        else:
            assert int((c.subjects[pos] != c.queries[owner]).sum()) == d, (pos, owner, d)
    assert (c.subjects[~planted] == c.background[~planted]).all()
    if c.kind == "nt2":
        assert c.subjects.max() == 3
    if c.kind == "nt3":
        assert c.subjects[: cases.FIRST_PART].max() == 3 and (c.subjects[cases.FIRST_PART:] == 4).any()
    seen = []
    for qi, m in enumerate(c.meta):
        if m["cls"] == "filler":
            continue
        seen.append(m["cls"])
        d = _distances(c.subjects, c.queries[qi])
        if m["cls"] != "g":
            near = np.nonzero(~planted & (d <= E + 1))[0]
            assert len(near) == 0, "background subjects %s within E + 1 of the base of query %d (%s)" % (near[:4], qi, m["cls"])
        if m["cls"] in ("d", "e", "twin"):
            assert int(((d <= D + 1) & ~planted).sum()) == 0, (qi, m["cls"])
        kth, rows = _answer(d, k, L)
        if m["kth"] is not None:
            assert (kth, rows) == (m["kth"], m["rows"]), (qi, m, kth, rows)
            if "ties_in" in m:
                ties = np.nonzero(d == kth)[0]
                assert (int((ties < S).sum()), int((ties >= S).sum())) == (m["ties_in"], m["ties_out"]), (qi, m)
        kth_D, rows_D = _answer(d, k, D)
        if m["rows_D"] is not None:
            assert rows_D == m["rows_D"], (qi, m, rows_D)
        if m["cls"] == "c":
            assert tuple(np.nonzero(d <= E)[0]) == tuple(sorted(m["at_E"])) and (d[list(m["at_E"])] == E).all()
        if m["cls"] in ("d", "twin"):
            assert kth_D is None  # fewer than k within the bound: it binds
        if m["cls"] == "e":
            assert kth_D == D
    want = ["a", "b", "c", "d", "e", "f"] + (["g"] if c.kind != "nt3" else []) + ["h", "twin", "a", "b", "h"]
    assert seen == want, seen
    cls = [m["cls"] for m in c.meta]
    assert cls[0] == "a" and cls[32] == "twin" and cls[72:] == ["a", "b", "h"] and len(cls) == 75
    assert not cases.level1_prunes(L, D) and not cases.level1_prunes(L, L)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,L", SHAPES, ids=["%s-%d" % s for s in SHAPES])
def test_planted_structure_of_every_shape(kind, L, k):
    c = cases.case(kind, L, k)
    assert c.n == 10241 and c.S == 5120 and c.n_tiles == 41
    _check(c)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,L", WALK_SHAPES, ids=["%s-%d" % s for s in WALK_SHAPES])
def test_planted_structure_of_the_walk_length_stores(kind, L, k):
    c = cases.walk_case(kind, L, k)
    assert c.n == 40961 and c.S == 20480 and c.n_tiles == 161
    _check(c)
    # the ties of a and b (and h's subjects one past its k-th distance) lie in the tiles of steps 3, 4, 7 and 19 — c's at
    # subject 0 and S - 1 in steps 0 and 19 — and so in tiles of different tile groups when two or three groups share the steps
    for qi, m in enumerate(c.meta):
        d = {"a": E, "b": E, "h": E + 1, "c": E}.get(m["cls"])
        if d is None:
            continue
        steps = c.planted_steps(qi, d)
        assert steps == [0, 19] if m["cls"] == "c" else (len(steps) >= 2 and set(steps) <= set(WALK_STEPS)), (qi, m["cls"], steps)
        for groups in (2, 3):
            assert len({s % groups for s in steps}) >= 2, (qi, m["cls"], steps, groups)


@pytest.mark.parametrize("kind,L", [("aa", 60), ("nt2", 31)])
def test_planted_structure_of_the_two_tile_sample(kind, L):
    """the store of the rule that turns the sample off: planted for k = 40 around S = 512"""
    c = cases.case(kind, L, 40, sample_tiles=2)
    assert c.S == 512
    _check(c)


def test_seed_kernel_names():
    assert cases.seed_kernel("nt2", 31) == "smafa::kth_seed_kernel<2, 3, 1>"
    assert cases.seed_kernel("nt3", 120) == "smafa::kth_seed_kernel<3, 3, 4>"
    assert cases.seed_kernel("aa", 150) == cases.seed_kernel("aa", 255) == "smafa::kth_seed_kernel<0, 0, 0>"
    assert cases.seed_kernel("aa", 256) is None

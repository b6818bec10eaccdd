"""CPU model of the store shapes of tests/self_join_cases.py (SHAPE_TABLE) and of the stores tests/test_gpu_self_join_shapes.py joins.

The record layout is restated here — qrec_stride, bound_slot, qslot of kernels.hip.h, kRecWindow of join.hip.h, and the window
loop of store_records_kernel — and held against the headers' own text, so that a change of the layout fails here and not as a
table that quietly stopped reaching the second window.  Per shape: the record stride, the number of windows, the width of the
last one, and which windows hold a slot of a plane the store keeps.  Per span setting: where the spans start within a wave tile.

The stores themselves are checked too (every distance 0..D occurs, at least one exact copy — shape_case asserts it) and their
expected rows, brute force on the code bytes, are held against oracle.scan_codes on a sample: CPU work, done here once."""
import os
import re

import numpy as np
import pytest

import self_join_cases as cases
from self_join_cases import (NARROW_SHAPES, REC_WINDOW, SHAPE_STORES, SHAPE_TABLE, SPANS_FAMILIES, WIDE_SHAPES, check_against_oracle,
                             join_scans, join_spans, replaned_case, shape_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smafa_amd", "csrc")
WAVE_TILE = 256


# ---- the layout, restated
def round_up4(x):
    return (x + 3) & ~3


def qrec_stride(planes, words):
    return round_up4(planes * words + 1)


def bound_slot(words):
    return words if words < 2 else 2


def qslot(planes, words, p, w):
    if p == 0:  # kFilterPlane: always plane 0
        return w if w < bound_slot(words) else w + 1
    return words + 1 + (p - 1) * words + w


def windows(QS):
    """[(s0, sc)] of store_records_kernel's loop: for (s0 = 0; s0 < QS; s0 += kRecWindow) sc = min(kRecWindow, QS - s0)"""
    return [(s0, min(REC_WINDOW, QS - s0)) for s0 in range(0, QS, REC_WINDOW)]


def stored_windows(PS, PQ, W, QS):
    """the windows that hold a slot of a stored plane (the kernel copies a word iff s0 <= slot < s0 + sc)"""
    slots = {qslot(PQ, W, p, w) for p in range(PS) for w in range(W)}
    return [any(s0 <= s < s0 + sc for s in slots) for s0, sc in windows(QS)]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_the_restated_layout_is_the_headers():
    k = _source("scan_plan.h") + " " + _source("kernels.hip.h")  # (the strides and tile sizes the host shares: scan_plan.h)
    for text in (
        "constexpr int kWaveTile = %d;" % WAVE_TILE,
        "constexpr int round_up4(int x) { return (x + 3) & ~3; }",
        "constexpr int qrec_stride(int planes, int words) { return round_up4(planes * words + 1); }",
        "constexpr int kFilterPlane = 0;",
        "constexpr int bound_slot(int words) { return words < 2 ? words : 2; }",
        "constexpr int qslot(int planes, int words, int p, int w) { return p == 0 ? (w < bound_slot(words) ? w : w + 1) "
        ": words + 1 + (p < 0 ? p : p - 1) * words + w; }",
    ):
        assert text in k, text
    j = _source("join.hip.h")
    for text in (
        "constexpr int kRecWindow = %d;" % REC_WINDOW,
        "for (uint32_t s0 = 0; s0 < QS; s0 += kRecWindow) {",
        "const uint32_t sc = min((uint32_t)kRecWindow, QS - s0), stride = sc | 1u;",
        "if (slot < s0 || slot >= s0 + sc) continue;",
    ):
        assert text in j, text


def test_slots_are_a_layout():
    """every (plane, word) has a slot of its own below QS, and none of them is the bound's"""
    for PQ in (3, 5):
        for W in range(1, 40):
            slots = [qslot(PQ, W, p, w) for p in range(PQ) for w in range(W)]
            assert len(set(slots)) == PQ * W and bound_slot(W) not in slots
            assert sorted(slots + [bound_slot(W)]) == list(range(PQ * W + 1)) and PQ * W + 1 <= qrec_stride(PQ, W)


# name -> (windows, width of the last window)
WINDOWS = {"aa200": (2, 4), "aa224": (2, 4), "aa250": (2, 12), "aa700": (4, 16), "nt330": (2, 4), "nt330n": (2, 4), "nt520": (2, 20)}


@pytest.mark.parametrize("name", list(SHAPE_TABLE))
def test_shape_table(name):
    kind, L, n_frac, PS, PQ, W, QS = SHAPE_TABLE[name]
    assert W == (L + 31) // 32 and QS == qrec_stride(PQ, W)
    assert (PS, PQ) == ((5, 5) if kind == "aa" else (3 if n_frac > 0 else 2, 3))
    win = windows(QS)
    assert sum(sc for _, sc in win) == QS
    if name in WIDE_SHAPES:
        assert (len(win), win[-1][1]) == WINDOWS[name]
        assert win[-1][1] < REC_WINDOW and win[-1][1] % 2 == 0  # a short last window, whose LDS row stride sc | 1 is not sc
        assert W > 4  # scan_wide_kernel / scan_generic_kernel
    else:
        assert len(win) == 1 and name not in WINDOWS
    assert (name in NARROW_SHAPES) == (W <= 4)


def test_every_word_count_of_the_per_length_kernels_is_there():
    assert sorted({SHAPE_TABLE[n][5] for n in NARROW_SHAPES}) == [1, 2, 3, 4]
    assert {(SHAPE_TABLE[n][3], SHAPE_TABLE[n][5]) for n in NARROW_SHAPES} >= {(2, 2), (2, 3), (2, 4), (5, 1), (5, 2), (5, 3), (5, 4)}
    assert set(WINDOWS) == set(WIDE_SHAPES)


def test_the_second_window_of_the_nucleotide_shapes():
    """nt330: the store's two planes end at slot 22 — the second window (slots 32..35) holds words of plane 2 alone and must leave as
    zeros; nt330n keeps that plane; nt520's plane 1 reaches slots 32..34"""
    for name, want in (("nt330", [True, False]), ("nt330n", [True, True]), ("nt520", [True, True])):
        _, _, _, PS, PQ, W, QS = SHAPE_TABLE[name]
        assert stored_windows(PS, PQ, W, QS) == want, name
    assert max(qslot(3, 11, p, w) for p in range(2) for w in range(11)) == 22
    assert sorted(qslot(3, 11, 2, w) for w in range(11) if qslot(3, 11, 2, w) >= 32) == [32, 33]
    assert sorted(s for s in (qslot(3, 17, 1, w) for w in range(17)) if s >= 32) == [32, 33, 34]
    assert min(qslot(3, 17, 2, w) for w in range(17)) == 35  # the rest of nt520's second window: the plane it does not keep
    for name in ("aa200", "aa224", "aa250", "aa700"):
        _, _, _, PS, PQ, W, QS = SHAPE_TABLE[name]
        assert all(stored_windows(PS, PQ, W, QS)), name


def test_spans_off_the_tile_grid():
    """blocks of 192 at stride 3: spans of 576 positions that start 64 and 128 rows into a wave tile, the last one short with
    another S and R; blocks of 64 at stride 5: every block within the few-query kernel's 64 records"""
    n = SPANS_FAMILIES * 10 + 20
    spans = join_spans(n, 192, 3)
    assert spans == [(0, 576, 3, 192), (576, 576, 3, 192), (1152, 368, 2, 184)]
    assert [p0 % WAVE_TILE for p0, _, _, _ in spans] == [0, 64, 128] and join_scans(n, 192, 3) == 8
    assert all((p0 + m) % WAVE_TILE for p0, m, _, _ in spans)  # ... and end inside one
    few = join_spans(n, 64, 5)
    assert [p0 % WAVE_TILE for p0, _, _, _ in few] == [0, 64, 128, 192, 0] and few[-1] == (1280, 240, 4, 60)
    assert all(R <= 64 for _, _, _, R in few) and join_scans(n, 64, 5) == 24
    big = join_spans(5020, 192, 3)
    assert len(big) == 9 and big[-1] == (4608, 412, 3, 138) and join_scans(5020, 192, 3) == 27
    assert join_spans(5020, 65536, 16) == [(0, 5020, 1, 5020)]  # the default knobs: one span from tile 0
    assert join_spans(1520, 200, 3) == spans  # the block is rounded down to a multiple of 64


@pytest.mark.parametrize("key", SHAPE_STORES, ids=lambda k: "%s-%d-d%d" % k[:3])
def test_stores_hold_every_distance_and_equal_the_oracle(key):
    codes, want = shape_case(*key)
    name, families, D, _ = key
    assert codes.shape == (families * 10 + 20, SHAPE_TABLE[name][1])
    assert len(want) >= families and (want["query"] < want["subject"]).all() and want["dist"].max() == D
    check_against_oracle(codes, want, D)


def test_the_replaned_store():
    pieces, want = replaned_case()
    assert [len(p) for p in pieces] == [1000, 20, 500]
    assert max(p.max() for p in pieces[:2]) == 3 and (pieces[2] == 4).any()
    check_against_oracle(np.concatenate(pieces), want, 5)


def test_tables_agree():
    """the shapes shared with SHAPES are the same stores' kinds and lengths"""
    old = {s[0]: s for s in cases.SHAPES}
    for name in ("nt130", "nt60", "aa60"):
        assert old[name][1:3] == SHAPE_TABLE[name][:2]

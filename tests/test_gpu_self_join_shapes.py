"""The self-join at every store SHAPE (tests/self_join_cases.py SHAPE_TABLE): records wider than one LDS window of
store_records_kernel, spans that start past wave tile 0 and in the middle of one, and each scan family behind such a span.

Every test compares `self_pairs(D).tobytes()` with brute force on the code bytes; nothing is expected from the code under test.
The stores, the window counts and the span arithmetic are checked on the CPU by tests/test_self_join_shapes_model.py.  The knobs
(SMAFA_JOIN_BLOCK, SMAFA_JOIN_STRIDE) are read when a handle is made: every test sets them, then makes its handle.  That a
store was cut into the spans the knobs say is observed through the call's scan count, which kernel ran through its name.
The file takes 2.3 s on an MI355X (brute force included)."""
import numpy as np
import pytest

import smafa_amd
from self_join_cases import (LOOSE_BOUND, LOOSE_SUBS, NARROW_SHAPES, ONE_SPAN_FAMILIES, SHAPE_TABLE, SORTED_FAMILIES, SPANS_FAMILIES,
                             WIDE_SHAPES, join_scans, replaned_case, shape_bound, shape_case)

pytestmark = pytest.mark.gpu
BLOCK, STRIDE = 192, 3  # spans of 576 positions: they start 64 and 128 rows into a wave tile


def make_store(name, pieces):
    kind = SHAPE_TABLE[name][0]
    store = smafa_amd.SubjectStore(SHAPE_TABLE[name][1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    for p in pieces:
        store.push(p)
    return store


def set_spans(monkeypatch, block=BLOCK, stride=STRIDE):
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", str(block))
    monkeypatch.setenv("SMAFA_JOIN_STRIDE", str(stride))


def join_and_check(store, want, D, min_scans, what):
    """one call (room for every row at once, so the statistics are this call's): the rows, the scan count -> the kernel names"""
    got = store.self_pairs(D, first_cap=1 << 20)
    stats, kernels = store.last_call_stats(), store.last_call_kernels()
    print("%s, D = %d: %d pairs, %d scans (at least %d), kernels %s" % (what, D, len(want), stats["scans"], min_scans, kernels))
    assert got.tobytes() == want.tobytes(), what
    assert stats["scans"] >= min_scans, (what, stats)  # (>=: a piece that overflowed the scratch list is scanned again)
    assert "smafa_join::store_records_kernel" in kernels and "smafa_join::join_filter_kernel" in kernels
    return [k for k in kernels if k.startswith("smafa::")]


def planes_of(name):
    return "%d, %d" % SHAPE_TABLE[name][3:5]


@pytest.mark.parametrize("name", WIDE_SHAPES)
def test_wide_records_one_span(name):
    """(a) does a record survive the windows: 1 020 rows (append order kept), default knobs — one span from tile 0"""
    codes, want = shape_case(name, ONE_SPAN_FAMILIES, 5)
    store = make_store(name, [codes])
    assert store.info().planes == SHAPE_TABLE[name][3]
    join_and_check(store, want, 5, 1, name)
    store.close()


@pytest.mark.parametrize("name", list(SHAPE_TABLE))
def test_spans_off_the_tile_grid(name, monkeypatch):
    """(b) 1 520 rows in spans of 3 x 192: three spans, the second and third begin inside a wave tile (store_records_kernel keeps to
    [p0, p1), the scan sees the rows in front of p0 again and join_filter_kernel drops them), the last one short (another S and R)"""
    D = shape_bound(name)
    codes, want = shape_case(name, SPANS_FAMILIES, D)
    set_spans(monkeypatch)
    store = make_store(name, [codes])
    assert store.info().planes == SHAPE_TABLE[name][3]
    assert join_scans(len(codes), BLOCK, STRIDE) == 8
    join_and_check(store, want, D, 8, name)
    store.close()


@pytest.mark.parametrize("bound", [5, LOOSE_BOUND])
@pytest.mark.parametrize("name", ["aa200", "nt520"])
def test_wide_and_generic_kernels_past_tile_0(name, bound, monkeypatch):
    """(c) more than four words per plane: scan_wide_kernel while level 1 of the prefilter prunes (bound 5), scan_generic_kernel
    above (bound 20, members planted up to 10 columns from their seed; scan_plan.h plan_scan — the rule
    test_wide_lengths_all_modes_equal_oracle pins), each over spans past tile 0"""
    codes, want = shape_case(name, SPANS_FAMILIES, bound, LOOSE_SUBS if bound == LOOSE_BOUND else 4)
    set_spans(monkeypatch)
    store = make_store(name, [codes])
    scan = join_and_check(store, want, bound, 8, name)
    if bound == 5:
        assert "smafa::scan_wide_kernel<%s, false, 3, 0>" % planes_of(name) in scan, scan
    else:
        assert scan == ["smafa::scan_generic_kernel"], scan
    store.close()


@pytest.mark.parametrize("variant", ["prefilter off", "zone level 0", "zone level 2"])
@pytest.mark.parametrize("name", NARROW_SHAPES)
def test_per_length_kernels_past_tile_0(name, variant, monkeypatch):
    """(c) one to four words per plane, the fixed-bound forms over the spans of (b).  Which family a setting takes (engine.hip
    launch_tiles / launch_scan): prefilter off -> scan_kernel; zone level 0 -> the filter-plane-resident kernel — scan_lazy_kernel,
    or scan_wide_kernel for one-word stores — as these bounds are ones level 1 prunes at; zone level 2 -> scan_zone_kernel, since
    every block here has more than 64 records (the few-query form: test_few_query_zone_kernel_past_tile_0)."""
    D = shape_bound(name)
    codes, want = shape_case(name, SPANS_FAMILIES, D)
    W, ids = SHAPE_TABLE[name][5], planes_of(name)
    set_spans(monkeypatch)
    store = make_store(name, [codes])
    if variant == "prefilter off":
        store.set_prefilter(False)
        family = "smafa::scan_kernel<%s, %d, " % (ids, W)
    elif variant == "zone level 0":
        store.set_zone_level(0)
        family = "smafa::scan_wide_kernel<%s, false, 1, 0>" % ids if W == 1 else "smafa::scan_lazy_kernel<%s, %d, " % (ids, W)
    else:
        store.set_zone_level(2)
        family = "smafa::scan_zone_kernel<%s, %d, true, " % (ids, W)  # (true: one bound for every query)
    scan = join_and_check(store, want, D, 8, "%s, %s" % (name, variant))
    assert scan and all(k.startswith(family) for k in scan), (family, scan)
    store.close()


@pytest.mark.parametrize("name", ["nt90", "aa120"])
def test_few_query_zone_kernel_past_tile_0(name, monkeypatch):
    """(c) blocks of 64 at stride 5: spans of 320 positions (they start 64, 128 and 192 rows into a tile), 24 blocks of at most 64
    records — scan_zone_few_kernel is the only scan kernel of the call"""
    codes, want = shape_case(name, SPANS_FAMILIES, 5)
    set_spans(monkeypatch, 64, 5)
    store = make_store(name, [codes])
    store.set_zone_level(2)
    assert join_scans(len(codes), 64, 5) == 24
    scan = join_and_check(store, want, 5, 24, name)
    assert scan == ["smafa::scan_zone_few_kernel<%s, %d>" % (planes_of(name), SHAPE_TABLE[name][5])], scan
    store.close()


def test_wide_kernels_zone_level_past_tile_0(monkeypatch):
    """(d) scan_wide_kernel's own zone level (ScanArgs::zone_on, zone[tile]) on a sorted store — 5 020 rows in one push — cut into
    nine spans"""
    codes, want = shape_case("nt330", SORTED_FAMILIES, 3)
    set_spans(monkeypatch)
    store = make_store("nt330", [codes])
    store.set_zone_level(2)
    assert join_scans(len(codes), BLOCK, STRIDE) == 27
    scan = join_and_check(store, want, 3, 27, "nt330, sorted")
    assert "smafa::scan_wide_kernel<2, 3, false, 3, 0> (zone level on)" in scan, scan
    store.close()


def test_a_store_replaned_before_the_join(tmp_path, monkeypatch):
    """(e) 1 000 + 20 + 500 rows of nt330, the first N in the last piece: two planes for two appends, three from the third on.
    The join of the re-planed store, and of the same store saved and loaded, equals brute force on the concatenation."""
    pieces, want = replaned_case()
    set_spans(monkeypatch)
    store = make_store("nt330", pieces[:2])
    assert store.info().planes == 2
    store.push(pieces[2])
    assert store.info().planes == 3 and len(store) == 1520
    join_and_check(store, want, 5, 8, "nt330 re-planed")
    path = str(tmp_path / "replaned.packed")
    store.save(path)
    store.close()
    loaded = smafa_amd.SubjectStore.load(path)
    assert loaded.info().planes == 3 and len(loaded) == 1520
    join_and_check(loaded, want, 5, 8, "nt330 re-planed, loaded")
    loaded.close()

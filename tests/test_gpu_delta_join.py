"""The delta self-join of a resident store (smafa_db_self_hits_since / smafa_db_self_since_launch / `smafa pairs --since`) and
the components update (smafa_db_self_components_update / _launch): the pairs and the components that the rows appended since
a mark have added, from m x n pair tests.

Expected rows are brute force on the code bytes (tests/self_join_cases.py: brute_pairs) filtered to subject >= first_row
(tests/delta_cases.py); expected labels are what smafa_db_self_components — held against brute force by
tests/test_gpu_components.py — gives on the same store, and brute force (tests/components_cases.py).  Nothing here is
expected from the code under test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from components_cases import brute_labels, n_components
from delta_cases import has_both_kinds, kind_of, library_log, marks, pair_keys, since, store_case
from self_join_cases import ONE_SPAN_FAMILIES, SHAPE_TABLE, SHAPES, replaned_case, shape_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER, FILTER, SEED = "smafa_dl::gather_records_kernel", "smafa_dl::delta_filter_kernel", "smafa_dl::seed_parents_kernel"


def new_store(L, kind):
    return smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)


def grown_store(codes, kind, *cuts):
    """the rows pushed in pieces cut at `cuts`"""
    store = new_store(codes.shape[1], kind)
    edges = [0, *cuts, len(codes)]
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            store.push(codes[a:b])
    return store


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_delta_pairs_equal_brute_force(name):
    codes, want, D = store_case(name)
    n, kind = len(codes), kind_of(name)
    for n0 in marks(n):
        store = grown_store(codes, kind, n0)
        got = store.self_pairs_since(n0, D)
        expect = since(want, n0)
        print("%s, first_row %d of %d: %d rows, kernels %s" % (name, n0, n, len(expect), store.last_call_kernels()))
        assert got.tobytes() == expect.tobytes(), (name, n0)
        if n0 in (n // 2, n - 300):
            assert has_both_kinds(expect, n0, D), (name, n0)
        if n0 == n:
            assert len(got) == 0
        if n0 == 0:
            assert got.tobytes() == store.self_pairs(D).tobytes()
        if n0 == n // 2:
            # the partition: pairs of the first n0 rows, from a store that holds only them, and the delta
            first = new_store(codes.shape[1], kind)
            first.push(codes[:n0])
            old = first.self_pairs(D)
            first.close()
            whole = store.self_pairs(D)
            assert whole.tobytes() == want.tobytes()
            assert len(np.intersect1d(pair_keys(old), pair_keys(got))) == 0
            both = np.concatenate([old, got])
            both = both[np.lexsort((both["subject"], both["dist"], both["query"]))]
            assert both.tobytes() == whole.tobytes()
        store.close()
    store = grown_store(codes, kind)
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_pairs_since(n + 1, D)
    assert e.value.code == _lib.ERR_INVALID and "first_row" in str(e.value)
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_pairs_since(0, None)
    assert e.value.code == _lib.ERR_INVALID
    store.close()


@pytest.mark.parametrize("name", ["aa60", "nt60n"])
def test_through_a_resort(name, monkeypatch):
    """SMAFA_RESORT_MIN=64: the store — two appends, the first below the size at which an append is sorted by itself, so all of
    it counts as grown since the last sort — is sorted again in front of the join, at either mark, and the new rows are
    scattered over the positions.  SMAFA_RESORT=0: never, they stay a run of their own.  Whether the store was sorted again is
    read from the library's own level-2 line.  The same rows every time."""
    codes, want, D = store_case(name)
    n, kind = len(codes), kind_of(name)
    for n0 in (n // 2, n - 300):
        rows = []
        for var, value in (("SMAFA_RESORT_MIN", "64"), ("SMAFA_RESORT", "0")):
            monkeypatch.setenv(var, value)
            store = grown_store(codes, kind, n0)
            monkeypatch.delenv(var)
            got, log = library_log(lambda: store.self_pairs_since(n0, D))
            assert "delta self-join of %d rows from row %d" % (n, n0) in log, log
            assert ("sorted again on the device" in log) == (var == "SMAFA_RESORT_MIN"), (var, n0, log)
            rows.append(got)
            assert GATHER in store.last_call_kernels()
            store.close()
        assert rows[0].tobytes() == since(want, n0).tobytes(), (name, n0)
        assert rows[1].tobytes() == rows[0].tobytes(), (name, n0)


@pytest.mark.parametrize("name", ["aa700", "nt330", "nt330n", "nt520"])
def test_record_shapes(name):
    """multi-window records, the zero slots of the plane a two-plane store does not keep, stored words in the second window"""
    codes, want = shape_case(name, ONE_SPAN_FAMILIES, 5, 4)
    n0 = len(codes) - 333  # no multiple of 64
    expect = since(want, n0)
    assert has_both_kinds(expect, n0, 5)
    store = grown_store(codes, SHAPE_TABLE[name][0], n0)
    assert store.info().planes == SHAPE_TABLE[name][3]
    assert store.self_pairs_since(n0, 5).tobytes() == expect.tobytes()
    store.close()


def test_replaned_store():
    pieces, want = replaned_case()
    store = new_store(330, "nt")
    for p in pieces:
        store.push(p)
    assert store.info().planes == 3
    expect = since(want, 1000)
    assert ((expect["query"] < 1000)).any() and (expect["query"] >= 1000).any()
    assert store.self_pairs_since(1000, 5).tobytes() == expect.tobytes()
    store.close()


def test_many_pieces(monkeypatch):
    """1 510 new rows in blocks of 192, three blocks to a span: several spans, a short last block"""
    codes, want, D = store_case("aa60")
    n0 = len(codes) - 1510
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "192")
    monkeypatch.setenv("SMAFA_JOIN_STRIDE", "3")
    store = grown_store(codes, "aa", n0)
    monkeypatch.delenv("SMAFA_JOIN_BLOCK")
    monkeypatch.delenv("SMAFA_JOIN_STRIDE")
    assert store.self_pairs_since(n0, D, first_cap=1 << 20).tobytes() == since(want, n0).tobytes()
    stats = store.last_call_stats()
    assert stats["scans"] >= -(-1510 // 192), stats
    assert stats["kernel_ms"] > 0 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    store.close()


def delta_kernels_ok(store):
    names = store.last_call_kernels()
    assert GATHER in names and FILTER in names and "smafa_join::store_records_kernel" not in names, names
    return names


@pytest.mark.parametrize("name", ["aa60", "nt60"])
def test_every_engine_one_answer(name, monkeypatch):
    """the switch matrix of tests/test_gpu_self_join.py::test_every_engine_one_answer; every case launches
    smafa_dl::gather_records_kernel and smafa_dl::delta_filter_kernel and not smafa_join::store_records_kernel"""
    codes, want, D = store_case(name, 2000)
    kind, n0 = kind_of(name), len(codes) // 2
    expect = since(want, n0)
    store = grown_store(codes, kind)
    assert store.self_pairs_since(n0, D, first_cap=1 << 20).tobytes() == expect.tobytes()
    names = delta_kernels_ok(store)
    assert names[0].startswith("smafa::scan_"), names
    assert [k for k in names if k.startswith(("smafa_join::", "smafa_dl::"))] == [GATHER, "smafa_join::inverse_order_kernel", FILTER]
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 4 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    store.set_prefilter(False)
    assert store.self_pairs_since(n0, D).tobytes() == expect.tobytes()
    delta_kernels_ok(store)
    store.set_prefilter(True)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        assert store.self_pairs_since(n0, D, first_cap=1 << 20).tobytes() == expect.tobytes(), level
        names = delta_kernels_ok(store)
        if level == 2:
            assert any("scan_zone_kernel" in k for k in names), names
    store.close()
    # a current block index answers the blocks (the limits lifted as tests/test_gpu_self_join.py lifts them)
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = grown_store(codes, kind)
    info = store.build_index(D)
    store.set_index(1)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    before = store.index_info()["probe_launches"]
    assert store.self_pairs_since(n0, D, first_cap=1 << 20).tobytes() == expect.tobytes()
    assert store.index_info()["probe_launches"] > before
    names = delta_kernels_ok(store)
    assert any(k.startswith("smafa::index_probe_kernel") for k in names), names
    store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    # the same rows appended in 40 pieces: unsorted runs, then the automatic re-sort in front of the join
    monkeypatch.setenv("SMAFA_RESORT_MIN", "4096")
    grown = grown_store(codes, kind, *np.linspace(0, len(codes), 41).astype(int)[1:-1])
    assert grown.self_pairs_since(n0, D).tobytes() == expect.tobytes()
    delta_kernels_ok(grown)
    grown.close()


@pytest.mark.parametrize("ceiling", [None, "1000000"])
def test_dense_store_rescans_and_capacity(ceiling, monkeypatch):
    """the 4 000-row store of tests/test_gpu_self_join.py::test_dense_store_grows_buffer_and_scratch — 2 000 copies of one row
    and 2 000 of a second row at distance 3, D = 3: every pair qualifies — with first_row = 2 000: the 2 000 new rows' scan
    reports 8M rows, twice the scratch list (grown, or with the ceiling halved down to pieces that fit)"""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 4, size=60).astype(np.uint8)
    b = a.copy()
    b[[3, 30, 59]] = (b[[3, 30, 59]] + 1) % 4
    group = rng.permutation(np.repeat([0, 1], 2000))
    codes = np.where(group[:, None] == 0, a[None, :], b[None, :]).astype(np.uint8)
    i, j = np.triu_indices(4000, 1)
    i, j = i[j >= 2000], j[j >= 2000]
    d = np.where(group[i] == group[j], 0, 3)
    order = np.lexsort((j, d, i))
    want = np.zeros(len(i), dtype=smafa_amd.HIT_DTYPE)
    want["query"], want["subject"], want["dist"] = i[order], j[order], d[order]
    total = (2000 + 3999) * 2000 // 2
    assert len(want) == total
    if ceiling:
        monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", ceiling)
    store = grown_store(codes, "nt")
    l, n_out = _lib.lib(), C.c_uint64(0)
    assert l.smafa_db_self_hits_since(store._h, 2000, 3, None, 0, C.byref(n_out)) == _lib.ERR_CAPACITY  # the count alone
    assert n_out.value == total
    # the path under test ran: the one block's first scan reports 8M rows, twice the 4M-row scratch list the handle starts with.
    # Without a ceiling the list grows and the block is scanned again: two scans.  Under the ceiling the list may not grow: the
    # block is halved, and no piece that is taken has more rows than the list holds, 4M of the 8M: the overflowing scan and two
    # more at the least.
    assert store.last_call_stats()["scans"] >= (3 if ceiling else 2), store.last_call_stats()
    small = np.zeros(1000, dtype=smafa_amd.HIT_DTYPE)
    n_out = C.c_uint64(0)
    assert l.smafa_db_self_hits_since(store._h, 2000, 3, small.ctypes.data, 1000, C.byref(n_out)) == _lib.ERR_CAPACITY
    assert n_out.value == total and b"%d rows needed" % total in l.smafa_last_error()
    got = np.zeros(total, dtype=smafa_amd.HIT_DTYPE)
    assert l.smafa_db_self_hits_since(store._h, 2000, 3, got.ctypes.data, total, C.byref(n_out)) == _lib.OK
    assert n_out.value == total and got.tobytes() == want.tobytes()
    if ceiling:
        assert store.last_call_stats()["scans"] >= 3, store.last_call_stats()  # (the list has not grown: halved again)
    store.close()


def check_update(store, n_before, D, labels_before, codes_now):
    labels, count = store.self_components_update(n_before, D, labels_before)
    names = store.last_call_kernels()
    full, full_count = store.self_components(D)
    assert labels.tobytes() == full.tobytes() and count == full_count, (n_before, D)
    brute, _ = brute_labels(codes_now, D)
    assert labels.tobytes() == brute.tobytes() and count == n_components(brute)
    return labels, names


@pytest.mark.parametrize("name", ["aa60", "nt60n"])
def test_components_update_over_three_appends(name):
    codes, _, _ = store_case(name)
    kind, L = kind_of(name), codes.shape[1]
    store = new_store(L, kind)
    labels = {D: np.zeros(0, dtype=np.uint32) for D in (0, 2, 5)}
    before = 0
    for now in (1000, 2000, 3020):
        store.push(codes[before:now])
        for D in (0, 2, 5):
            labels[D], names = check_update(store, before, D, labels[D], codes[:now])
            assert "smafa_dl::seed_parents_kernel" in names and GATHER in names and "smafa_cc::flatten_labels_kernel" in names, names
            assert "smafa_cc::init_labels_kernel" not in names and "smafa_join::store_records_kernel" not in names, names
        before = now
    n = 3020
    # first_row = 0 is the full call: what labels[] holds is ignored
    got, count = store.self_components_update(0, 5, np.full(n, 0xffffffff, dtype=np.uint32))
    assert got.tobytes() == labels[5].tobytes() and count == n_components(labels[5])
    # first_row = n: the labels as given, the representatives counted; nothing is scanned
    got, count = store.self_components_update(n, 2, labels[2])
    assert got.tobytes() == labels[2].tobytes() and count == n_components(labels[2])
    assert store.last_call_stats()["scans"] == 0 and GATHER not in store.last_call_kernels()
    # max_div = seq_len: one set
    got, count = store.self_components_update(2000, L, labels[5][:2000])
    assert not got.any() and count == 1
    # labels that cannot be labels: SMAFA_ERR_INVALID with their number, labels[] untouched, the handle usable
    first = labels[5][:2000]
    member = int(np.nonzero(first != np.arange(2000))[0][0])                                   # no representative ...
    other = int(np.nonzero((first != np.arange(2000)) & (np.arange(2000) > member))[0][0])     # ... and another behind it
    above, chained = first.copy(), first.copy()
    above[10] = 11
    chained[other] = member
    l = _lib.lib()
    for bad in (above, chained):
        buf = np.zeros(n, dtype=np.uint32)
        buf[:2000] = bad
        buf[2000:] = 0xabcdef
        given = buf.copy()
        count = C.c_uint64(7)
        assert l.smafa_db_self_components_update(store._h, 2000, 5, buf.ctypes.data, n, C.byref(count)) == _lib.ERR_INVALID
        assert b"labels" in l.smafa_last_error() and buf.tobytes() == given.tobytes()
        got, count = store.self_components_update(2000, 5, first)  # the next valid call on the same handle
        assert got.tobytes() == labels[5].tobytes() and count == n_components(labels[5])
    count = C.c_uint64(0)
    buf = np.zeros(n, dtype=np.uint32)
    assert l.smafa_db_self_components_update(store._h, n + 1, 5, buf.ctypes.data, n, C.byref(count)) == _lib.ERR_INVALID
    assert l.smafa_db_self_components_update(store._h, 0, 5, buf.ctypes.data, n - 1, C.byref(count)) == _lib.ERR_INVALID
    assert l.smafa_db_self_components_update(store._h, 0, 5, None, n, C.byref(count)) == _lib.ERR_INVALID
    assert l.smafa_db_self_components_update(store._h, 0, 5, buf.ctypes.data, n, None) == _lib.ERR_INVALID
    assert l.smafa_db_self_components_update(store._h, 0, _lib.NONE, buf.ctypes.data, n, C.byref(count)) == _lib.ERR_INVALID
    store.close()


def test_device_forms():
    """smafa_db_self_since_launch and smafa_db_self_components_update_launch on torch buffers — tests/delta_worker.py, a process
    of its own: torch has to initialise HIP before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "delta_worker.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "delta device forms ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_against_the_query_path_at_scale():
    """200 000 x 60 aa in 2 000 families of 100, the last 2 000 rows new, D = 5: the delta rows are `scan` of the new rows' codes
    against the store — the path the rest of the suite holds against the oracle — reduced by partner number < own number"""
    D, m = 5, 2000
    codes = synth.related_subjects(2000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    assert n == 200_000
    n0 = n - m
    store = grown_store(codes, "aa", n0)
    got = store.self_pairs_since(n0, D, first_cap=1 << 20)
    ref = store.scan(codes[n0:], max_divergence=D)
    own = ref["query"].astype(np.int64) + n0
    keep = ref["subject"] < own
    want = np.zeros(int(keep.sum()), dtype=smafa_amd.HIT_DTYPE)
    want["query"], want["subject"], want["dist"] = ref["subject"][keep], own[keep], ref["dist"][keep]
    want = want[np.lexsort((want["subject"], want["dist"], want["query"]))]
    print("%d rows, %d new: %d delta rows" % (n, m, len(want)))
    assert len(want) >= m and (want["query"] >= n0).any() and (want["query"] < n0).any()
    assert got.tobytes() == want.tobytes()
    store.close()


def test_cli_pairs_since(tmp_path):
    codes, want, D = store_case("nt60")
    n = len(codes)
    fa, db = str(tmp_path / "s.fa"), str(tmp_path / "s.db")
    synth.write_fasta(fa, codes, 0)
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, "--alphabet", "nt"], capture_output=True).returncode == 0
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", str(D)], capture_output=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines(keepends=True)
    assert len(lines) == len(want)
    for row in (n // 2, n - 1):
        r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", str(D), "--since", str(row)], capture_output=True)
        assert r.returncode == 0, r.stderr
        expect = [x for x in lines if max(int(x.split(b"\t")[0]), int(x.split(b"\t")[1])) >= row]
        assert len(expect) == len(since(want, row)) and r.stdout == b"".join(expect), row
    out = str(tmp_path / "since.tsv")
    with open(out, "wb") as f:
        smafa_amd.pairs_since(db, n // 2, D, out_fd=f.fileno())
    assert open(out, "rb").read() == b"".join(x for x in lines if int(x.split(b"\t")[1]) >= n // 2)
    r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", db, "--max-divergence", str(D), "--since", str(n + 1)], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"first_row %d" % (n + 1) in r.stderr, r.stderr

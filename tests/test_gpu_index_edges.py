"""The block index against inputs planted for its own geometry (tests/index_edges.py; the classes are validated on the CPU by
tests/test_index_edges_model.py): blocks on two words, exactly one probed block clean — for every block in turn —, pairs
that agree on several probed blocks, bounds below blocks - 1 where the planner picks the probed blocks, 32 blocks of 3 to 4
columns, one column per block, stores of fewer than 256 rows.  Every scan must be answered by the expected
index_probe_kernel<..> with the oracle's rows, byte for byte.  And index_stats_kernel's run statistics, which decide what
is probed, against runs of known length.  Everything through the C ABI."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import oracle
import smafa_amd
from index_edges import SHAPES, SIZES, IndexPlanter, small_store
from kernel_census_table import PSPQ, SWITCHES
from kernel_edges import KINDS
from smafa_amd import _lib
from test_gpu_layout import expected_with_k

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    assert smafa_amd.device_count() >= 1


@pytest.fixture
def index_switches():
    """the census's `index` switches (no limit on runs or candidates: routing does not depend on the data); read when a
    handle is created"""
    env = dict(SWITCHES["index"])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _scan(store, q, D, k=None):
    """smafa_scan_hits with room for every pair: one call (tests/test_gpu_kernel_census.py)"""
    cap = max(1, len(q) * len(store))
    out = np.zeros(cap, dtype=smafa_amd.HIT_DTYPE)
    n_out = C.c_uint64(0)
    rc = _lib.lib().smafa_scan_hits(store._h, q.ctypes.data, len(q), D, _lib.NONE if not k else k, out.ctypes.data, cap, C.byref(n_out))
    assert rc == 0, (rc, _lib.lib().smafa_last_error())
    return out[: n_out.value]


def probe_name(kind, L):
    return "smafa::index_probe_kernel<%d, %d, %d>" % (PSPQ[kind] + ((L + 31) // 32,))


def diff(got, want):
    g, w = {tuple(r) for r in got.tolist()}, {tuple(r) for r in want.tolist()}
    return "%d rows, oracle %d; missing %s; extra %s" % (len(got), len(want), sorted(w - g)[:6], sorted(g - w)[:6])


def check_every_bound(store, kind, L, D, s, q):
    """bounds D, D - 1, .., 0 and k = 2 on top of D: the probe kernel, the oracle's rows"""
    info = store.build_index(D)
    assert info["current"] == 1 and info["blocks"] == D + 1 and info["max_div_served"] == D, info
    full = oracle.scan_codes(s, q, D)
    name = probe_name(kind, L)
    for bound in range(D, -1, -1):
        # (ordered (query, dist, subject): the rows of a lower bound are those of bound D within it, in the same order —
        # held against oracle.scan_codes at the lower bound by tests/test_index_edges_model.py)
        want = full if bound == D else full[full["dist"] <= bound]
        got = _scan(store, q, bound)
        assert store.last_scan_kernel() == name, (bound, store.last_scan_kernel())
        assert store.last_call_kernels() == [name], (bound, store.last_call_kernels())
        assert got.tobytes() == want.tobytes(), "bound %d: %s" % (bound, diff(got, want))
    got = _scan(store, q, D, 2)
    want = expected_with_k(full, 2)
    assert got.tobytes() == want.tobytes(), "k = 2: %s" % diff(got, want)
    # (with k the fixed-bound rows come first — collect_range — unless the bound is past the near-hit ladder's first step,
    # (min(32, L) - 1) / 6: scan_to_host then walks its ladder)
    if D <= (min(32, L) - 1) // 6:
        assert store.last_scan_kernel() == name, store.last_scan_kernel()
    return full


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,L,D", SHAPES, ids=["%s-%d-%d" % s for s in SHAPES])
def test_planted_block_edges(index_switches, kind, L, D, n):
    p = IndexPlanter(kind, L, n, D, seed=zlib.crc32(repr((kind, L, D, n)).encode()))
    store = smafa_amd.SubjectStore(L, KINDS[kind][0])
    store.push(p.first)  # the layout is fixed by the first append
    assert store.info().planes == (2 if kind == "nt3" else KINDS[kind][1])
    store.push(p.second)
    assert store.info().planes == KINDS[kind][1] and len(store) == n
    s, q = p.subjects(), p.queries()
    assert len(q) >= 65
    full = check_every_bound(store, kind, L, D, s, q)
    # (the model test's statement once more, on the rows just compared: nothing planted went missing from the expectation)
    rows = {(int(r["query"]), int(r["subject"])): int(r["dist"]) for r in full}
    for pair in p.planted:
        key = (pair["query"], pair["subject"])
        assert (key not in rows) if pair["cls"] in ("none_clean", "over") else rows[key] == len(pair["cols"]), pair
    store.close()


@pytest.mark.parametrize("n", [1, 200, 257])
@pytest.mark.parametrize("kind,L,D", [(k, L, D) for k in ("nt2", "nt3", "aa") for L, D in ((31, 5), (60, 5), (128, 3))] + [("aa", 120, 31)])
def test_small_stores(index_switches, kind, L, D, n):
    """fewer than 256 rows, and one row past a tile: a directory of 2^8 slots, one partial tile; a store of one row"""
    s, q = small_store(kind, L, n, D, seed=zlib.crc32(repr((kind, L, D, n)).encode()))
    store = smafa_amd.SubjectStore(L, KINDS[kind][0])
    store.push(s)
    assert store.info().planes == KINDS[kind][1] and len(store) == n
    full = check_every_bound(store, kind, L, D, s, q)
    assert len(full) >= 8  # (the last queries are untouched copies of subjects)
    store.close()


N_RANDOM = 3000


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("alone", [False, True], ids=["mixed", "alone"])
def test_run_statistics(index_switches, R, alone):
    """index_stats_kernel: the longest run of equal keys and the sum of squared run lengths of every block, which
    smafa_index_info reports as longest_run and candidates_per_query and index_plan chooses the probed blocks by.

    Store: amino acids, 60 columns, build_index(2) — 3 blocks of 20 columns — of N_RANDOM random rows plus R exact copies of one
    more row (`alone`: the R copies only, so the run ends where the key array ends).  20 random amino-acid columns are distinct
    among 3000 rows (20^20 values), so in every block the keys form n - R runs of one and one run of R: longest_run == R.

    candidates_per_query, by the header: "subjects a query drawn like the store's rows is compared with at max_div_served".  A
    query drawn from the store's n rows falls into a run of length len with probability len / n and is then compared with that
    run's len subjects: sum over runs of len^2 / n = ((n - R) + R * R) / n per probed block, and max_div_served + 1 blocks are
    probed.  smafa_index_info (engine.hip) sums exactly that: mean_run[b] = stats[1] / n — index_stats_kernel's sum of len^2 —
    over the max_div_served + 1 usable blocks of the smallest mean_run; here every block has the same.  No difference to report.

    Two different blocks sharing a 32-bit key would merge two runs: about n^2 / 2^33 = 1e-3 per block for the fixed seed below.
    """
    rng = np.random.default_rng(20 * R + int(alone))
    one = rng.integers(0, 20, size=(1, 60), dtype=np.uint8)
    s = np.repeat(one, R, axis=0)
    if not alone:
        s = np.concatenate([rng.integers(0, 20, size=(N_RANDOM, 60), dtype=np.uint8), s])
        rng.shuffle(s, axis=0)
    n = len(s)
    store = smafa_amd.SubjectStore(60, 1)
    store.push(s)
    info = store.build_index(2)
    assert info["current"] == 1 and info["blocks"] == 3 and info["usable_blocks"] == 3 and info["max_div_served"] == 2, info
    print("R=%d n=%d longest_run=%d candidates_per_query=%r" % (R, n, info["longest_run"], info["candidates_per_query"]))
    assert info["longest_run"] == R, info
    want = 3.0 * ((n - R) + R * R) / n
    assert abs(info["candidates_per_query"] - want) <= 1e-12 * want, (info, want)
    store.close()

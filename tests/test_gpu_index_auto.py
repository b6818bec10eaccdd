"""The automatic builds of the block index across shapes — mode 2 (built by the first eligible scan), mode 3 on the fixed-bound
path and on the path without a bound (rent or buy) — for nucleotide stores of two and three planes and amino-acid stores of
one to four words per plane; and a build that fails (tests/index_fail_worker.py).  Rows always against the oracle.

Handles are created under SMAFA_INDEX_MIN_ROWS=1 (stores of a few thousand rows) and the census's `index` switches (no limit on
runs or candidates): what is under test is WHEN an index is built and that the probe then answers with the oracle's rows, not
whether probing pays on a store of this size — short nucleotide blocks of a few thousand rows would be left to the scan kernels."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import smafa_amd
from kernel_census_table import PSPQ, SWITCHES
from kernel_edges import KINDS
from self_join_cases import brute_pairs, planted_store
from smafa_amd import _lib
from test_gpu_layout import expected_with_k, queries_from

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(kind, L) for kind in ("nt2", "nt3", "aa") for L in (31, 60, 90, 120)]
IDS = ["%s-%d" % s for s in SHAPES]
N = 6000


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    assert smafa_amd.device_count() >= 1


@pytest.fixture
def auto_env():
    keys = dict(SWITCHES["index"], SMAFA_INDEX_MIN_ROWS="1", SMAFA_INDEX="1")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(keys)
    yield os.environ
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def make(kind, L, seed, n=N, nq=300, max_subs=8):
    """queries_from-style random rows, a few of them duplicated; (subjects, queries, letters)"""
    rng = np.random.default_rng(seed)
    letters = {"nt2": 4, "nt3": 5, "aa": 20}[kind]
    s = rng.integers(0, letters, size=(n, L), dtype=np.uint8)
    s[50:54] = s[49]
    s[n - 1] = s[n // 2]
    q = queries_from(rng, s, nq, 5 if kind != "aa" else 20, max_subs)
    return s, np.ascontiguousarray(q)


def open_store(kind, L, s):
    store = smafa_amd.SubjectStore(L, KINDS[kind][0])
    store.push(s)
    assert store.info().planes == KINDS[kind][1]
    return store


def probe_name(kind, L):
    return "smafa::index_probe_kernel<%d, %d, %d>" % (PSPQ[kind] + ((L + 31) // 32,))


def scan_once(store, q, D, cap):
    """smafa_scan_hits, one call with room for `cap` rows (SubjectStore.scan offers 65 536 first and calls again)"""
    out = np.zeros(cap, dtype=smafa_amd.HIT_DTYPE)
    n_out = C.c_uint64(0)
    rc = _lib.lib().smafa_scan_hits(store._h, q.ctypes.data, len(q), D, _lib.NONE, out.ctypes.data, cap, C.byref(n_out))
    assert rc == 0, (rc, _lib.lib().smafa_last_error())
    return out[: n_out.value]


def with_k(full, k):
    """expected_with_k without the loop over rows: per query, the rows up to its k-th smallest distance, ties included"""
    first = np.flatnonzero(np.r_[True, full["query"][1:] != full["query"][:-1]])
    size = np.diff(np.r_[first, len(full)])
    kth = np.where(size >= k, full["dist"][np.minimum(first + k - 1, len(full) - 1)], 0xFFFFFFFF)
    return full[full["dist"] <= np.repeat(kth, size)]


def test_with_k_is_expected_with_k():
    s, q = make("nt3", 31, 1, n=300, nq=40)
    full = oracle.scan_codes(s, q, 31)
    for k in (1, 3, 40, 400):
        assert with_k(full, k).tobytes() == expected_with_k(full, k).tobytes()


@pytest.mark.parametrize("kind,L", SHAPES, ids=IDS)
def test_mode_2_builds_at_the_first_eligible_scan_and_only_grows(auto_env, kind, L):
    auto_env["SMAFA_INDEX"] = "2"
    s, q = make(kind, L, 200 + L)
    store = open_store(kind, L, s)
    assert store.index_info()["current"] == 0
    blocks, build_ms = 0, None
    for D in (3, 5, 2, 6, 4):
        got = store.scan(q, max_divergence=D)
        assert store.last_scan_kernel() == probe_name(kind, L), (D, store.last_scan_kernel())
        assert got.tobytes() == oracle.scan_codes(s, q, D).tobytes(), D
        info = store.index_info()
        if D + 1 > blocks:
            blocks = D + 1
        else:  # a bound the index holds: no rebuild
            assert info["build_ms"] == build_ms, (D, info)
        assert info["current"] == 1 and info["blocks"] == blocks, (D, info)
        build_ms = info["build_ms"]
    assert store.index_info()["probe_launches"] == 5
    store.close()


@pytest.mark.parametrize("kind,L", SHAPES, ids=IDS)
def test_mode_3_fixed_bound_rents_then_buys(auto_env, kind, L):
    auto_env["SMAFA_INDEX"] = "3"
    D, nq0 = 3, 256
    s, q0 = make(kind, L, 300 + L, nq=nq0, max_subs=5)
    vectors = KINDS[kind][1] * ((L + 31) // 32)
    # rent or buy (kth_plan.h index_rent_charge / index_rent_due): every eligible scan is charged nq x n x (planes x words) x 1.7e-12 ms, and the index
    # is built by the call at which the sum reaches 0.3 ms + (D + 1) blocks x n x 1e-7 ms = 0.3024 ms.  The batch is the 256
    # queries `times` over (the rows of a copy are the oracle's with the query number shifted), as many times as bring the
    # build to about the 100th call: a two-plane one-word store needs 579 copies, 148 224 queries, a five-plane four-word one 57.
    price = 0.3 + (D + 1) * N * 1.0e-7
    times = max(1, int(price / (100 * nq0 * N * vectors * 1.7e-12)))
    per_call = float(nq0 * times) * N * vectors * 1.7e-12
    due = math.ceil(price / per_call)  # the call that builds, and that the probe answers
    assert 90 <= due <= 130, due
    q = np.ascontiguousarray(np.tile(q0, (times, 1)))
    base = oracle.scan_codes(s, q0, D)
    want = np.tile(base, times)
    want["query"] += np.repeat(np.arange(times, dtype=np.uint32) * nq0, len(base))
    cap, want = len(want) + 64, want.tobytes()
    store = open_store(kind, L, s)
    calls = by_scan = 0
    while True:
        assert scan_once(store, q, D, cap).tobytes() == want, calls
        calls += 1
        if "index_probe" in store.last_scan_kernel():
            break
        by_scan += 1
        assert calls < 1.1 * due, (calls, due)
    print("%s L=%d: probe at call %d (rule: %d), %d queries" % (kind, L, calls, due, len(q)))
    assert by_scan >= 2 and store.last_scan_kernel() == probe_name(kind, L), (by_scan, store.last_scan_kernel())
    info = store.index_info()
    assert info["current"] == 1 and info["blocks"] == D + 1 and info["probe_launches"] == 1, info
    store.close()


def ladder_blocks(kind, n, L):
    """scan_to_host: blocks as narrow as the store's size leaves selective, 32 at the most"""
    bits = {"aa": 4.3, "nt2": 2.0, "nt3": 2.3}[kind]
    width = int(max(2.0, math.floor((math.log2(n) - 2.0) / bits)))
    return min(32, L // width)


# (kind, L, n): n = 6000 leaves every shape an index of at least ladder[0] + 1 = 6 blocks ((min(32, L) - 1) / 6 = 5 for every L
# here): aa width 2 -> 15 .. 32 blocks, nt3 width 4 -> 7 .. 30, nt2 width 5 -> 6 .. 24.  The rule excludes short rows of a big
# two-plane store: nt2, L = 31 from n = 16 384 (width 6: 5 blocks) — run below at n = 20 000.
LADDER_RULED_OUT = [("nt2", 31, 20000)]


@pytest.mark.parametrize("kind,L", SHAPES, ids=IDS)
def test_mode_3_without_a_bound(auto_env, kind, L):
    auto_env["SMAFA_INDEX"] = "3"
    want_blocks = ladder_blocks(kind, N, L)
    assert want_blocks >= 6
    vectors = KINDS[kind][1] * ((L + 31) // 32)
    # calls without a bound are charged 1.6e-11 ms per pair and stored vector against 0.3 ms + blocks x n x 1e-7 ms: the query
    # count that brings the build to about the 60th call, but no more than 2000 (from 2048 the ladder plans its later steps on a
    # sample scanned at a fixed bound): a two-plane one-word store then builds at call 791, a five-plane four-word one at call 84
    price = 0.3 + want_blocks * N * 1.0e-7
    nq = int(min(2000, max(80, price / (60 * N * vectors * 1.6e-11))))
    due = math.ceil(price / (nq * N * vectors * 1.6e-11))
    s, q = make(kind, L, 400 + L, nq=nq, max_subs=9)
    full = oracle.scan_codes(s, q, L)
    want = {k: with_k(full, k).tobytes() for k in (1, 3, 40)}
    store = open_store(kind, L, s)
    calls = 0
    while store.index_info()["probe_launches"] == 0:
        k = (1, 3, 40)[calls % 3]
        assert store.scan(q, max_num_hits=k).tobytes() == want[k], (calls, k)
        calls += 1
        assert calls < 1.1 * due + 1, (calls, due)
    print("%s L=%d: probe at call %d (rule: %d), %d queries, %d blocks" % (kind, L, calls, due, nq, want_blocks))
    info = store.index_info()
    assert calls >= 3 and info["current"] == 1 and info["blocks"] == want_blocks, (calls, info)
    for k in (1, 3, 40):
        before = store.index_info()["probe_launches"]
        assert store.scan(q, max_num_hits=k).tobytes() == want[k], k
        assert store.index_info()["probe_launches"] > before
    store.close()


@pytest.mark.parametrize("kind,L,n", LADDER_RULED_OUT)
def test_mode_3_without_a_bound_where_the_ladder_rules_the_index_out(auto_env, kind, L, n):
    auto_env["SMAFA_INDEX"] = "3"
    assert ladder_blocks(kind, n, L) < 6
    nq = 2000
    s, q = make(kind, L, 500 + L, n=n, nq=nq, max_subs=4)
    near = oracle.scan_codes(s, q, 8)  # every query is within 4 of its subject: its best hits are among the rows within 8
    assert len(np.unique(near["query"])) == nq
    best = with_k(near, 1).tobytes()
    price = 0.3 + 32 * n * 1.0e-7
    due = math.ceil(price / (nq * n * 2 * 1.6e-11))  # (two planes, one word)  # an index of any size would have come due by this call
    store = open_store(kind, L, s)
    for _ in range(due + 3):
        assert store.scan(q, max_num_hits=1).tobytes() == best
    info = store.index_info()
    assert info["probe_launches"] == 0 and info["current"] == 0, info
    store.close()


def test_self_join_builds_its_index_under_mode_2(auto_env):
    auto_env["SMAFA_INDEX"] = "2"
    codes = planted_store(31, "aa", 60, 250)
    store = smafa_amd.SubjectStore(60, 1)
    store.push(codes)
    assert store.index_info()["current"] == 0
    assert store.self_pairs(5, first_cap=1 << 20).tobytes() == brute_pairs(codes, 5).tobytes()
    info = store.index_info()
    assert info["current"] == 1 and info["blocks"] == 6 and info["probe_launches"] >= 1, info
    assert any("index_probe_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()
    store.close()


@pytest.mark.parametrize("kind", ["aa", "nt2"])
def test_a_build_that_fails_is_not_the_scans_failure(kind):
    """tests/index_fail_worker.py: six cases under SMAFA_INDEX_FAIL_BUILDS=1, in a process of its own at verbosity 1.
    "block index not built" once per automatic case — no retry while the store is unchanged — and never for the explicit build.
    (Before index_build cleared the runtime's last error on its failing paths, the scan that should have fallen back failed.)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "index_fail_worker.py"), kind], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "index fail worker ok: %s" % kind in r.stdout
    sections = r.stderr.split("== case ")[1:]
    assert [sec[0] for sec in sections] == list("abcdef"), r.stderr[-2000:]
    lines = {sec[0]: sec.count("block index not built") for sec in sections}
    assert lines == {"a": 1, "b": 0, "c": 1, "d": 1, "e": 0, "f": 1}, (lines, r.stderr[-3000:])
    assert "out of memory" in r.stderr.lower(), r.stderr[-2000:]

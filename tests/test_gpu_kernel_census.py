"""GPU kernel census: one case per scan-family instantiation of tests/kernel_census_table.py.  Each case asserts that the
instantiation is among the kernels the call launched (smafa_last_call_kernels) and that the rows are byte-identical to the
oracle's, on two stores whose last wave tile and workgroup are partial (n = 1281 and 2047), with queries planted at exactly
the launch's bound and one past it (tests/kernel_edges.py).

Every case runs twice: on the sparse stores above (test_census_case) and on dense ones (test_census_case_dense), where a family
of near-identical rows makes up at least 40 % of the store and most queries lie next to it (tests/kernel_edges.py), so every
workgroup and chunk appends more rows than its LDS stage parks.  Routing does not depend on the data here (the census forces
the zone level and the index limits), so a dense case launches the same instantiation as its sparse twin.

Switches are read when a handle is created: the stores of one switch set are created with it and the environment is
restored right after.  Cases that share a store run on one handle, which varies bound, k, queries, prefilter and zone level."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle
import smafa_amd
from kernel_census_table import CENSUS, SWITCHES
from kernel_edges import KINDS, Planter
from smafa_amd import _lib
from test_gpu_layout import expected_with_k

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1281, 2047)  # 1 and 255 (mod 256), both past one 1024-subject workgroup


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    assert smafa_amd.device_count() >= 1


def _key(c):
    return tuple(sorted((k, v) for k, v in c.items()))


def _store_key(c):
    return (c["switches"], c["kind"], c["L"])


PARAMS = sorted(((name, i, c) for name, cases in CENSUS.items() for i, c in enumerate(cases)),
                key=lambda t: (_store_key(t[2]), t[0], t[1]))


def _scan(store, q, D, k):
    """smafa_scan_hits with room for every pair: ONE call, so last_call_kernels() names its launches (SubjectStore.scan retries
    a call whose rows did not fit its first buffer, and the retry is served from the kept rows: its kernel list is empty)"""
    cap = max(1, len(q) * len(store))
    out = np.zeros(cap, dtype=smafa_amd.HIT_DTYPE)
    n_out = C.c_uint64(0)
    rc = _lib.lib().smafa_scan_hits(store._h, q.ctypes.data, len(q), _lib.NONE if D is None else D, _lib.NONE if not k else k,
                                    out.ctypes.data, cap, C.byref(n_out))
    assert rc == 0, (rc, _lib.lib().smafa_last_error())
    return out[: n_out.value]


def open_stores(key, dense=False):
    """[(store, planter)] of one (switches, kind, L): both sizes, planted for every census case that uses them"""
    switches, kind, L = key
    cases = [c for _, _, c in PARAMS if _store_key(c) == key]
    env = dict(SWITCHES[switches])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    out = []
    try:
        for n in SIZES:
            p = Planter(kind, L, n, seed=zlib.crc32(repr((switches, kind, L, n) + (("dense",) if dense else ())).encode()),
                        dense_bounds=sorted({c["E"] for c in cases}) if dense else None)
            for c in cases:
                p.plant(c["E"], c["k"], c["spread"])
            p.seal()
            store = smafa_amd.SubjectStore(L, KINDS[kind][0])
            store.push(p.first)  # the layout is fixed by the first append
            if kind == "nt2" or kind == "aa":
                assert store.info().planes == KINDS[kind][1]
            elif kind == "nt3":
                assert store.info().planes == 2  # ... and the three-plane store receives its first N only now
            store.push(p.second)
            assert store.info().planes == KINDS[kind][1] and len(store) == n
            out.append((store, p))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


class _Stores:
    """the stores of one (switches, kind, L) at a time, planted for every case that uses them (dense: with a family)"""

    def __init__(self, dense=False):
        self.dense = dense
        self.key, self.stores, self.results = None, [], {}

    def close(self):
        for store, _ in self.stores:
            store.close()
        self.stores = []

    def open(self, key):
        if key == self.key:
            return
        self.close()
        self.key = key
        self.stores = open_stores(key, self.dense)

    def run(self, c):
        """(kernels of every call of the case, list of failures)"""
        key = _key(c)
        if key in self.results:
            return self.results[key]
        self.open(_store_key(c))
        kernels, bad = set(), []
        for store, p in self.stores:
            store.set_prefilter(c["prefilter"])
            store.set_zone_level(c["zone"])
            if c["index"] and not store.index_info()["current"]:
                info = store.build_index(c["D"])
                assert info["max_div_served"] == c["D"], info
            s = p.subjects()
            counts = [c["nq"]] + ([1] if c["nq"] == 64 else [])  # (the few-query form also with a single query)
            for nq in counts:
                q = p.queries(c["E"], nq, c["k"], c["spread"])
                got = _scan(store, q, c["D"], c["k"])
                call = store.last_call_kernels()
                kernels.update(call)
                want = oracle.scan_codes(s, q, c["L"] if c["D"] is None else c["D"])
                if self.dense and c["D"] is not None and not c["k"]:
                    # the dense queries must stay dense: a later planter change must not quietly make these cases sparse
                    per_query = np.bincount(want["query"], minlength=nq)
                    thin = [(int(i), int(per_query[i])) for i in np.nonzero(p.dense_queries(c["E"], nq, c["k"], c["spread"])[1])[0]
                            if per_query[i] < 0.4 * p.n]
                    if thin:
                        bad.append("n=%d nq=%d: dense queries with fewer than 0.4 n rows (query, rows): %s" % (p.n, nq, thin[:6]))
                if c["k"]:
                    want = expected_with_k(want, c["k"])
                if got.tobytes() != want.tobytes():
                    g, w = {tuple(r) for r in got.tolist()}, {tuple(r) for r in want.tolist()}
                    bad.append("n=%d nq=%d: %d rows, oracle %d; missing %s; extra %s; kernels %s" % (
                        p.n, nq, len(got), len(want), sorted(w - g)[:6], sorted(g - w)[:6], call))
        self.results[key] = (kernels, bad)
        return self.results[key]


@pytest.fixture(scope="module")
def stores():
    s = _Stores()
    yield s
    s.close()


@pytest.fixture(scope="module")
def dense_stores():
    s = _Stores(dense=True)
    yield s
    s.close()


def _check_case(stores, name, c):
    kernels, bad = stores.run(c)
    assert not bad, "%s %s: rows differ from the oracle:\n%s" % (name, c, "\n".join(bad))
    want = name + (" (%s)" % c["marker"] if c["marker"] else "")
    assert want in kernels, "%s not launched by %s; launched: %s" % (want, c, sorted(kernels))
    if name.startswith("smafa::scan_wide_kernel") and not c["marker"] and c["zone"] == 0:
        assert name + " (zone level on)" not in kernels, sorted(kernels)
    if name.startswith("smafa::kth_seed_kernel") and not c["marker"]:  # the seed form only: nothing counted a sample
        assert name + " (sample counts)" not in kernels, sorted(kernels)


@pytest.mark.parametrize("name,i,c", PARAMS, ids=["%s#%d" % (n, i) for n, i, _ in PARAMS])
def test_census_case(stores, name, i, c):
    _check_case(stores, name, c)


@pytest.mark.parametrize("name,i,c", PARAMS, ids=["%s#%d-dense" % (n, i) for n, i, _ in PARAMS])
def test_census_case_dense(dense_stores, name, i, c):
    """the same case on the dense stores: the LDS stage full, the spill path, ties far past k"""
    _check_case(dense_stores, name, c)


@pytest.mark.parametrize("switches", sorted({c["switches"] for _, _, c in PARAMS if c["D"] is not None and not c["k"]}))
def test_device_launch_capacity_of_every_fixed_bound_instantiation(switches):
    """smafa_scan_launch's capacity contract for every dense census case of a switch set with a bound and k = 0 — every
    instantiation but the seed forms, which write no rows (tests/device_capacity_worker.py --census, a process of its own:
    torch must initialise HIP before the library does)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "device_capacity_worker.py"), "--census", switches],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "device capacity ok: census switch set %s" % switches in r.stdout, r.stdout[-2000:]


def test_call_kernel_list_is_per_call_and_distinct():
    """the list restarts with every call, names each instantiation once, in first-launch order"""
    rng = np.random.default_rng(3)
    s = rng.integers(0, 4, size=(3000, 60), dtype=np.uint8)
    store = smafa_amd.SubjectStore(60, 0)
    store.push(s)
    store.set_zone_level(0)
    q = s[:100].copy()
    store.scan(q, max_divergence=5)
    assert store.last_call_kernels() == ["smafa::scan_lazy_kernel<2, 3, 2, 4, false, false>"], store.last_call_kernels()
    assert store.last_scan_kernel() == "smafa::scan_lazy_kernel<2, 3, 2, 4, false, false>"
    store.scan(q, max_num_hits=1)  # the ladder's seeds and tightening launches, then the seed at the bound L
    many = store.last_call_kernels()
    assert len(many) == len(set(many)) >= 2 and many[0] == "smafa::scan_lazy_kernel<2, 3, 2, 4, true, false>", many
    assert store.last_scan_kernel() in many
    store.get_distances(q[0])
    assert store.last_call_kernels() == []
    store.close()


def test_hbm_read_probe_measures_a_rate():
    """smafa_hbm_read_probe (both of its kernels: grid-stride and contiguous spans) reports a plausible HBM read rate"""
    rate = smafa_amd.hbm_read_probe(0, 256 << 20)
    assert 100.0 < rate < 20000.0, rate

"""The sampled counting path of the k-th distance modes (k >= 3 without a bound level 1 prunes at; scan_host.hip.h scan_kth with
kth_sample_tiles != 0) below benchmark size, on the planted stores of tests/kth_sample_cases.py (checked on the CPU by
tests/test_kth_sample_model.py): kth_seed_kernel counting a whole sample into cnt[q][d] — every instantiation, the run-time
shape one included —, kth_from_counts_kernel, the one counting-and-appending pass over the rest, the sample's tiles again,
filter_rows_kernel.  Rows are compared byte for byte with the oracle's, and the call's kernel list says which form ran
("<template-id> (sample counts)").

Without a bound the rows come through smafa_scan_hits (one call with room for every row).  Under a bound they come through the device-resident launch
(smafa_scan_launch, rows ordered here): the host path answers a bound from one fixed-bound scan whenever its rows fit, and
would never reach the k-th path at these sizes.  The bound is L // 2, which level 1 of the prefilter does not prune at
(prefilter_prunes; mirrored by kth_sample_cases.level1_prunes), so the k modes still count first.

Switches are read when a handle is created; every handle is created under monkeypatch.setenv and closed."""
import ctypes as C

import numpy as np
import pytest

import kth_sample_cases as cases
import oracle
import smafa_amd
from smafa_amd import _lib
from kth_sample_cases import ALPHABET, BATCHES, KS, PLANES, SHAPES, WALK_SHAPES, WALK_STEPS, seed_kernel
from test_gpu_layout import expected_with_k

pytestmark = pytest.mark.gpu

MARK = " (sample counts)"


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    assert smafa_amd.device_count() >= 1


class _DeviceRows:
    """a row buffer and a counter in HBM for smafa_scan_launch, from the HIP runtime the library has loaded"""

    def __init__(self, cap):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.cap, self.rows, self.count = cap, C.c_void_p(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.rows), cap * 12) == 0
        assert self.hip.hipMalloc(C.byref(self.count), 8) == 0

    def launch(self, store, qset, D, k):
        """the rows of one device-resident launch, ordered (query, dist, subject)"""
        store.scan_launch(qset, D, k, self.rows.value, self.cap, self.count.value)
        store.sync()
        n = C.c_uint64(0)
        assert self.hip.hipMemcpy(C.byref(n), self.count, 8, 2) == 0  # 2: device to host
        assert n.value <= self.cap, (n.value, self.cap)
        out = np.zeros((max(n.value, 1), 3), dtype=np.uint32)
        assert self.hip.hipMemcpy(out.ctypes.data, self.rows, n.value * 12, 2) == 0
        out = out[: n.value]
        order = np.lexsort((out[:, 1], out[:, 2], out[:, 0]))
        return np.ascontiguousarray(out[order]).view(smafa_amd.HIT_DTYPE).reshape(-1)

    def close(self):
        self.hip.hipFree(self.rows)
        self.hip.hipFree(self.count)


@pytest.fixture(scope="module")
def device_rows():
    d = _DeviceRows(1 << 20)
    yield d
    d.close()


def _open(monkeypatch, c, sample, **switches):
    """the case's store on a handle created under the module's switches, SMAFA_KTH_SAMPLE=sample and `switches`"""
    env = dict(cases.ENV, SMAFA_KTH_SAMPLE=str(sample))
    for name in ("SMAFA_KTH_GROUPS", "SMAFA_KTH_HIST_SEED"):
        monkeypatch.delenv(name, raising=False)
    env.update({k: str(v) for k, v in switches.items()})
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    store = smafa_amd.SubjectStore(c.L, ALPHABET[c.kind])
    first, second = c.parts()
    store.push(first)
    if c.kind == "nt3":
        assert store.info().planes == 2  # the first N arrives with the second part: the sampled store is the re-planed one
    store.push(second)
    assert store.info().planes == PLANES[c.kind] and len(store) == c.n
    return store


def _diff(got, want):
    g, w = {tuple(r) for r in got.tolist()}, {tuple(r) for r in want.tolist()}
    return "%d rows, oracle %d; missing %s; extra %s" % (len(got), len(want), sorted(w - g)[:6], sorted(g - w)[:6])


def _seed_lines(kernels):
    return [k for k in kernels if "kth_seed_kernel" in k]


HOST_CAP = 1 << 20  # rows: more than 75 queries x 10241 subjects, and than any k <= 40 answer on the 40961-row stores


def _host_scan(store, q, k):
    """smafa_scan_hits without a bound, with room for every row: ONE call, so last_call_kernels() names its launches
    (SubjectStore.scan retries a call whose rows did not fit its first buffer from the kept rows: an empty kernel list)"""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    out = np.zeros(HOST_CAP, dtype=smafa_amd.HIT_DTYPE)
    n_out = C.c_uint64(0)
    rc = _lib.lib().smafa_scan_hits(store._h, q.ctypes.data, len(q), _lib.NONE, k, out.ctypes.data, HOST_CAP, C.byref(n_out))
    assert rc == 0, (rc, _lib.lib().smafa_last_error())
    return out[: n_out.value].copy()


def _scan(store, device_rows, q, D, k):
    """(rows, the call's kernel list): no bound: the host path; a bound: the device-resident launch"""
    if D is None:
        return _host_scan(store, q, k), store.last_call_kernels()
    qset = smafa_amd.QuerySet(store, q)
    try:
        got = device_rows.launch(store, qset, D, k)
        return got, store.last_call_kernels()
    finally:
        qset.close()


def _full(c, D):
    """every pair within the bound, from the oracle: once per store and bound"""
    return oracle.scan_codes(c.subjects, c.queries, c.L if D is None else D)


@pytest.mark.parametrize("kind,L", SHAPES, ids=["%s-%d" % s for s in SHAPES])
def test_sampled_counts_of_every_shape(kind, L, monkeypatch, device_rows):
    """41 tiles of which 20 are the sample (5 steps of 4 tiles), k = 3, 5, 40 on 75, 33 and 1 queries, without a bound and
    under L // 2: rows == the oracle's; the shape's kth_seed_kernel instantiation ran in its counting form for L <= 255, and
    for L = 256 (no histogram: counting launches of the scan kernels in front of the same sampled passes) not at all.
    k = 2 is the control: the tightening path, no counts."""
    name = seed_kernel(kind, L)
    for k in KS:
        c = cases.case(kind, L, k)
        assert not cases.level1_prunes(L, c.D)
        store = _open(monkeypatch, c, 2)
        try:
            for D in (None, c.D):
                full = _full(c, D)
                for nq in BATCHES:
                    got, kernels = _scan(store, device_rows, c.queries[:nq], D, k)
                    want = expected_with_k(full[full["query"] < nq], k)
                    assert got.tobytes() == want.tobytes(), "k=%d D=%s nq=%d: %s; kernels %s" % (k, D, nq, _diff(got, want), kernels)
                    if name:
                        assert name + MARK in kernels and name in kernels, (k, D, nq, kernels)
                    else:
                        assert not _seed_lines(kernels), (k, D, nq, kernels)
            if k == KS[0]:
                got = _host_scan(store, c.queries, 2)
                kernels = store.last_call_kernels()
                want = expected_with_k(_full(c, None), 2)
                assert got.tobytes() == want.tobytes(), "k=2: %s; kernels %s" % (_diff(got, want), kernels)
                assert not [x for x in kernels if x.endswith(MARK)], kernels
        finally:
            store.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,L", WALK_SHAPES, ids=["%s-%d" % s for s in WALK_SHAPES])
def test_walk_of_many_steps_per_tile_group(kind, L, k, monkeypatch, device_rows):
    """161 tiles, a sample of 80 = 20 steps, walked by 1, 2, 3 tile groups per query chunk (SMAFA_KTH_GROUPS) and by the
    automatic 20: the running bound in LDS, its update every 4th step, the stale bound in between, the flush that keeps a
    group's bins up to its own final bound and adds the shares of groups that ended at different bounds.  The ties of a, b
    and c sit in the tiles of steps 3, 4, 7 and 19 (c: 0 and 19), which belong to different groups when there are 2 or 3
    (step s belongs to group s mod n_groups).  The same bytes four times, the oracle's."""
    c = cases.walk_case(kind, L, k)
    name = seed_kernel(kind, L)
    for qi, m in enumerate(c.meta):
        if m["cls"] in ("a", "b", "c"):
            steps = c.planted_steps(qi, cases.E)
            assert set(steps) <= set(WALK_STEPS) | {0}, steps
            for groups in (2, 3):
                assert len({s % groups for s in steps}) >= 2, (m["cls"], steps, groups)
    wants = {D: expected_with_k(_full(c, D), k) for D in (None, c.D)}
    for groups in (1, 2, 3, None):
        store = _open(monkeypatch, c, 2, **({} if groups is None else {"SMAFA_KTH_GROUPS": groups}))
        try:
            for D, want in wants.items():
                got, kernels = _scan(store, device_rows, c.queries, D, k)
                assert got.tobytes() == want.tobytes(), "groups=%s D=%s: %s; kernels %s" % (groups, D, _diff(got, want), kernels)
                assert name + MARK in kernels, (groups, D, kernels)
        finally:
            store.close()


@pytest.mark.parametrize("kind,L", [("aa", 60), ("nt2", 31)])
def test_rule_that_turns_the_sample_off(kind, L, monkeypatch, device_rows):
    """SMAFA_KTH_SAMPLE=16 on 41 tiles: a sample of 2 tiles = 512 subjects, used while 4 k <= 512.  k = 128 is sampled, k = 129
    is not (everything counted first), k = 20000 > n gives every subject within the bound; k = 40 is what the store is planted for."""
    c = cases.case(kind, L, 40, sample_tiles=2)
    name = seed_kernel(kind, L)
    store = _open(monkeypatch, c, 16)
    try:
        for D in (None, c.D):
            full = _full(c, D)
            for k, sampled in ((40, True), (128, True), (129, False), (20000, False)):
                got, kernels = _scan(store, device_rows, c.queries, D, k)
                want = expected_with_k(full, k)
                assert got.tobytes() == want.tobytes(), "k=%d D=%s: %s; kernels %s" % (k, D, _diff(got, want), kernels)
                assert (name + MARK in kernels) == sampled and name in kernels, (k, D, kernels)
                if k == 20000:
                    assert len(got) == len(full)
    finally:
        store.close()


@pytest.mark.parametrize("kind,L", [(kind, L) for L in (60, 150) for kind in cases.KINDS], ids=lambda v: str(v))
def test_counting_launches_in_place_of_the_histogram(kind, L, monkeypatch, device_rows):
    """SMAFA_KTH_HIST_SEED=0: the sample is counted by launches of the scan kernels.  The same bytes as with the histogram,
    no kth_seed_kernel line at all."""
    name = seed_kernel(kind, L)
    for k in KS:
        c = cases.case(kind, L, k)
        rows = {}
        for hist in (1, 0):
            store = _open(monkeypatch, c, 2, SMAFA_KTH_HIST_SEED=hist)
            try:
                for D in (None, c.D):
                    got, kernels = _scan(store, device_rows, c.queries, D, k)
                    rows[hist, D] = got.tobytes()
                    if hist:
                        assert name + MARK in kernels, (k, D, kernels)
                    else:
                        assert not _seed_lines(kernels), (k, D, kernels)
                        assert rows[0, D] == rows[1, D], (k, D)
                        want = expected_with_k(_full(c, D), k)
                        assert got.tobytes() == want.tobytes(), "k=%d D=%s: %s" % (k, D, _diff(got, want))
            finally:
                store.close()

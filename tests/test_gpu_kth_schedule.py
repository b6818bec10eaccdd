"""A tightening scan launches what kth_schedule (smafa_amd/csrc/kth_plan.h) lists, in that order: the planted stores of
tests/kth_sample_cases.py (10 241 rows = 41 wave tiles, under that module's switches), 75 queries, k = 1 and k = 5 through the
host-buffer call without a bound — one scan, no ladder (SMAFA_TWO_PHASE=0).  (a) the rows are the oracle's; (b) the call's
kernel list and its launch and scan counts are what the schedule gives, the schedule taken from the header itself through the
model driver of tests/kth_plan_model.py (g++ alone; skipped where there is no host compiler).

What a step launches, and whether scan_host.hip.h counts it among the scan's launches (launch_tiles counts, nothing else does):
  Z   ZeroCounts          a memset                                                        no kernel
  SH  SeedHist            kth_seed_kernel                                                 listed, not counted
  MH  SampleHist          kth_seed_kernel, then the marker "<id> (sample counts)"         listed, not counted
  SS  SeedScan            launch_tiles without a row list (k = 1: the SEED instantiation) listed, counted
  C   Count               launch_tiles without a row list                                 listed, counted
  A   CountAppend         launch_tiles into the scratch list                              listed, counted
  XS  FixedAppendScratch  launch_tiles, per-query bounds fixed                            listed, counted
  XC  FixedAppendCaller   launch_tiles, per-query bounds fixed, the caller's list         listed, counted
  B   BoundsFromCounts    kth_from_counts_kernel                                          not listed, not counted
  F   Filter              filter_rows_kernel                                              not listed, not counted
The scan kernel of a launch_tiles step, by scan_plan.h's rules at the bound these launches start from (L, "no bound": level 1
does not prune, no fold rejects, no zone level on an unsorted store): scan_kernel with one tile per wave up to four words per
plane — FOLD 3 (all planes but the last) on the five-plane two-word store except in the seed form, FOLD 0 on the one-word store —
and scan_generic_kernel beyond (150 columns)."""
import pytest

import kth_plan_model as model
import kth_sample_cases as cases
import oracle
import smafa_amd
from kth_sample_cases import ALPHABET, PLANES, seed_kernel
from test_gpu_kth_sample import _diff, _host_scan
from test_gpu_layout import expected_with_k

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(model.compiler() is None, reason="no host C++ compiler")]

SHAPES = [("aa", 60), ("nt2", 31), ("aa", 150)]
# (kind, L) -> the scan kernel of a launch_tiles step: (the seed form of k = 1, every other launch)
SCAN_KERNEL = {
    ("aa", 60): ("smafa::scan_kernel<5, 5, 2, 1, true, 0>", "smafa::scan_kernel<5, 5, 2, 1, false, 3>"),
    ("nt2", 31): ("smafa::scan_kernel<2, 3, 1, 1, true, 0>", "smafa::scan_kernel<2, 3, 1, 1, false, 0>"),
    ("aa", 150): ("smafa::scan_generic_kernel", "smafa::scan_generic_kernel"),
}
COUNTED = ("SS", "C", "A", "XS", "XC")
# the handle's defaults that the schedule's inputs come from, and the module's SMAFA_KTH_SAMPLE_MIN_TILES
COUNT_FIRST_K, SAMPLE_DIV, MIN_TILES = 3, 32, int(cases.ENV["SMAFA_KTH_SAMPLE_MIN_TILES"])


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    assert smafa_amd.device_count() >= 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return model.build(tmp_path_factory.mktemp("kth_plan"))


def _schedule(exe, kind, L, k, n_tiles):
    P = PLANES[kind]
    pq = 5 if kind == "aa" else 3
    (cf,), (hist,) = model.ask(exe, ["count_first %d %d %d %d %d %d %d" % (k, COUNT_FIRST_K, P, pq, (L + 31) // 32, L, L), "hist_seed %d %d 1" % (k, L)])
    (sample,) = model.ask(exe, ["sample_tiles %s %d %d %d %d" % (cf, SAMPLE_DIV, MIN_TILES, n_tiles, k)])[0]
    return model.parse_schedule(model.ask(exe, ["schedule %d %d %s %s %s" % (n_tiles, k, cf, sample, hist)])[0])


def _expected_launches(kind, L, k, steps):
    """(the call's kernel list: distinct names in first-launch order, the launches counted)"""
    seed_form, plain = SCAN_KERNEL[kind, L]
    names, counted = [], 0
    for step, _, _ in steps:
        new = []
        if step in ("SH", "MH"):
            new = [seed_kernel(kind, L)] + ([seed_kernel(kind, L) + " (sample counts)"] if step == "MH" else [])
        elif step in COUNTED:
            new = [seed_form if step == "SS" and k == 1 else plain]
            counted += 1
        names += [n for n in new if n not in names]
    return names, counted


@pytest.mark.parametrize("kind,L", SHAPES, ids=["%s-%d" % s for s in SHAPES])
def test_a_scan_launches_its_schedule(kind, L, exe, monkeypatch):
    for name in ("SMAFA_KTH_SAMPLE", "SMAFA_KTH_GROUPS", "SMAFA_KTH_HIST_SEED", "SMAFA_COUNT_FIRST_K"):
        monkeypatch.delenv(name, raising=False)
    for name, value in cases.ENV.items():
        monkeypatch.setenv(name, value)
    c = cases.case(kind, L, 5)
    assert c.n == cases.N_ROWS and c.n_tiles == 41
    full = oracle.scan_codes(c.subjects, c.queries, L)
    store = smafa_amd.SubjectStore(L, ALPHABET[kind])
    try:
        for part in c.parts():
            store.push(part)
        assert store.info().planes == PLANES[kind]
        for k in (1, 5):
            steps = _schedule(exe, kind, L, k, c.n_tiles)
            # (what these cases are here for: k = 1 walks growing segments behind a seed launch; k = 5 counts a one-tile sample
            # in the histogram kernel — 41 / 32 tiles —, walks the rest in three segments and scans the sample again)
            assert [s[0] for s in steps] == (["SS", "A", "A", "A", "F"] if k == 1 else ["Z", "MH", "B", "A", "A", "A", "B", "XS", "F"]), steps
            got = _host_scan(store, c.queries, k)
            kernels, stats = store.last_call_kernels(), store.last_call_stats()
            want = expected_with_k(full, k)
            assert got.tobytes() == want.tobytes(), "k=%d: %s; kernels %s" % (k, _diff(got, want), kernels)
            names, counted = _expected_launches(kind, L, k, steps)
            assert kernels == names, (k, steps, kernels, names)
            assert (stats["launches"], stats["scans"]) == (counted, 1), (k, steps, stats)
    finally:
        store.close()

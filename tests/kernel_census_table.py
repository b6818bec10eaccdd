"""The kernel census: every smafa:: kernel in the gfx950 code object of libsmafa_amd.so, each mapped to where it runs.

CENSUS maps each scan-family instantiation (the names smafa_last_call_kernels reports) to the case(s) of
tests/test_gpu_kernel_census.py that must launch it, with oracle-identical rows.  EXEMPT maps every other kernel to an
existing test that runs it.  tests/test_kernel_census.py checks that the two together are exactly the kernels in the binary.

A case: the switches read when the handle is created, the store kind (nt2: nucleotides on two planes, nt3: on three, aa:
amino acids on five), the row length L, the bound D (None: none) and k (0: every row within D), the number of queries, the
prefilter, the zone level (0 off, 2 forced), whether a block index is built, `marker` (the note the call's kernel list adds after
the template-id for one form of the kernel: "zone level on", "sample counts"), E — the bound its edge pairs are planted at
(tests/kernel_edges.py) — and `spread` (fillers at distances 0..spread, so every step of the near-hit ladder finishes some).

Which instantiation a launch runs is decided in smafa_amd/csrc/scan_plan.h (plan_scan, scan_kernel_name) and nowhere else;
tests/test_scan_plan_model.py asks that header, compiled for the host, for the name of every fixed-bound case below.

Every fixed-bound case here launches over the whole store (first tile 0).  The fixed-bound forms at a non-zero first tile — the
self-join's triangular cut, for every word count and the wide, generic, zone and few-query kernels — are covered by the self-join
shape tests (tests/test_gpu_self_join_shapes.py).
"""
from __future__ import annotations

SWITCHES = {
    "default": (),
    "tiles4": (("SMAFA_TILES", "4"),),
    "tiles2": (("SMAFA_TILES", "2"),),
    "wide_one_off": (("SMAFA_WIDE_ONE", "0"),),
    "wide_from3": (("SMAFA_WIDE_FROM", "3"),),
    "zone_staged": (("SMAFA_ZONE_DIRECT", "0"),),
    "index": (("SMAFA_INDEX_MAX_RUN", "100000000"), ("SMAFA_INDEX_CAND", "100")),
    # the k-th modes count a sample (half of the census stores' 6 and 8 tiles) first, no near-hit ladder in front
    "kth_sample": (("SMAFA_KTH_SAMPLE", "2"), ("SMAFA_KTH_SAMPLE_MIN_TILES", "4"), ("SMAFA_TWO_PHASE", "0")),
}
KINDS = ("nt2", "nt3", "aa")
PSPQ = {"nt2": (2, 3), "nt3": (3, 3), "aa": (5, 5)}
L_OF_W = {1: 31, 2: 60, 3: 90, 4: 120}
L_FOLD = 45   # two words per plane below 56 columns: level 2 of the filter-plane-resident kernel is not used (fold_rejects)
L_WIDE = 150  # five words per plane


def ladder_top(kind, L):
    """the last bound of the near-hit ladder (kth_plan.h ladder_bounds) for a batch under 2048 queries"""
    cols = min(32, L)
    top = 3 * cols // 8
    if (L + 31) // 32 == 2 and L >= 33:
        top = 16 if kind == "nt2" else 30
    return top


def case(switches, kind, L, D=None, k=0, nq=129, E=None, prefilter=True, zone=0, index=False, marker=None, spread=0):
    return dict(switches=switches, kind=kind, L=L, D=D, k=k, nq=nq, E=D if E is None else E, prefilter=prefilter, zone=zone,
                index=index, marker=marker, spread=spread)


def best_hit(switches, kind, L, zone=0):
    """best hit without a bound: the ladder's steps (seeds at its bounds, then tightening launches), the rest from the seed at L"""
    return case(switches, kind, L, None, 1, 129, E=5, zone=zone, spread=ladder_top(kind, L) + 3)


def _census():
    c = {}

    def add(name, *cases):
        c.setdefault(name, []).extend(cases)

    for kind in KINDS:
        ps, pq = PSPQ[kind]
        for W in (1, 2, 3, 4):
            L = L_FOLD if W == 2 else L_OF_W[W]
            sk = "smafa::scan_kernel<%d, %d, %d, %%d, %%s, %%d>" % (ps, pq, W)
            # one tile per wave: the seed at the bound L (best hit), every pair compared (prefilter off)
            add(sk % (1, "true", 0), best_hit("default", kind, L))
            add(sk % (1, "false", 0), case("default", kind, L, 5, prefilter=False))
            if W <= 2:  # two tiles per wave at bounds up to 16 the filter-plane-resident kernels do not take
                add(sk % (2, "true", 0), best_hit("default", kind, L))  # the ladder's step at 3/8 of the columns
                add(sk % (2, "false", 0), case("default", kind, L, 10))
            if W == 2:  # level 2 of scan_kernel: FOLD 1 at 13..17, FOLD 2 at 18..32 (3+ planes), FOLD 3 beyond (5 planes)
                add(sk % (2, "false", 1), case("default", kind, L, 15))
                add(sk % (1, "false", 1), case("default", kind, L, 17))
                if ps >= 3:
                    add(sk % (1, "false", 2), case("default", kind, L, 24))
                    add(sk % (2, "false", 2), case("tiles2", kind, L, 24))
                if ps >= 5:
                    add(sk % (1, "false", 3), case("default", kind, L, 40))
                    add(sk % (2, "false", 3), case("tiles2", kind, L, 40))
            # the filter-plane-resident kernel (one-word stores only without scan_wide_kernel's one-word form)
            L2 = L_OF_W[W]
            sw = "wide_one_off" if W == 1 else "default"
            T = 4 if W <= 2 else 2
            lk = "smafa::scan_lazy_kernel<%d, %d, %d, %d, %%s, %%s>" % (ps, pq, W, T)
            add(lk % ("true", "false"), best_hit(sw, kind, L2))
            add(lk % ("false", "false"), case(sw, kind, L2, 5))
            if W == 2:
                add(lk % ("false", "true"), case(sw, kind, L2, 13))
            # the zone level of a sorted store (forced), its few-query form, the staged fixed-bound form, per-query bounds
            zk = "smafa::scan_zone_kernel<%d, %d, %d, %%s, %%s>" % (ps, pq, W)
            add(zk % ("true", "true"), case("default", kind, L2, 5, nq=65, zone=2))
            add(zk % ("true", "false"), case("zone_staged", kind, L2, 5, nq=129, zone=2))
            add(zk % ("false", "false"), best_hit("default", kind, L2, zone=2))
            add("smafa::scan_zone_few_kernel<%d, %d, %d>" % (ps, pq, W), case("default", kind, L2, 5, nq=64, zone=2))
            # the seed bound of the first tiles, and the counting form over a whole sample (marker "sample counts")
            add("smafa::kth_seed_kernel<%d, %d, %d>" % (ps, pq, W), case("default", kind, L2, None, 3, 65, E=5),
                case("kth_sample", kind, L2, None, 3, 65, E=5, marker="sample counts"))
            add("smafa::index_probe_kernel<%d, %d, %d>" % (ps, pq, W), case("index", kind, L2, 5, index=True))
        # scan_wide_kernel: one-word stores, stores of more than four words, and three / four words under SMAFA_WIDE_FROM=3
        wk = "smafa::scan_wide_kernel<%d, %d, %%s, %%d, %%d>" % (ps, pq)
        for fw, wc, sw, L in ((1, 0, "default", 31), (3, 0, "default", L_WIDE), (3, 3, "wide_from3", 90), (3, 4, "wide_from3", 120)):
            add(wk % ("true", fw, wc), best_hit(sw, kind, L))
            add(wk % ("false", fw, wc), case(sw, kind, L, 5))
            if wc == 0 and fw == 3:  # its own zone level (more than four words only)
                add(wk % ("false", fw, wc), case(sw, kind, L, 5, zone=2, marker="zone level on"))
        # two tiles per wave forced to four (two-plane stores only)
        if kind == "nt2":
            for W, L in ((1, 31), (2, L_FOLD)):
                sk = "smafa::scan_kernel<2, 3, %d, 4, %%s, %%d>" % W
                add(sk % ("true", 0), best_hit("tiles4", kind, L))
                add(sk % ("false", 0), case("tiles4", kind, L, 10))
                if W == 2:
                    add(sk % ("false", 1), case("tiles4", kind, L, 15))
    add("smafa::kth_seed_kernel<0, 0, 0>", case("default", "aa", L_WIDE, None, 3, 65, E=5),
        case("kth_sample", "aa", L_WIDE, None, 3, 65, E=5, marker="sample counts"))
    add("smafa::scan_generic_kernel", case("default", "aa", L_WIDE, 20))
    return c


CENSUS = _census()

# every other kernel -> an existing test that runs it
EXEMPT = {
    "smafa::pack_rows_kernel<2>": "tests/test_gpu_layout.py::test_host_packed_file_equals_device_saved_file",
    "smafa::pack_rows_kernel<3>": "tests/test_gpu_layout.py::test_host_packed_file_equals_device_saved_file",
    "smafa::pack_rows_kernel<5>": "tests/test_gpu_layout.py::test_host_packed_file_equals_device_saved_file",
    "smafa::zone_kernel": "tests/test_gpu_layout.py::test_host_packed_file_equals_device_saved_file",
    "smafa::row_keys_kernel": "tests/test_gpu_layout.py::test_skewed_columns_sorted_store_all_modes",
    "smafa::replane_kernel": "tests/test_gpu_parity.py::test_nt_store_uses_two_planes_until_an_N_arrives",
    "smafa::position_keys_kernel": "tests/test_gpu_layout.py::test_store_grown_by_small_appends_is_sorted_again",
    "smafa::permute_rows_kernel": "tests/test_gpu_layout.py::test_store_grown_by_small_appends_is_sorted_again",
    "smafa::distances_kernel": "tests/test_gpu_parity.py::test_get_distances_equals_oracle",
    "smafa::fill_u32_kernel": "tests/test_gpu_parity.py::test_kth_bound_modes",
    "smafa::filter_rows_kernel": "tests/test_gpu_kth_sample.py::test_sampled_counts_of_every_shape",
    "smafa::kth_from_counts_kernel": "tests/test_gpu_kth_sample.py::test_sampled_counts_of_every_shape",
    "smafa::rows_to_keys_kernel": "tests/test_gpu_parity.py::test_dense_hits_overflow_path",
    "smafa::keys_to_rows_kernel": "tests/test_gpu_parity.py::test_dense_hits_overflow_path",
    "smafa::index_rows_kernel": "tests/test_gpu_index.py::test_index_rows_equal_scan_rows_and_oracle",
    "smafa::index_keys_kernel": "tests/test_gpu_index.py::test_index_rows_equal_scan_rows_and_oracle",
    "smafa::index_dir_kernel": "tests/test_gpu_index.py::test_index_rows_equal_scan_rows_and_oracle",
    "smafa::index_stats_kernel": "tests/test_gpu_index.py::test_index_rows_equal_scan_rows_and_oracle",
    "smafa::index_interleave_kernel": "tests/test_gpu_index.py::test_index_rows_equal_scan_rows_and_oracle",
    "smafa::hbm_read_probe_kernel": "tests/test_gpu_kernel_census.py::test_hbm_read_probe_measures_a_rate",
    "smafa::hbm_read_probe_span_kernel": "tests/test_gpu_kernel_census.py::test_hbm_read_probe_measures_a_rate",
}

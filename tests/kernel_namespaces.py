"""The kernels of every project namespace other than smafa:: (tests/kernel_census_table.py holds that one), each beside the GPU
test that runs it and asserts it by name (smafa_last_call_kernels), and the words a namespace keeps to itself.  Data only:
tests/test_namespace_census.py holds the gfx950 code object to it.

A new call adds one dict to NAMESPACES, and its words to RESERVED if it reserves any."""

_SELF_JOIN = "tests/test_gpu_self_join.py::"
_COMPONENTS = "tests/test_gpu_components.py::"
_LEVELS = "tests/test_gpu_levels.py::"
_DENSITY = "tests/test_gpu_density.py::"
_PEAKS = "tests/test_gpu_peaks.py::"
_NEIGHBOURS = "tests/test_gpu_neighbours.py::test_neighbours_equal_brute_force"
_DELTA = "tests/test_gpu_delta_join.py::"
_FOREST = "tests/test_gpu_forest.py::"
_REACH = "tests/test_gpu_reach_forest.py::test_dense_store"
_STABLE = "tests/test_gpu_stable.py::test_dense_store"
_CONSENSUS = "tests/test_gpu_consensus.py::"
_CHIMERA = "tests/test_gpu_chimeras.py::test_kernels_by_name_and_statistics"
_ASSIGN = "tests/test_gpu_assign.py::test_every_shape_equals_the_model"
_CLASSIFY = "tests/test_gpu_classify.py::test_every_shape_equals_the_model"
_SUBSET = "tests/test_gpu_subset.py::test_kernels_by_name"

# namespace -> {kernel: the GPU test that runs it}
NAMESPACES = {
    # every self-join builds records and filters; the inverse order map is asserted by name
    "smafa_join::": {
        "smafa_join::store_records_kernel": _SELF_JOIN + "test_self_pairs_equal_brute_force",
        "smafa_join::inverse_order_kernel": _SELF_JOIN + "test_stale_state_after_push",
        "smafa_join::join_filter_kernel": _SELF_JOIN + "test_every_engine_one_answer",
    },
    "smafa_cc::": {
        "smafa_cc::init_labels_kernel": _COMPONENTS + "test_dense_store",
        "smafa_cc::link_rows_kernel": _COMPONENTS + "test_dense_store",
        "smafa_cc::flatten_labels_kernel": _COMPONENTS + "test_against_the_join_and_the_query_path_at_scale",
    },
    "smafa_lv::": {
        "smafa_lv::init_levels_kernel": _LEVELS + "test_dense_store",
        "smafa_lv::hook_levels_kernel": _LEVELS + "test_dense_store",
        "smafa_lv::flatten_levels_kernel": _LEVELS + "test_nesting_and_the_components_call_at_scale",
    },
    "smafa_dn::": {
        "smafa_dn::init_density_kernel": _DENSITY + "test_dense_store",
        "smafa_dn::count_keep_kernel": _DENSITY + "test_dense_store",
        "smafa_dn::link_cores_kernel": _DENSITY + "test_one_join_against_two_joins",
        "smafa_dn::flatten_density_kernel": _DENSITY + "test_dense_store",
    },
    "smafa_pk::": {
        "smafa_pk::init_peaks_kernel": _PEAKS + "test_dense_store",
        "smafa_pk::weigh_keep_kernel": _PEAKS + "test_dense_store",
        "smafa_pk::climb_kernel": _PEAKS + "test_one_join_against_two_joins",
        "smafa_pk::crown_kernel": _PEAKS + "test_edges_and_errors",
        "smafa_pk::settle_kernel": _PEAKS + "test_dense_store",
        "smafa_pk::jump_kernel": _PEAKS + "test_climb_chain",
    },
    "smafa_nb::": {
        "smafa_nb::mirror_pack_kernel": _NEIGHBOURS,
        "smafa_nb::row_bounds_kernel": _NEIGHBOURS,
        "smafa_nb::cut_degrees_kernel": _NEIGHBOURS,
        "smafa_nb::emit_kernel": _NEIGHBOURS,
    },
    "smafa_dl::": {
        "smafa_dl::gather_records_kernel": _DELTA + "test_every_engine_one_answer",
        "smafa_dl::delta_filter_kernel": _DELTA + "test_every_engine_one_answer",
        "smafa_dl::seed_parents_kernel": _DELTA + "test_components_update_over_three_appends",
    },
    "smafa_sf::": {
        "smafa_sf::init_forest_kernel": _FOREST + "test_dense_store",
        "smafa_sf::keep_pairs_kernel": _FOREST + "test_dense_store",
        "smafa_sf::span_edges_kernel": _FOREST + "test_dense_store",
        "smafa_sf::star_roots_kernel": _FOREST + "test_edges_and_errors",
    },
    "smafa_mr::": {
        "smafa_mr::tally_keep_kernel": _REACH,
        "smafa_mr::core_dist_kernel": _REACH,
        "smafa_mr::span_reach_kernel": _REACH,
    },
    "smafa_st::": {
        "smafa_st::unite_class_kernel": _STABLE,
        "smafa_st::snapshot_kernel": _STABLE,
        "smafa_st::census_kernel": _STABLE,
        "smafa_st::adopt_kernel": _STABLE,
        "smafa_st::excess_kernel": _STABLE,
        "smafa_st::choose_kernel": _STABLE,
        "smafa_st::assign_kernel": _STABLE,
    },
    "consensus::": {
        "consensus::mark_groups_kernel": _CONSENSUS + "test_dense_store",
        "consensus::group_ids_kernel": _CONSENSUS + "test_dense_store",
        "consensus::group_keys_kernel": _CONSENSUS + "test_dense_store",
        "consensus::segment_bounds_kernel": _CONSENSUS + "test_dense_store",
        "consensus::tally_vote_kernel<2>": _CONSENSUS + "test_dense_store",
        "consensus::vote_tables_kernel<2>": _CONSENSUS + "test_store_states",
        "consensus::tally_vote_kernel<3>": _CONSENSUS + "test_store_states",
        "consensus::vote_tables_kernel<3>": _CONSENSUS + "test_store_states",
        "consensus::tally_vote_kernel<5>": _CONSENSUS + "test_every_shape_equals_the_model",
        "consensus::vote_tables_kernel<5>": _CONSENSUS + "test_chunks_of_64",
        "consensus::measure_kernel": _CONSENSUS + "test_dense_store",
        "consensus::finish_groups_kernel": _CONSENSUS + "test_dense_store",
    },
    "chimera::": {
        "chimera::init_sides_kernel": _CHIMERA,
        "chimera::offer_sides_kernel": _CHIMERA,
        "chimera::verdict_kernel": _CHIMERA,
    },
    "assign::": {
        "assign::init_kernel": _ASSIGN,
        "assign::best_kernel": _ASSIGN,
        "assign::bin_kernel": _ASSIGN,
        "assign::heads_kernel": _ASSIGN,
        "assign::fold_kernel": _ASSIGN,
    },
    "classify::": {
        "classify::start_kernel": _CLASSIFY,
        "classify::agree_kernel": _CLASSIFY,
        "classify::key_kernel": _CLASSIFY,
    },
    "subset::": {
        "subset::keep_flags_kernel": _SUBSET,
        "subset::run_ends_kernel": _SUBSET,
        "subset::move_rows_kernel": _SUBSET,
        "subset::unpack_rows_kernel<2>": _SUBSET,
        "subset::unpack_rows_kernel<3>": _SUBSET,
        "subset::unpack_rows_kernel<5>": _SUBSET,
    },
}

# what the radix sorts, the scans and the sums bring in; nothing is pinned inside it
LIBRARY_NAMESPACES = ("rocprim::",)

# word -> the one namespace whose kernel names may carry it.  Anywhere else in the code object — smafa::, the other owners and
# the library's kernels included, where a functor or a type handed to a sort would show — it is an offender.
RESERVED = {
    "label": "smafa_cc::", "link_rows": "smafa_cc::",
    "levels": "smafa_lv::", "hook": "smafa_lv::",
    "density": "smafa_dn::", "count_keep": "smafa_dn::", "link_cores": "smafa_dn::",
    "peaks": "smafa_pk::", "weigh_keep": "smafa_pk::", "climb": "smafa_pk::", "crown": "smafa_pk::", "settle": "smafa_pk::",
    "jump": "smafa_pk::",
    "mirror_pack": "smafa_nb::", "row_bounds": "smafa_nb::", "cut_degrees": "smafa_nb::", "emit_kernel": "smafa_nb::",
    "gather_records": "smafa_dl::", "delta_filter": "smafa_dl::", "seed_parents": "smafa_dl::",
}

# kernels whose GPU test builds the template argument at run time ("...<%d>" % planes), so its text holds the stem only
STEM_ONLY = {"subset::unpack_rows_kernel<2>", "subset::unpack_rows_kernel<3>", "subset::unpack_rows_kernel<5>"}

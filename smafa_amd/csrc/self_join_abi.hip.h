// self_join_abi.hip.h — the C ABI of the self-join: the twenty-four smafa_db_self_* entry points, twelve calls in two forms each — and,
// last, the two forms of smafa_db_consensus, which takes labels such as theirs and shares their host form.  The
// *_launch form checks its arguments and hands the caller's device pointers to the call of self_join.hip.h.  The host form checks
// the same, then runs the same call on the handle's own buffers and copies the results out: pairs_to_host for the two pair
// lists, HostForm for the ten calls that return arrays and counters.
// A new call: its two entry points here, built from self_args / HostForm / trim; what it checks beyond self_args, and where it zeroes
// its outputs among its checks, is its own (the order is part of the contract: tests hold what a failing check leaves untouched).
// Included once by engine.hip, inside extern "C", behind self_join.hip.h.
#pragma once

static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "counters and offsets are copied to the caller as they lie");

// ---- argument checks: `who` is the entry point, the name is the argument's
static int missing(const char *who, const char *name) { return set_error(SMAFA_ERR_INVALID, "%s: NULL %s", who, name); }

// what twenty-two of the entry points check first, in this order: the handle, two arguments, the bound (`needs`: the bound's text)
static int self_args(const char *who, const smafa_db *db, bool has_a, const char *a, bool has_b, const char *b, uint32_t max_div,
                     const char *needs) {
    if (!db) return missing(who, "handle");
    if (!has_a) return missing(who, a);
    if (!has_b) return missing(who, b);
    if (max_div == SMAFA_NONE) return set_error(SMAFA_ERR_INVALID, "%s: %s (max_div)", who, needs);
    return SMAFA_OK;
}
static int pair_args(const char *who, const smafa_db *db, const void *count, const void *rows, uint64_t cap, uint32_t max_div) {
    return self_args(who, db, count, "count", rows || !cap, "row buffer with a capacity", max_div, "a self-join needs a bound");
}
static int first_row_arg(const char *who, const smafa_db *db, uint64_t first_row) {
    if (first_row <= db->n) return SMAFA_OK;
    return set_error(SMAFA_ERR_INVALID, "%s: first_row %llu, the store has %llu subjects", who, (unsigned long long)first_row,
                     (unsigned long long)db->n);
}
static int labels_cap_arg(const char *who, const smafa_db *db, uint64_t cap) {
    if (cap >= db->n) return SMAFA_OK;
    return set_error(SMAFA_ERR_INVALID, "%s: labels holds %llu entries, the store has %llu subjects", who, (unsigned long long)cap,
                     (unsigned long long)db->n);
}
static int radius_arg(const char *who, uint32_t radius, uint32_t max_div) {
    if (radius == SMAFA_NONE || radius <= max_div) return SMAFA_OK;
    return set_error(SMAFA_ERR_INVALID, "%s: radius %u is larger than max_div %u", who, radius, max_div);
}
// the checks the two neighbours calls share (nothing is written before they pass)
static int neighbours_args(const char *who, const smafa_db *db, uint32_t max_div, uint32_t max_num_hits, const void *offsets,
                           const void *neighbours, uint64_t cap, const void *total, const char *total_name) {
    if (!offsets) return missing(who, "offsets");
    if (!total) return missing(who, total_name);
    if (!neighbours && cap) return missing(who, "neighbours with a capacity");
    if (max_div == SMAFA_NONE) return set_error(SMAFA_ERR_INVALID, "%s: neighbour lists need a bound (max_div)", who);
    if (max_num_hits == 0) return set_error(SMAFA_ERR_INVALID, "%s: max_num_hits is 0 (SMAFA_NONE: no cut)", who);
    if (!db) return missing(who, "handle");  // (last: the checks above need no handle, and no device)
    return SMAFA_OK;
}

// ---- the two host forms
// The host form of a pair-list call: `join` fills J.out (room rows: cap, or all_pairs if that is less) and J.cnt on the device;
// the count comes back, then — where it fits cap — the rows, ordered (query, dist, subject) on the device or the host.
static int pairs_to_host(smafa_db *db, uint64_t all_pairs, smafa_hit *out, uint64_t cap, uint64_t *n_out,
                         const std::function<int(smafa_hit *, uint64_t, unsigned long long *)> &join) {
    RC_TRY(use_device(db));
    auto &J = db->join;
    const uint64_t room = std::min<uint64_t>(cap, all_pairs);
    RC_TRY(J.out.ensure(std::max<uint64_t>(room, 1) * sizeof(smafa_hit)));
    RC_TRY(J.cnt.ensure(sizeof(unsigned long long)));
    RC_TRY(join(J.out.as<smafa_hit>(), room, J.cnt.as<unsigned long long>()));
    unsigned long long count = 0;
    HIP_TRY(hipMemcpyAsync(&count, J.cnt.p, sizeof count, hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    *n_out = count;
    if (count > cap)
        return set_error(SMAFA_ERR_CAPACITY, "hit buffer too small: %llu rows needed, capacity %llu", count, (unsigned long long)cap);
    if (count) {
        bool sorted = false;
        if (count >= 4096) RC_TRY(sort_rows_on_device(db, count, 0, (uint32_t)db->n, &sorted, J.out.as<smafa_hit>()));
        HIP_TRY(hipMemcpyAsync(out, J.out.p, count * sizeof(smafa_hit), hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        if (!sorted) std::sort(out, out + count, hit_less);
    }
    trim({&J.out, &db->hits});
    trim_together(db->keys_a, {&db->keys_b, &db->sort_tmp});
    return SMAFA_OK;
}

// The host form of a call that returns arrays and counters.  `stage` gives J.out the bytes of the arrays and J.cnt the counters;
// the call's device form runs on them; `fetch` enqueues one copy to the caller's memory (no taker, or nothing to take: no copy)
// and `wait` ends a group of copies.  What is released behind the call is the call's own list (trim).
struct HostForm {
    smafa_db *db;
    int stage(uint64_t out_bytes, uint64_t counters) const {
        RC_TRY(use_device(db));
        RC_TRY(db->join.out.ensure(out_bytes));
        return db->join.cnt.ensure(counters * sizeof(unsigned long long));
    }
    unsigned long long *cnt() const { return db->join.cnt.as<unsigned long long>(); }
    int fetch(void *to, const void *from, uint64_t bytes) const {
        if (to && bytes) HIP_TRY(hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToHost, db->stream));
        return SMAFA_OK;
    }
    int wait() const {
        HIP_TRY(hipStreamSynchronize(db->stream));
        return SMAFA_OK;
    }
};

// ---- pairs
int smafa_db_self_launch(smafa_db *db, uint32_t max_div, void *d_hits, uint64_t cap, void *d_count) try {
    RC_TRY(pair_args("smafa_db_self_launch", db, d_count, d_hits, cap, max_div));
    return join_pairs(db, max_div, (smafa_hit *)d_hits, cap, (unsigned long long *)d_count);
} catch (...) {
    return smafa::exception_code("smafa_db_self_launch");
}

int smafa_db_self_hits(smafa_db *db, uint32_t max_div, smafa_hit *out, uint64_t cap, uint64_t *n_out) try {
    RC_TRY(pair_args("smafa_db_self_hits", db, n_out, out, cap, max_div));
    *n_out = 0;
    const uint64_t all_pairs = db->n < 2 ? 0 : db->n * (db->n - 1) / 2;
    return pairs_to_host(db, all_pairs, out, cap, n_out, [&](smafa_hit *d_hits, uint64_t room, unsigned long long *d_count) {
        return join_pairs(db, max_div, d_hits, room, d_count);
    });
} catch (...) {
    return smafa::exception_code("smafa_db_self_hits");
}

int smafa_db_self_since_launch(smafa_db *db, uint64_t first_row, uint32_t max_div, void *d_hits, uint64_t cap, void *d_count) try {
    RC_TRY(pair_args("smafa_db_self_since_launch", db, d_count, d_hits, cap, max_div));
    RC_TRY(first_row_arg("smafa_db_self_since_launch", db, first_row));
    return delta_pairs(db, (uint32_t)first_row, max_div, (smafa_hit *)d_hits, cap, (unsigned long long *)d_count);
} catch (...) {
    return smafa::exception_code("smafa_db_self_since_launch");
}

int smafa_db_self_hits_since(smafa_db *db, uint64_t first_row, uint32_t max_div, smafa_hit *out, uint64_t cap, uint64_t *n_out) try {
    RC_TRY(pair_args("smafa_db_self_hits_since", db, n_out, out, cap, max_div));
    *n_out = 0;
    RC_TRY(first_row_arg("smafa_db_self_hits_since", db, first_row));
    // pairs whose larger number is j: j of them, for every new row j
    const uint64_t all_pairs = (db->n - first_row) * (db->n + first_row - (db->n > first_row ? 1 : 0)) / 2;
    return pairs_to_host(db, all_pairs, out, cap, n_out, [&](smafa_hit *d_hits, uint64_t room, unsigned long long *d_count) {
        return delta_pairs(db, (uint32_t)first_row, max_div, d_hits, room, d_count);
    });
} catch (...) {
    return smafa::exception_code("smafa_db_self_hits_since");
}

// ---- components, and their update
int smafa_db_self_components_launch(smafa_db *db, uint32_t max_div, void *d_labels, void *d_n_components) try {
    RC_TRY(self_args("smafa_db_self_components_launch", db, d_labels, "labels", d_n_components, "count", max_div, "components need a bound"));
    return join_components(db, max_div, (uint32_t *)d_labels, (unsigned long long *)d_n_components);
} catch (...) {
    return smafa::exception_code("smafa_db_self_components_launch");
}

int smafa_db_self_components(smafa_db *db, uint32_t max_div, uint32_t *labels, uint64_t cap, uint64_t *n_components) try {
    RC_TRY(self_args("smafa_db_self_components", db, labels, "labels", n_components, "count", max_div, "components need a bound"));
    *n_components = 0;
    RC_TRY(labels_cap_arg("smafa_db_self_components", db, cap));
    const HostForm h{db};
    auto &J = db->join;
    RC_TRY(h.stage(std::max<uint64_t>(db->n, 1) * sizeof(uint32_t), 1));  // the labels on their way to the caller: 4 B per subject
    RC_TRY(join_components(db, max_div, J.out.as<uint32_t>(), h.cnt()));
    unsigned long long count = 0;
    RC_TRY(h.fetch(&count, h.cnt(), sizeof count));
    RC_TRY(h.fetch(labels, J.out.p, db->n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    *n_components = count;
    trim({&db->hits});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_components");
}

int smafa_db_self_components_update_launch(smafa_db *db, uint64_t first_row, uint32_t max_div, void *d_labels, void *d_n_components) try {
    RC_TRY(self_args("smafa_db_self_components_update_launch", db, d_labels, "labels", d_n_components, "count", max_div,
                     "components need a bound"));
    RC_TRY(first_row_arg("smafa_db_self_components_update_launch", db, first_row));
    return delta_components(db, (uint32_t)first_row, max_div, (uint32_t *)d_labels, (unsigned long long *)d_n_components);
} catch (...) {
    return smafa::exception_code("smafa_db_self_components_update_launch");
}

int smafa_db_self_components_update(smafa_db *db, uint64_t first_row, uint32_t max_div, uint32_t *labels, uint64_t cap,
                                    uint64_t *n_components) try {
    RC_TRY(self_args("smafa_db_self_components_update", db, labels, "labels", n_components, "count", max_div, "components need a bound"));
    *n_components = 0;
    RC_TRY(first_row_arg("smafa_db_self_components_update", db, first_row));
    RC_TRY(labels_cap_arg("smafa_db_self_components_update", db, cap));
    const HostForm h{db};
    auto &J = db->join;
    RC_TRY(h.stage(std::max<uint64_t>(db->n, 1) * sizeof(uint32_t), 1));  // the labels on their way in and out: 4 B per subject
    if (first_row) HIP_TRY(hipMemcpyAsync(J.out.p, labels, first_row * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    RC_TRY(delta_components(db, (uint32_t)first_row, max_div, J.out.as<uint32_t>(), h.cnt()));  // (a failure: labels[] is as it came)
    unsigned long long count = 0;
    RC_TRY(h.fetch(&count, h.cnt(), sizeof count));
    RC_TRY(h.fetch(labels, J.out.p, db->n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    *n_components = count;
    trim({&db->hits});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_components_update");
}

// ---- levels
int smafa_db_self_levels_launch(smafa_db *db, uint32_t max_div, void *d_labels, void *d_n_components) try {
    RC_TRY(self_args("smafa_db_self_levels_launch", db, d_labels, "labels", d_n_components, "count", max_div, "levels need a bound"));
    return join_levels(db, max_div, (uint32_t *)d_labels, (unsigned long long *)d_n_components);
} catch (...) {
    return smafa::exception_code("smafa_db_self_levels_launch");
}

int smafa_db_self_levels(smafa_db *db, uint32_t max_div, uint32_t *labels, uint64_t cap, uint64_t *n_components) try {
    RC_TRY(self_args("smafa_db_self_levels", db, labels, "labels", n_components, "count", max_div, "levels need a bound"));
    const uint64_t T = (uint64_t)max_div + 1u;
    // (n_subjects < 2^32 and T <= 2^32 - 1: the product cannot wrap)
    if (cap < T * db->n)
        return set_error(SMAFA_ERR_INVALID, "smafa_db_self_levels: labels holds %llu entries, %llu levels of %llu subjects need %llu",
                         (unsigned long long)cap, (unsigned long long)T, (unsigned long long)db->n, (unsigned long long)(T * db->n));
    std::fill(n_components, n_components + T, (uint64_t)0);
    const HostForm h{db};
    auto &J = db->join;
    RC_TRY(h.stage(std::max<uint64_t>(T * db->n, 1) * sizeof(uint32_t), T));  // the labels on their way to the caller
    RC_TRY(join_levels(db, max_div, J.out.as<uint32_t>(), h.cnt()));
    RC_TRY(h.fetch(n_components, h.cnt(), T * sizeof(uint64_t)));
    RC_TRY(h.fetch(labels, J.out.p, T * db->n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    trim({&db->hits, &J.out, &J.parent});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_levels");
}

// ---- forest
int smafa_db_self_forest_launch(smafa_db *db, uint32_t max_div, void *d_edges, void *d_level_ends) try {
    RC_TRY(self_args("smafa_db_self_forest_launch", db, d_edges, "edges", d_level_ends, "level_ends", max_div, "a forest needs a bound"));
    return join_forest(db, max_div, (smafa_hit *)d_edges, (unsigned long long *)d_level_ends);
} catch (...) {
    return smafa::exception_code("smafa_db_self_forest_launch");
}

int smafa_db_self_forest(smafa_db *db, uint32_t max_div, smafa_hit *edges, uint64_t cap, uint64_t *level_ends) try {
    RC_TRY(self_args("smafa_db_self_forest", db, edges, "edges", level_ends, "level_ends", max_div, "a forest needs a bound"));
    const uint64_t T = (uint64_t)max_div + 1u, room = db->n ? db->n - 1 : 0;
    if (cap < room)  // (nothing is written, level_ends included)
        return set_error(SMAFA_ERR_INVALID, "smafa_db_self_forest: edges holds %llu rows, a forest of %llu subjects may need %llu",
                         (unsigned long long)cap, (unsigned long long)db->n, (unsigned long long)room);
    std::fill(level_ends, level_ends + T, (uint64_t)0);
    const HostForm h{db};
    auto &J = db->join;
    RC_TRY(h.stage(std::max<uint64_t>(room, 1) * sizeof(smafa_hit), T));  // the edges on their way to the caller
    RC_TRY(join_forest(db, max_div, J.out.as<smafa_hit>(), h.cnt()));
    RC_TRY(h.fetch(level_ends, h.cnt(), T * sizeof(uint64_t)));
    RC_TRY(h.wait());  // (a wait of its own: the edge total decides the second copy)
    const uint64_t total = level_ends[T - 1];
    if (total > room) return set_error(SMAFA_ERR_DEVICE, "smafa_db_self_forest: %llu edges among %llu subjects are no forest",
                                       (unsigned long long)total, (unsigned long long)db->n);
    RC_TRY(h.fetch(edges, J.out.p, total * sizeof(smafa_hit)));
    RC_TRY(h.wait());
    // a level's edges arrive in any order: (query, subject) inside each level, so that a given forest prints one way
    for (uint64_t t = 0, begin = 0; t < T && begin < total; begin = level_ends[t++])
        std::sort(edges + begin, edges + level_ends[t], [](const smafa_hit &x, const smafa_hit &y) {
            return x.query != y.query ? x.query < y.query : x.subject < y.subject;
        });
    trim({&db->hits, &J.kept});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_forest");
}

// ---- mutual-reachability forest
int smafa_db_self_reach_forest_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, void *d_edges, void *d_level_ends,
                                      void *d_cores) try {
    RC_TRY(self_args("smafa_db_self_reach_forest_launch", db, d_edges, "edges", d_level_ends, "level_ends", max_div,
                     "a reach forest needs a bound"));
    return join_reach_forest(db, max_div, std::max<uint32_t>(min_pts, 1u), (smafa_hit *)d_edges, (unsigned long long *)d_level_ends,
                             (uint32_t *)d_cores);
} catch (...) {
    return smafa::exception_code("smafa_db_self_reach_forest_launch");
}

int smafa_db_self_reach_forest(smafa_db *db, uint32_t max_div, uint32_t min_pts, smafa_hit *edges, uint64_t cap, uint64_t *level_ends,
                               uint32_t *cores) try {
    RC_TRY(self_args("smafa_db_self_reach_forest", db, edges, "edges", level_ends, "level_ends", max_div, "a reach forest needs a bound"));
    const uint64_t T = (uint64_t)max_div + 1u, n = db->n, room = n ? n - 1 : 0;
    if (cap < room)  // (nothing is written, level_ends and cores included)
        return set_error(SMAFA_ERR_INVALID, "smafa_db_self_reach_forest: edges holds %llu rows, a forest of %llu subjects may need %llu",
                         (unsigned long long)cap, (unsigned long long)n, (unsigned long long)room);
    std::fill(level_ends, level_ends + T, (uint64_t)0);
    const HostForm h{db};
    auto &J = db->join;
    // the edges, and the cores behind them, on their way to the caller: 12 B per edge, 4 B per subject
    const uint64_t edge_bytes = std::max<uint64_t>(room, 1) * sizeof(smafa_hit);
    RC_TRY(h.stage(edge_bytes + (cores ? n * sizeof(uint32_t) : 0), T));
    uint32_t *const d_cores = cores ? reinterpret_cast<uint32_t *>(J.out.as<char>() + edge_bytes) : nullptr;
    RC_TRY(join_reach_forest(db, max_div, std::max<uint32_t>(min_pts, 1u), J.out.as<smafa_hit>(), h.cnt(), d_cores));
    RC_TRY(h.fetch(level_ends, h.cnt(), T * sizeof(uint64_t)));
    RC_TRY(h.fetch(cores, d_cores, n * sizeof(uint32_t)));
    RC_TRY(h.wait());  // (a wait of its own: the edge total decides the next copy)
    const uint64_t total = level_ends[T - 1];
    if (total > room) return set_error(SMAFA_ERR_DEVICE, "smafa_db_self_reach_forest: %llu edges among %llu subjects are no forest",
                                       (unsigned long long)total, (unsigned long long)n);
    RC_TRY(h.fetch(edges, J.out.p, total * sizeof(smafa_hit)));
    RC_TRY(h.wait());
    // a level's edges arrive in any order: (query, subject) inside each level, so that a given forest prints one way
    for (uint64_t t = 0, begin = 0; t < T && begin < total; begin = level_ends[t++])
        std::sort(edges + begin, edges + level_ends[t], [](const smafa_hit &x, const smafa_hit &y) {
            return x.query != y.query ? x.query < y.query : x.subject < y.subject;
        });
    trim({&db->hits, &J.kept, &J.hist});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_reach_forest");
}

// ---- stable clusters
// min_cluster_size 0: min_pts, as min_pts 0 is 1
static uint32_t stable_min_size(uint32_t min_pts, uint32_t min_cluster_size) { return min_cluster_size ? min_cluster_size : std::max<uint32_t>(min_pts, 1u); }

int smafa_db_self_stable_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t min_cluster_size, void *d_labels, void *d_joined,
                                void *d_cores, uint64_t *n_clusters) try {
    RC_TRY(self_args("smafa_db_self_stable_launch", db, d_labels, "labels", n_clusters, "n_clusters", max_div, "stable clusters need a bound"));
    return join_stable(db, max_div, std::max<uint32_t>(min_pts, 1u), stable_min_size(min_pts, min_cluster_size), (uint32_t *)d_labels,
                       (uint32_t *)d_joined, (uint32_t *)d_cores, n_clusters);
} catch (...) {
    return smafa::exception_code("smafa_db_self_stable_launch");
}

int smafa_db_self_stable(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t min_cluster_size, uint32_t *labels, uint32_t *joined,
                         uint32_t *cores, uint64_t cap, uint64_t *n_clusters) try {
    RC_TRY(self_args("smafa_db_self_stable", db, labels, "labels", n_clusters, "n_clusters", max_div, "stable clusters need a bound"));
    RC_TRY(labels_cap_arg("smafa_db_self_stable", db, cap));  // (nothing is written, the count included)
    *n_clusters = 0;
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n;
    // the labels, and the joined levels and the cores behind them, on their way to the caller: 4 B x 3 per subject
    RC_TRY(h.stage(std::max<uint64_t>(n, 1) * 3u * sizeof(uint32_t), 1));
    uint32_t *const d_labels = J.out.as<uint32_t>();
    uint64_t count = 0;
    RC_TRY(join_stable(db, max_div, std::max<uint32_t>(min_pts, 1u), stable_min_size(min_pts, min_cluster_size), d_labels,
                       joined ? d_labels + n : nullptr, cores ? d_labels + 2 * n : nullptr, &count));
    RC_TRY(h.fetch(labels, d_labels, n * sizeof(uint32_t)));
    RC_TRY(h.fetch(joined, d_labels + n, n * sizeof(uint32_t)));
    RC_TRY(h.fetch(cores, d_labels + 2 * n, n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    *n_clusters = count;
    trim({&db->hits, &J.kept, &J.hist, &J.stable});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_stable");
}

// ---- density
int smafa_db_self_density_launch(smafa_db *db, uint32_t max_div, uint32_t min_pts, void *d_labels, void *d_degrees,
                                 void *d_counts) try {
    RC_TRY(self_args("smafa_db_self_density_launch", db, d_labels, "labels", d_counts, "counts", max_div, "density needs a bound"));
    return join_density(db, max_div, std::max<uint32_t>(min_pts, 1u), (uint32_t *)d_degrees, (uint32_t *)d_labels, (unsigned long long *)d_counts);
} catch (...) {
    return smafa::exception_code("smafa_db_self_density_launch");
}

int smafa_db_self_density(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t *labels, uint32_t *degrees, uint64_t cap,
                          uint64_t counts[3]) try {
    RC_TRY(self_args("smafa_db_self_density", db, labels, "labels", counts, "counts", max_div, "density needs a bound"));
    RC_TRY(labels_cap_arg("smafa_db_self_density", db, cap));  // (nothing is written, the counts included)
    counts[0] = counts[1] = counts[2] = 0;
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n;
    // the labels, and the degrees behind them, on their way to the caller: 4 B (8 B) per subject
    RC_TRY(h.stage(std::max<uint64_t>(n, 1) * (degrees ? 2u : 1u) * sizeof(uint32_t), 3));
    uint32_t *const d_labels = J.out.as<uint32_t>();
    RC_TRY(join_density(db, max_div, std::max<uint32_t>(min_pts, 1u), degrees ? d_labels + n : nullptr, d_labels, h.cnt()));
    RC_TRY(h.fetch(counts, h.cnt(), 3 * sizeof(uint64_t)));
    RC_TRY(h.fetch(labels, d_labels, n * sizeof(uint32_t)));
    RC_TRY(h.fetch(degrees, d_labels + n, n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    trim({&db->hits, &J.kept});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_density");
}

// ---- peaks
int smafa_db_self_peaks_launch(smafa_db *db, uint32_t max_div, uint32_t radius, void *d_labels, void *d_parents, void *d_weights,
                               void *d_n_peaks) try {
    RC_TRY(self_args("smafa_db_self_peaks_launch", db, d_labels, "labels", d_n_peaks, "n_peaks", max_div, "peaks need a bound"));
    RC_TRY(radius_arg("smafa_db_self_peaks_launch", radius, max_div));
    return join_peaks(db, max_div, radius == SMAFA_NONE ? max_div : radius, (uint32_t *)d_labels, (uint32_t *)d_parents, (uint32_t *)d_weights,
                      (unsigned long long *)d_n_peaks);
} catch (...) {
    return smafa::exception_code("smafa_db_self_peaks_launch");
}

int smafa_db_self_peaks(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t *labels, uint32_t *parents, uint32_t *weights,
                        uint64_t cap, uint64_t *n_peaks) try {
    RC_TRY(self_args("smafa_db_self_peaks", db, labels, "labels", n_peaks, "n_peaks", max_div, "peaks need a bound"));
    RC_TRY(radius_arg("smafa_db_self_peaks", radius, max_div));
    RC_TRY(labels_cap_arg("smafa_db_self_peaks", db, cap));  // (nothing is written, the count included)
    *n_peaks = 0;
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n;
    // the labels, and the parents and weights behind them, on their way to the caller: 4 B x 3 per subject
    RC_TRY(h.stage(std::max<uint64_t>(n, 1) * 3u * sizeof(uint32_t), 1));
    uint32_t *const d_labels = J.out.as<uint32_t>();
    RC_TRY(join_peaks(db, max_div, radius == SMAFA_NONE ? max_div : radius, d_labels, parents ? d_labels + n : nullptr,
                      weights ? d_labels + 2 * n : nullptr, h.cnt()));
    unsigned long long count = 0;
    RC_TRY(h.fetch(&count, h.cnt(), sizeof count));
    RC_TRY(h.fetch(labels, d_labels, n * sizeof(uint32_t)));
    RC_TRY(h.fetch(parents, d_labels + n, n * sizeof(uint32_t)));
    RC_TRY(h.fetch(weights, d_labels + 2 * n, n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    *n_peaks = count;
    trim({&db->hits, &J.kept});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_peaks");
}

// ---- peaks with given weights
// behind self_args and radius_arg: the weights, unless the store is empty
int smafa_db_self_peaks_weighted_launch(smafa_db *db, uint32_t max_div, uint32_t radius, const void *d_weights_in, void *d_labels, void *d_parents,
                                        void *d_weights, void *d_n_peaks) try {
    const char *const who = "smafa_db_self_peaks_weighted_launch";
    RC_TRY(self_args(who, db, d_labels, "labels", d_n_peaks, "n_peaks", max_div, "peaks need a bound"));
    RC_TRY(radius_arg(who, radius, max_div));
    if (!d_weights_in && db->n) return missing(who, "weights_in");
    return join_peaks_weighted(db, who, max_div, radius == SMAFA_NONE ? max_div : radius, (const uint32_t *)d_weights_in, (uint32_t *)d_labels,
                               (uint32_t *)d_parents, (uint32_t *)d_weights, (unsigned long long *)d_n_peaks);
} catch (...) {
    return smafa::exception_code("smafa_db_self_peaks_weighted_launch");
}

int smafa_db_self_peaks_weighted(smafa_db *db, uint32_t max_div, uint32_t radius, const uint32_t *weights_in, uint32_t *labels, uint32_t *parents,
                                 uint32_t *weights, uint64_t cap, uint64_t *n_peaks) try {
    const char *const who = "smafa_db_self_peaks_weighted";
    RC_TRY(self_args(who, db, labels, "labels", n_peaks, "n_peaks", max_div, "peaks need a bound"));
    RC_TRY(radius_arg(who, radius, max_div));
    if (!weights_in && db->n) return missing(who, "weights_in");
    RC_TRY(labels_cap_arg(who, db, cap));  // (nothing is written, the count included)
    *n_peaks = 0;
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n;
    // the labels, the parents and weights behind them on their way to the caller, and the caller's weights on their way in
    RC_TRY(h.stage(std::max<uint64_t>(n, 1) * 4u * sizeof(uint32_t), 1));
    uint32_t *const d_labels = J.out.as<uint32_t>(), *const d_in = d_labels + 3 * n;
    if (n) HIP_TRY(hipMemcpyAsync(d_in, weights_in, n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    RC_TRY(join_peaks_weighted(db, who, max_div, radius == SMAFA_NONE ? max_div : radius, d_in, d_labels, parents ? d_labels + n : nullptr,
                               weights ? d_labels + 2 * n : nullptr, h.cnt()));
    unsigned long long count = 0;
    RC_TRY(h.fetch(&count, h.cnt(), sizeof count));
    RC_TRY(h.fetch(labels, d_labels, n * sizeof(uint32_t)));
    RC_TRY(h.fetch(parents, d_labels + n, n * sizeof(uint32_t)));
    RC_TRY(h.fetch(weights, d_labels + 2 * n, n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    *n_peaks = count;
    trim({&db->hits, &J.kept});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_peaks_weighted");
}

// ---- chimeras
// behind self_args: the radius, then the fold (nothing is written before they pass)
static int chimera_args(const char *who, uint32_t radius, uint32_t max_div, uint32_t min_fold) {
    RC_TRY(radius_arg(who, radius, max_div));
    if (min_fold == 0) return set_error(SMAFA_ERR_INVALID, "%s: min_fold is 0 (1: any heavier row may be a parent)", who);
    return SMAFA_OK;
}

int smafa_db_self_chimeras_launch(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t min_fold, const void *d_weights_in, void *d_flags,
                                  void *d_left_parent, void *d_left_len, void *d_right_parent, void *d_right_len, void *d_weights,
                                  void *d_n_chimeras) try {
    RC_TRY(self_args("smafa_db_self_chimeras_launch", db, d_flags, "flags", d_n_chimeras, "n_chimeras", max_div, "a chimera check needs a bound"));
    RC_TRY(chimera_args("smafa_db_self_chimeras_launch", radius, max_div, min_fold));
    return join_chimeras(db, max_div, radius == SMAFA_NONE ? max_div : radius, min_fold, (const uint32_t *)d_weights_in, (uint32_t *)d_flags,
                         (uint32_t *)d_left_parent, (uint32_t *)d_left_len, (uint32_t *)d_right_parent, (uint32_t *)d_right_len,
                         (uint32_t *)d_weights, (unsigned long long *)d_n_chimeras);
} catch (...) {
    return smafa::exception_code("smafa_db_self_chimeras_launch");
}

int smafa_db_self_chimeras(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t min_fold, const uint32_t *weights_in, uint32_t *flags,
                           uint32_t *left_parent, uint32_t *left_len, uint32_t *right_parent, uint32_t *right_len, uint32_t *weights,
                           uint64_t cap, uint64_t *n_chimeras) try {
    RC_TRY(self_args("smafa_db_self_chimeras", db, flags, "flags", n_chimeras, "n_chimeras", max_div, "a chimera check needs a bound"));
    RC_TRY(chimera_args("smafa_db_self_chimeras", radius, max_div, min_fold));
    if (cap < db->n)  // (nothing is written, the count included)
        return set_error(SMAFA_ERR_INVALID, "smafa_db_self_chimeras: cap: flags holds %llu entries, the store has %llu subjects",
                         (unsigned long long)cap, (unsigned long long)db->n);
    *n_chimeras = 0;
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n;
    // the flags, the five optional arrays behind them on their way to the caller and the caller's weights on their way in: 4 B x 7
    // per subject
    RC_TRY(h.stage(std::max<uint64_t>(n, 1) * 7u * sizeof(uint32_t), 1));
    uint32_t *const d_flags = J.out.as<uint32_t>(), *const d_in = d_flags + 6 * n;
    uint32_t *const taker[5] = {left_parent, left_len, right_parent, right_len, weights};
    uint32_t *d_out[5];
    for (int k = 0; k < 5; k++) d_out[k] = taker[k] ? d_flags + (uint64_t)(k + 1) * n : nullptr;
    if (weights_in && n) HIP_TRY(hipMemcpyAsync(d_in, weights_in, n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    RC_TRY(join_chimeras(db, max_div, radius == SMAFA_NONE ? max_div : radius, min_fold, weights_in ? d_in : nullptr, d_flags, d_out[0],
                         d_out[1], d_out[2], d_out[3], d_out[4], h.cnt()));
    unsigned long long count = 0;
    RC_TRY(h.fetch(&count, h.cnt(), sizeof count));
    RC_TRY(h.fetch(flags, d_flags, n * sizeof(uint32_t)));
    for (int k = 0; k < 5; k++) RC_TRY(h.fetch(taker[k], d_out[k], n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    *n_chimeras = count;
    trim({&db->hits, &J.kept});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_self_chimeras");
}

// ---- neighbours
int smafa_db_self_neighbours_launch(smafa_db *db, uint32_t max_div, uint32_t max_num_hits, void *d_offsets, void *d_neighbours,
                                    void *d_dists, uint64_t cap, void *d_total) try {
    RC_TRY(neighbours_args("smafa_db_self_neighbours_launch", db, max_div, max_num_hits, d_offsets, d_neighbours, cap, d_total, "total"));
    return join_neighbours(db, max_div, max_num_hits, (unsigned long long *)d_offsets, (uint32_t *)d_neighbours, (uint32_t *)d_dists, cap,
                           (unsigned long long *)d_total);
} catch (...) {
    return smafa::exception_code("smafa_db_self_neighbours_launch");
}

int smafa_db_self_neighbours(smafa_db *db, uint32_t max_div, uint32_t max_num_hits, uint64_t *offsets, uint32_t *neighbours,
                             uint32_t *dists, uint64_t cap, uint64_t *n_out) try {
    RC_TRY(neighbours_args("smafa_db_self_neighbours", db, max_div, max_num_hits, offsets, neighbours, cap, n_out, "n_out"));
    *n_out = 0;
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n;
    // no row lists more than the others, or than the cut: beyond that a larger capacity buys nothing
    const uint64_t room = std::min<uint64_t>(cap, n < 2 ? 0 : n * std::min<uint64_t>(n - 1, max_num_hits));
    // the offsets, the neighbours and the distances behind them, on their way to the caller
    RC_TRY(h.stage((n + 1) * sizeof(uint64_t) + room * (dists ? 2u : 1u) * sizeof(uint32_t), 1));
    unsigned long long *const d_offsets = J.out.as<unsigned long long>();
    uint32_t *const d_neighbours = reinterpret_cast<uint32_t *>(d_offsets + n + 1), *const d_dists = dists ? d_neighbours + room : nullptr;
    const int rc = join_neighbours(db, max_div, max_num_hits, d_offsets, d_neighbours, d_dists, room, h.cnt());
    if (rc && rc != SMAFA_ERR_CAPACITY) return rc;
    unsigned long long total = 0;
    RC_TRY(h.fetch(&total, h.cnt(), sizeof total));
    RC_TRY(h.fetch(offsets, d_offsets, (n + 1) * sizeof(uint64_t)));
    if (!rc) {
        RC_TRY(h.fetch(neighbours, d_neighbours, total * sizeof(uint32_t)));
        RC_TRY(h.fetch(dists, d_dists, total * sizeof(uint32_t)));
    }
    RC_TRY(h.wait());
    *n_out = total;
    if (rc)  // (join_neighbours saw `room`; the text names the capacity the caller gave)
        set_error(SMAFA_ERR_CAPACITY, "neighbour lists too small: %llu entries needed, capacity %llu", total, (unsigned long long)cap);
    trim({&J.out, &db->hits, &J.entries});
    trim_together(db->keys_a, {&db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp});
    return rc;  // (SMAFA_ERR_CAPACITY: its text stands, the offsets and *n_out are written, the lists are not)
} catch (...) {
    return smafa::exception_code("smafa_db_self_neighbours");
}

// ---- consensus (no bound, no join: the caller's labels and the store's planes)
// handle, labels, n_clusters, then the three arrays a capacity asks for; nothing is written before they pass
static int consensus_args(const char *who, const smafa_db *db, const void *labels, const void *n_clusters, const void *ids, const void *sizes,
                          const void *codes, uint64_t cap) {
    if (!db) return missing(who, "handle");
    if (!labels) return missing(who, "labels");
    if (!n_clusters) return missing(who, "n_clusters");
    if (cap && !ids) return missing(who, "ids with a capacity");
    if (cap && !sizes) return missing(who, "sizes with a capacity");
    if (cap && !codes) return missing(who, "codes with a capacity");
    return SMAFA_OK;
}

int smafa_db_consensus_launch(smafa_db *db, const void *d_labels, void *d_ids, void *d_sizes, void *d_codes, void *d_nearest, void *d_div,
                              uint64_t cap_clusters, uint64_t *n_clusters) try {
    RC_TRY(consensus_args("smafa_db_consensus_launch", db, d_labels, n_clusters, d_ids, d_sizes, d_codes, cap_clusters));
    return join_consensus(db, "smafa_db_consensus_launch", (const uint32_t *)d_labels, (uint32_t *)d_ids, (uint32_t *)d_sizes, (uint8_t *)d_codes,
                          (uint32_t *)d_nearest, (uint32_t *)d_div, cap_clusters, n_clusters);
} catch (...) {
    return smafa::exception_code("smafa_db_consensus_launch");
}

int smafa_db_consensus(smafa_db *db, const uint32_t *labels, uint32_t *ids, uint32_t *sizes, uint8_t *codes, uint32_t *nearest, uint32_t *div,
                       uint64_t cap_clusters, uint64_t *n_clusters) try {
    RC_TRY(consensus_args("smafa_db_consensus", db, labels, n_clusters, ids, sizes, codes, cap_clusters));
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n, L = db->L, room = std::min<uint64_t>(cap_clusters, n);  // no more clusters than rows
    // the labels on their way in, and behind them div, ids, sizes, nearest (4 B each) and the codes (L bytes per cluster) on their way out
    RC_TRY(h.stage(std::max<uint64_t>((2u * n + 3u * room) * sizeof(uint32_t) + room * L, 1), 0));
    uint32_t *const d_labels = J.out.as<uint32_t>(), *const d_div = d_labels + n, *const d_ids = d_div + n, *const d_sizes = d_ids + room;
    uint32_t *const d_nearest = d_sizes + room;
    uint8_t *const d_codes = reinterpret_cast<uint8_t *>(d_nearest + room);
    if (n) HIP_TRY(hipMemcpyAsync(d_labels, labels, n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    uint64_t count = 0;
    const int rc = join_consensus(db, "smafa_db_consensus", d_labels, d_ids, d_sizes, d_codes, nearest ? d_nearest : nullptr, div ? d_div : nullptr,
                                  cap_clusters, &count);
    if (rc && rc != SMAFA_ERR_CAPACITY) return rc;  // (nothing is written, the count included)
    *n_clusters = count;
    if (rc) return rc;  // SMAFA_ERR_CAPACITY: the count alone
    RC_TRY(h.fetch(ids, d_ids, count * sizeof(uint32_t)));
    RC_TRY(h.fetch(sizes, d_sizes, count * sizeof(uint32_t)));
    RC_TRY(h.fetch(codes, d_codes, count * L));
    RC_TRY(h.fetch(nearest, d_nearest, count * sizeof(uint32_t)));
    if (n) RC_TRY(h.fetch(div, d_div, n * sizeof(uint32_t)));
    RC_TRY(h.wait());
    trim({&J.out});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_consensus");
}

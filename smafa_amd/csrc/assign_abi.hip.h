// assign_abi.hip.h — the abundance table of a resident store: its call (assign_reads) and the two smafa_db_assign entry points.
// A read-table call (read_table.hip.h: the opening, the span loop, the table's tail, the host form): the reads are a query set of
// the caller's, scanned span by span in the tightening mode (k = 1), and the call's own kernels (assign.hip.h) consume each span's
// list.  Included once by engine.hip, inside extern "C", behind read_table.hip.h.
#pragma once

// The call.  Every pointer is the device's; d_group_of, d_samples, d_weights, d_subject, d_dist, d_subject_counts: or nullptr;
// d_entries: cap entries (nullptr with cap = 0).  No words of its own in J.parent.
static int assign_reads(smafa_db *db, smafa_qset *qs, const char *who, uint32_t max_div, const uint32_t *d_group_of, const uint32_t *d_samples,
                        uint32_t n_samples, const uint32_t *d_weights, uint32_t *d_subject, uint32_t *d_dist, unsigned long long *d_subject_counts,
                        smafa_table_entry *d_entries, uint64_t cap, unsigned long long *d_totals) {
    auto &J = db->join;
    const uint64_t n = db->n;
    const dim3 block(256);
    ReadTable t{{db}, qs, who};
    RC_TRY(read_table_begin(t, "the table takes fewer than 2^31 reads per call", d_totals, 4, 0,
                            "table: best[], the subject counts and the totals initialised", "assign::init_kernel", [&] {
        hipLaunchKernelGGL(assign::init_kernel, list_grid(std::max<uint64_t>(std::max<uint64_t>(t.m, d_subject_counts ? n : 0), 4)), block, 0,
                           db->stream, t.best, (uint64_t)t.m, d_subject_counts, n, d_totals);
    }));
    const uint32_t m = t.m;
    if (m == 0) return SMAFA_OK;
    // ---- the spans: each read's rows at its minimum distance, and their minimum by (dist, subject)
    bool listed = false;
    RC_TRY(read_table_spans(t, max_div, 1, "table", "at their smallest distance within", [&](unsigned long long count) {
        listed = true;
        return timed_pass(t.c, &J.link_ms, "table: the span's rows to best[]", [&] {
            hipLaunchKernelGGL(assign::best_kernel, list_grid(count), block, 0, db->stream, db->hits.as<smafa_hit>(), count, m, t.best);
        });
    }));
    RC_TRY(read_table_tail(t, n_samples, d_entries, cap, d_totals, [&](unsigned long long *ka, uint32_t *va, uint32_t sample_bits) {
        hipLaunchKernelGGL(assign::bin_kernel, row_grid(m), block, 0, db->stream, t.best, m, d_group_of, d_samples, n_samples, sample_bits, d_weights,
                           d_subject, d_dist, d_subject_counts, ka, va, d_totals);
    }));
    note_call_kernel(db, "assign::init_kernel");  // (behind the scan family's, which the spans have listed)
    if (listed) note_call_kernel(db, "assign::best_kernel");
    note_call_kernel(db, "assign::bin_kernel");
    note_call_kernel(db, "assign::heads_kernel");
    note_call_kernel(db, "assign::fold_kernel");
    log_line(2, "table of %u reads against %llu rows within %u, %u samples: %u scans (%u repeated) %.3f ms, best %.3f ms, keys, sort and sums "
             "%.3f ms", m, (unsigned long long)n, max_div, n_samples, J.blocks + J.rescans, J.rescans, J.scan_ms, J.link_ms, J.flatten_ms);
    return SMAFA_OK;
}


// what both entry points check first, in this order (nothing is written before they pass): self_args' four, the samples, the entries
static int assign_args(const char *who, const smafa_db *db, bool has_reads, const char *reads, const void *totals, uint32_t max_div,
                       uint32_t n_samples, const void *entries, uint64_t cap) {
    RC_TRY(self_args(who, db, has_reads, reads, totals, "totals", max_div, "a table needs a bound"));
    if (n_samples == 0) return set_error(SMAFA_ERR_INVALID, "%s: n_samples is 0 (1: every read is in sample 0)", who);
    if (!entries && cap) return missing(who, "entries with a capacity");
    return SMAFA_OK;
}

int smafa_db_assign_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, const void *d_labels, const void *d_samples, uint32_t n_samples,
                           const void *d_weights, void *d_subject, void *d_dist, void *d_subject_counts, void *d_entries, uint64_t cap,
                           void *d_totals) try {
    RC_TRY(assign_args("smafa_db_assign_launch", db, qs, "query set", d_totals, max_div, n_samples, d_entries, cap));
    if (qs->db != db) return set_error(SMAFA_ERR_INVALID, "smafa_db_assign_launch: the query set was packed for a different store");
    return assign_reads(db, qs, "smafa_db_assign_launch", max_div, (const uint32_t *)d_labels, (const uint32_t *)d_samples, n_samples,
                        (const uint32_t *)d_weights, (uint32_t *)d_subject, (uint32_t *)d_dist, (unsigned long long *)d_subject_counts,
                        (smafa_table_entry *)d_entries, cap, (unsigned long long *)d_totals);
} catch (...) {
    return smafa::exception_code("smafa_db_assign_launch");
}

int smafa_db_assign(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div, const uint32_t *labels,
                    const uint32_t *samples, uint32_t n_samples, const uint32_t *weights, uint32_t *subject, uint32_t *dist,
                    uint64_t *subject_counts, smafa_table_entry *entries, uint64_t cap, uint64_t totals[4]) try {
    const char *const who = "smafa_db_assign";
    RC_TRY(assign_args(who, db, query_codes || !n_queries, "query_codes", totals, max_div, n_samples, entries, cap));
    RC_TRY(read_codes_args(who, db, query_codes, n_queries, samples, n_samples));
    const uint64_t n = db->n, m = n_queries;
    Staged a[] = {staged_out(subject_counts, n * 8u), staged_in(labels, n * 4u),  staged_in(samples, m * 4u),
                  staged_in(weights, m * 4u),         staged_out(subject, m * 4u), staged_out(dist, m * 4u)};
    return read_table_host(who, db, query_codes, m, a, entries, cap, totals, 4,
                           [&](smafa_qset *qs, smafa_table_entry *d_entries, uint64_t room, unsigned long long *d_totals) {
        return assign_reads(db, qs, who, max_div, a[1].as<const uint32_t>(), a[2].as<const uint32_t>(), n_samples, a[3].as<const uint32_t>(),
                            a[4].as<uint32_t>(), a[5].as<uint32_t>(), a[0].as<unsigned long long>(), d_entries, room, d_totals);
    });
} catch (...) {
    return smafa::exception_code("smafa_db_assign");
}

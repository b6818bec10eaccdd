// classify_abi.hip.h — the LCA classification of a resident query set: its call (classify_reads) and the two smafa_db_classify
// entry points.  A read-table call (read_table.hip.h, under SMAFA_ASSIGN_SPAN and SMAFA_ASSIGN_ROWS_MAX as the abundance table)
// with one kernel more per span and another per-read pass: classify.hip.h.  With slack 0 a span is scanned in the tightening
// mode (k = 1), as the table scans it; with a slack it is scanned at the fixed bound, which lists every row within it and counts
// them exactly even above the room.  A span that grows or is halved has run no kernel of the call, so no member is counted twice.
// Included once by engine.hip, inside extern "C", behind assign_abi.hip.h.
#pragma once

// The call.  Every pointer is the device's; d_lineage: n x n_ranks (nullptr for an empty store); d_samples, d_weights, d_subject,
// d_dist, d_taxon, d_depth, d_ties: or nullptr; d_entries: cap entries (nullptr with cap = 0).
// Its words in J.parent: depth[] and ties[].
static int classify_reads(smafa_db *db, smafa_qset *qs, const char *who, uint32_t max_div, uint32_t slack, const uint32_t *d_lineage,
                          uint32_t n_ranks, const uint32_t *d_samples, uint32_t n_samples, const uint32_t *d_weights, uint32_t *d_subject,
                          uint32_t *d_dist, uint32_t *d_taxon, uint32_t *d_depth, uint32_t *d_ties, smafa_table_entry *d_entries, uint64_t cap,
                          unsigned long long *d_totals) {
    auto &J = db->join;
    const uint64_t n = db->n;
    const dim3 block(256);
    ReadTable t{{db}, qs, who};
    RC_TRY(read_table_begin(t, "the call takes fewer than 2^31 reads", d_totals, 6, 2, "classify: best[], depth[], ties[] and the totals initialised",
                            "classify::start_kernel", [&] {
        hipLaunchKernelGGL(classify::start_kernel, list_grid(std::max<uint64_t>(t.m, 6)), block, 0, db->stream, t.best, t.words, t.words + t.m,
                           (uint64_t)t.m, n_ranks, d_totals);
    }));
    const uint32_t m = t.m;
    if (m == 0) return SMAFA_OK;
    uint32_t *const depth = t.words, *const ties = depth + m;
    // ---- the spans: each read's rows within its smallest distance + slack, their minimum by (dist, subject), then their agreement
    unsigned long long listed = 0;
    bool agreeing = false;  // an agree pass between ev[0] and ev[1] whose time is not read yet: read behind a later wait
    const auto book_agree = [&] {
        float ms = 0.f;
        if (agreeing && hipEventElapsedTime(&ms, J.ev[0], J.ev[1]) == hipSuccess) J.filter_ms += ms;
        agreeing = false;
    };
    RC_TRY(read_table_spans(t, max_div, slack ? 0u : 1u, "classify", slack ? "within the bound" : "within their smallest distance within",
                            [&](unsigned long long count) {
        book_agree();  // (the span's wait has ended the agree pass before)
        RC_TRY(timed_pass(t.c, &J.link_ms, "classify: the span's rows to best[]", [&] {
            hipLaunchKernelGGL(assign::best_kernel, list_grid(count), block, 0, db->stream, db->hits.as<smafa_hit>(), count, m, t.best);
        }));
        // behind it on the same stream, timed apart (filter_ms) by the two events the table's passes use later
        HIP_TRY(hipEventRecord(J.ev[0], db->stream));
        hipLaunchKernelGGL(classify::agree_kernel, list_grid(count), block, 0, db->stream, db->hits.as<smafa_hit>(), count, m, t.best, slack,
                           d_lineage, (uint32_t)n, n_ranks, depth, ties);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(J.ev[1], db->stream));
        db->call_launches++;
        agreeing = true;
        listed += count;
        return (int)SMAFA_OK;
    }));
    RC_TRY(read_table_tail(t, n_samples, d_entries, cap, d_totals, [&](unsigned long long *ka, uint32_t *va, uint32_t sample_bits) {
        hipLaunchKernelGGL(classify::key_kernel, row_grid(m), block, 0, db->stream, t.best, depth, ties, m, d_lineage, n_ranks, d_samples, n_samples,
                           sample_bits, d_weights, d_subject, d_dist, d_taxon, d_depth, d_ties, ka, va, d_totals);
    }, [&] {
        RC_TRY(timed_sync(t.c));  // (the last span's passes are booked here: the events are used again behind it)
        book_agree();
        return (int)SMAFA_OK;
    }));
    note_call_kernel(db, "classify::start_kernel");  // (behind the scan family's, which the spans have listed)
    if (listed) note_call_kernel(db, "assign::best_kernel");
    if (listed) note_call_kernel(db, "classify::agree_kernel");
    note_call_kernel(db, "classify::key_kernel");
    note_call_kernel(db, "assign::heads_kernel");
    note_call_kernel(db, "assign::fold_kernel");
    log_line(2, "classification of %u reads against %llu rows within %u, slack %u, %u ranks, %u samples: %u scans (%u repeated) %.3f ms, best "
             "%.3f ms, agree %.3f ms over %llu rows, keys, sort and sums %.3f ms", m, (unsigned long long)n, max_div, slack, n_ranks, n_samples,
             J.blocks + J.rescans, J.rescans, J.scan_ms, J.link_ms, J.filter_ms, listed, J.flatten_ms);
    return SMAFA_OK;
}

// what both entry points check first, in this order (nothing is written before they pass): assign_args' six, the ranks, the lineage
static int classify_args(const char *who, const smafa_db *db, bool has_reads, const char *reads, const void *totals, uint32_t max_div,
                         uint32_t n_samples, const void *entries, uint64_t cap, uint32_t n_ranks, const void *lineage) {
    RC_TRY(assign_args(who, db, has_reads, reads, totals, max_div, n_samples, entries, cap));
    if (n_ranks < 1u || n_ranks > classify::kMaxRanks)
        return set_error(SMAFA_ERR_INVALID, "%s: n_ranks is %u (1 .. %u)", who, n_ranks, classify::kMaxRanks);
    if (!lineage && db->n) return missing(who, "lineage");
    return SMAFA_OK;
}

int smafa_db_classify_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, uint32_t slack, const void *d_lineage, uint32_t n_ranks,
                             const void *d_samples, uint32_t n_samples, const void *d_weights, void *d_subject, void *d_dist, void *d_taxon,
                             void *d_depth, void *d_ties, void *d_entries, uint64_t cap, void *d_totals) try {
    const char *const who = "smafa_db_classify_launch";
    RC_TRY(classify_args(who, db, qs, "query set", d_totals, max_div, n_samples, d_entries, cap, n_ranks, d_lineage));
    if (qs->db != db) return set_error(SMAFA_ERR_INVALID, "%s: the query set was packed for a different store", who);
    return classify_reads(db, qs, who, max_div, slack, (const uint32_t *)d_lineage, n_ranks, (const uint32_t *)d_samples, n_samples,
                          (const uint32_t *)d_weights, (uint32_t *)d_subject, (uint32_t *)d_dist, (uint32_t *)d_taxon, (uint32_t *)d_depth,
                          (uint32_t *)d_ties, (smafa_table_entry *)d_entries, cap, (unsigned long long *)d_totals);
} catch (...) {
    return smafa::exception_code("smafa_db_classify_launch");
}

int smafa_db_classify(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div, uint32_t slack, const uint32_t *lineage,
                      uint32_t n_ranks, const uint32_t *samples, uint32_t n_samples, const uint32_t *weights, uint32_t *subject, uint32_t *dist,
                      uint32_t *taxon, uint32_t *depth, uint32_t *ties, smafa_table_entry *entries, uint64_t cap, uint64_t totals[6]) try {
    const char *const who = "smafa_db_classify";
    RC_TRY(classify_args(who, db, query_codes || !n_queries, "query_codes", totals, max_div, n_samples, entries, cap, n_ranks, lineage));
    RC_TRY(read_codes_args(who, db, query_codes, n_queries, samples, n_samples));
    const uint64_t n = db->n, m = n_queries;
    for (uint64_t i = 0; i < n; i++) {
        bool ended = false;
        for (uint32_t r = 0; r < n_ranks; r++) {
            const uint32_t id = lineage[i * n_ranks + r];
            if (id == SMAFA_TAXON_ROOT)
                return set_error(SMAFA_ERR_INVALID, "%s: lineage[%llu][%u] is SMAFA_TAXON_ROOT, which no subject may carry", who,
                                 (unsigned long long)i, r);
            if (id != SMAFA_NONE && ended)
                return set_error(SMAFA_ERR_INVALID, "%s: lineage[%llu][%u] holds an id behind a SMAFA_NONE", who, (unsigned long long)i, r);
            ended = ended || id == SMAFA_NONE;
        }
    }
    Staged a[] = {staged_in(n ? lineage : nullptr, n * n_ranks * 4u), staged_in(samples, m * 4u), staged_in(weights, m * 4u),
                  staged_out(subject, m * 4u), staged_out(dist, m * 4u), staged_out(taxon, m * 4u), staged_out(depth, m * 4u),
                  staged_out(ties, m * 4u)};
    return read_table_host(who, db, query_codes, m, a, entries, cap, totals, 6,
                           [&](smafa_qset *qs, smafa_table_entry *d_entries, uint64_t room, unsigned long long *d_totals) {
        return classify_reads(db, qs, who, max_div, slack, a[0].as<const uint32_t>(), n_ranks, a[1].as<const uint32_t>(), n_samples,
                              a[2].as<const uint32_t>(), a[3].as<uint32_t>(), a[4].as<uint32_t>(), a[5].as<uint32_t>(), a[6].as<uint32_t>(),
                              a[7].as<uint32_t>(), d_entries, room, d_totals);
    });
} catch (...) {
    return smafa::exception_code("smafa_db_classify");
}

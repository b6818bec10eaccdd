// assign_abi.hip.h — the abundance table of a resident store: its call (assign_reads) and the two smafa_db_assign entry points.
// Not a consumer of the join: the reads are a query set of the caller's, scanned span by span through scan_range in the tightening
// mode (k = 1), and the call's own kernels (assign.hip.h) consume each span's list.  It shares the join's call frame (join_begin,
// the timed passes, so that smafa_last_call_* and smafa_last_scan_ms report it) and the self-join's checks and host form
// (self_args, HostForm).  Included once by engine.hip, inside extern "C", behind self_join_abi.hip.h.
#pragma once

#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// The call.  Every pointer is the device's; d_group_of, d_samples, d_weights, d_subject, d_dist, d_subject_counts: or nullptr;
// d_entries: cap entries (nullptr with cap = 0).  The span rule is engine.h's (assign_first_room, assign_span_rule).
// J.parent holds best[] (8 B per read), mark[] and its sums (4 B x 2 per read); the sort's double buffers are the handle's keys_a /
// keys_b (8 B per read), idx_a / idx_b (4 B per read) and the shared sort_tmp.  pos_of[], the kept list and the index are not touched.
static int assign_reads(smafa_db *db, smafa_qset *qs, const char *who, uint32_t max_div, const uint32_t *d_group_of, const uint32_t *d_samples,
                        uint32_t n_samples, const uint32_t *d_weights, uint32_t *d_subject, uint32_t *d_dist, unsigned long long *d_subject_counts,
                        smafa_table_entry *d_entries, uint64_t cap, unsigned long long *d_totals) {
    auto &J = db->join;
    if (qs->nq >= (1ull << 31))  // (the device radix sort counts its items in an int)
        return set_error(SMAFA_ERR_INVALID, "%s: the table takes fewer than 2^31 reads per call (this set: %llu)", who, (unsigned long long)qs->nq);
    const uint32_t m = (uint32_t)qs->nq;
    const uint64_t n = db->n;
    JoinCall c{db};
    RC_TRY(join_begin(c, d_totals, 4, 0));
    RC_TRY(J.parent.ensure(((size_t)m + 1u) * 16u));
    unsigned long long *const best = J.parent.as<unsigned long long>();
    uint32_t *const mark = reinterpret_cast<uint32_t *>(best + m), *const sum = mark + m + 1u;
    const dim3 block(256);
    RC_TRY(timed_pass(c, &J.count_ms, "table: best[], the subject counts and the totals initialised", [&] {
        hipLaunchKernelGGL(assign::init_kernel, list_grid(std::max<uint64_t>(std::max<uint64_t>(m, d_subject_counts ? n : 0), 4)), block, 0,
                           db->stream, best, (uint64_t)m, d_subject_counts, n, d_totals);
    }));
    if (m == 0) {
        RC_TRY(timed_sync(c));
        note_call_kernel(db, "assign::init_kernel");
        db->call_ms += (float)J.count_ms;
        db->call_timed = true;
        return SMAFA_OK;
    }
    // ---- the spans: each read's rows at its minimum distance, and their minimum by (dist, subject)
    uint64_t span = db->assign_span, room = std::min<uint64_t>(assign_first_room(span, db->assign_rows_max), db->hits_cap());
    bool listed = false;
    for (uint64_t q0 = 0; q0 < m;) {
        const uint64_t q1 = std::min<uint64_t>(m, q0 + span);
        RC_TRY(scan_range(db, qs, (uint32_t)q0, (uint32_t)q1, max_div, 1, db->hits.as<smafa_hit>(), room, db->count.as<unsigned long long>()));
        unsigned long long count = 0;
        HIP_TRY(hipMemcpyAsync(&count, db->count.p, sizeof count, hipMemcpyDeviceToHost, db->stream));
        RC_TRY(timed_sync(c));  // (with it ends the pass over the span before)
        const float before = db->call_ms;
        note_call_scan(db);
        J.scan_ms += db->call_ms - before;
        log_line(3, "table: reads %llu..%llu: %llu rows (room %llu)", (unsigned long long)q0, (unsigned long long)q1, count, (unsigned long long)room);
        const PieceRule rule = assign_span_rule(count, room, db->assign_rows_max, q1 - q0);
        if (rule.verdict != kPieceTake) J.rescans++;
        if (rule.verdict == kPieceFail)
            return set_error(SMAFA_ERR_NOMEM, "%s: %llu reads have more rows at their smallest distance within %u than the row list may hold "
                             "(%llu rows did not fit %llu)", who, (unsigned long long)(q1 - q0), max_div, count, (unsigned long long)room);
        if (rule.verdict == kPieceGrow) {
            room = std::min<uint64_t>(db->assign_rows_max, room * 2);
            RC_TRY(db->hits.ensure(room * sizeof(smafa_hit)));
            continue;  // the same reads once more
        }
        if (rule.verdict == kPieceHalve) {
            span = rule.piece;
            continue;  // their first half
        }
        if (count) {
            RC_TRY(timed_pass(c, &J.link_ms, "table: the span's rows to best[]", [&] {
                hipLaunchKernelGGL(assign::best_kernel, list_grid(count), block, 0, db->stream, db->hits.as<smafa_hit>(), count, m, best);
            }));
            listed = true;
        }
        J.blocks++;
        q0 = q1;
    }
    // ---- the table: keys, the sort, the heads and their numbers, the sums — enqueued at once and waited for once
    uint32_t sample_bits = 1;
    while (sample_bits < 32u && (1ull << sample_bits) <= n_samples) sample_bits++;  // (holds n_samples itself: the dead key's sample)
    const int key_bits = (int)(32u + sample_bits);
    RC_TRY(db->keys_a.ensure((size_t)m * sizeof(unsigned long long)));
    RC_TRY(db->keys_b.ensure((size_t)m * sizeof(unsigned long long)));
    RC_TRY(db->idx_a.ensure((size_t)m * sizeof(uint32_t)));
    RC_TRY(db->idx_b.ensure((size_t)m * sizeof(uint32_t)));
    unsigned long long *const ka = db->keys_a.as<unsigned long long>(), *const kb = db->keys_b.as<unsigned long long>();
    uint32_t *const va = db->idx_a.as<uint32_t>(), *const vb = db->idx_b.as<uint32_t>();
    size_t sort_bytes = 0, sum_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, ka, kb, va, vb, (int)m, 0, key_bits, db->stream));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, sum_bytes, mark, sum, m + 1u, db->stream));
    RC_TRY(db->sort_tmp.ensure(std::max(sort_bytes, sum_bytes)));
    const uint64_t stored = std::min<uint64_t>(cap, m);  // no more entries than reads
    const dim3 reads = row_grid(m);
    HIP_TRY(hipEventRecord(J.ev[0], db->stream));
    if (stored) HIP_TRY(hipMemsetAsync(d_entries, 0, stored * sizeof(smafa_table_entry), db->stream));
    hipLaunchKernelGGL(assign::bin_kernel, reads, block, 0, db->stream, best, m, d_group_of, d_samples, n_samples, sample_bits, d_weights, d_subject,
                       d_dist, d_subject_counts, ka, va, d_totals);
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, sort_bytes, ka, kb, va, vb, (int)m, 0, key_bits, db->stream));
    hipLaunchKernelGGL(assign::heads_kernel, row_grid(m + 1u), block, 0, db->stream, kb, m, sample_bits, mark);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(db->sort_tmp.p, sum_bytes, mark, sum, m + 1u, db->stream));
    hipLaunchKernelGGL(assign::fold_kernel, reads, block, 0, db->stream, kb, vb, mark, sum, m, sample_bits, d_entries, (unsigned long long)cap,
                       d_totals);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[1], db->stream));
    RC_TRY(timed_sync(c));  // (the last span's pass is booked here)
    float table_ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&table_ms, J.ev[0], J.ev[1]));
    J.flatten_ms = table_ms;
    db->call_ms += (float)(J.count_ms + J.link_ms + J.flatten_ms);
    db->call_launches += 5u;  // (the sort's and the sum's launches count as one each)
    db->call_timed = true;    // (scan_range cleared it)
    note_call_kernel(db, "assign::init_kernel");  // (behind the scan family's, which the spans have listed)
    if (listed) note_call_kernel(db, "assign::best_kernel");
    note_call_kernel(db, "assign::bin_kernel");
    note_call_kernel(db, "assign::heads_kernel");
    note_call_kernel(db, "assign::fold_kernel");
    log_line(2, "table of %u reads against %llu rows within %u, %u samples: %u scans (%u repeated) %.3f ms, best %.3f ms, keys, sort and sums "
             "%.3f ms", m, (unsigned long long)n, max_div, n_samples, J.blocks + J.rescans, J.rescans, J.scan_ms, J.link_ms, J.flatten_ms);
    trim({&db->hits, &db->scratch, &J.parent});
    trim_together(db->keys_a, {&db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp});
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
    if (n_queries > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "%s: too many reads in one call", who);
    RC_TRY(validate_codes(db, query_codes, n_queries));
    if (samples)
        for (uint64_t q = 0; q < n_queries; q++)
            if (samples[q] >= n_samples)
                return set_error(SMAFA_ERR_INVALID, "%s: samples[%llu] is %u, n_samples is %u", who, (unsigned long long)q, samples[q], n_samples);
    std::fill(totals, totals + 4, (uint64_t)0);
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n, m = n_queries, room = std::min<uint64_t>(cap, m);  // no more entries than reads
    // the subject counts and the entries on their way out, the labels, samples and weights on their way in, subject and dist on
    // their way out: 8 B and 4 B per subject, 16 B per entry, 4 B x 4 per read
    RC_TRY(h.stage(std::max<uint64_t>(n * 12u + room * sizeof(smafa_table_entry) + m * 16u, 1), 4));
    unsigned long long *const d_counts = J.out.as<unsigned long long>();
    smafa_table_entry *const d_entries = reinterpret_cast<smafa_table_entry *>(d_counts + n);
    uint32_t *const d_labels = reinterpret_cast<uint32_t *>(d_entries + room), *const d_samples = d_labels + n, *const d_weights = d_samples + m;
    uint32_t *const d_subject = d_weights + m, *const d_dist = d_subject + m;
    struct Reads {  // the call's own query set
        smafa_qset qs;
        ~Reads() {
            for (DevBuf *b : {&qs.qrec, &qs.thr, &qs.cnt}) b->release();
        }
    } reads;
    RC_TRY(qset_fill(&reads.qs, db, query_codes, m));
    if (labels && n) HIP_TRY(hipMemcpyAsync(d_labels, labels, n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    if (samples && m) HIP_TRY(hipMemcpyAsync(d_samples, samples, m * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    if (weights && m) HIP_TRY(hipMemcpyAsync(d_weights, weights, m * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    RC_TRY(assign_reads(db, &reads.qs, who, max_div, labels ? d_labels : nullptr, samples ? d_samples : nullptr, n_samples,
                        weights ? d_weights : nullptr, subject ? d_subject : nullptr, dist ? d_dist : nullptr, subject_counts ? d_counts : nullptr,
                        room ? d_entries : nullptr, room, h.cnt()));
    uint64_t got[4] = {0, 0, 0, 0};
    RC_TRY(h.fetch(got, h.cnt(), sizeof got));
    RC_TRY(h.wait());  // (a wait of its own: the number of entries decides the rest)
    std::copy(got, got + 4, totals);
    if (got[0] > cap)
        return set_error(SMAFA_ERR_CAPACITY, "%s: entry buffer too small: %llu entries needed, capacity %llu", who, (unsigned long long)got[0],
                         (unsigned long long)cap);
    RC_TRY(h.fetch(entries, d_entries, got[0] * sizeof(smafa_table_entry)));
    RC_TRY(h.fetch(subject, d_subject, m * sizeof(uint32_t)));
    RC_TRY(h.fetch(dist, d_dist, m * sizeof(uint32_t)));
    RC_TRY(h.fetch(subject_counts, d_counts, n * sizeof(uint64_t)));
    RC_TRY(h.wait());
    trim({&J.out});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_assign");
}
#undef RC_TRY

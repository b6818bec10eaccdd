// classify_abi.hip.h — the LCA classification of a resident query set: its call (classify_reads) and the two smafa_db_classify
// entry points.  The abundance table's frame (assign_abi.hip.h: join_begin, the timed passes, the span loop under
// assign_first_room / assign_span_rule, SMAFA_ASSIGN_SPAN and SMAFA_ASSIGN_ROWS_MAX) with one kernel more per span and another
// per-read pass: classify.hip.h.  With slack 0 a span is scanned in the tightening mode (k = 1), as the table scans it; with a
// slack it is scanned at the fixed bound, which lists every row within it and counts them exactly even above the room.  A span
// that grows or is halved has run no kernel of the call, so no member is counted twice.
// Included once by engine.hip, inside extern "C", behind assign_abi.hip.h.
#pragma once

#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// The call.  Every pointer is the device's; d_lineage: n x n_ranks (nullptr for an empty store); d_samples, d_weights, d_subject,
// d_dist, d_taxon, d_depth, d_ties: or nullptr; d_entries: cap entries (nullptr with cap = 0).
// J.parent holds best[] (8 B per read), depth[], ties[], mark[] and its sums (4 B x 4 per read); the sort's double buffers are the
// handle's keys_a / keys_b (8 B per read), idx_a / idx_b (4 B per read) and the shared sort_tmp.
static int classify_reads(smafa_db *db, smafa_qset *qs, const char *who, uint32_t max_div, uint32_t slack, const uint32_t *d_lineage,
                          uint32_t n_ranks, const uint32_t *d_samples, uint32_t n_samples, const uint32_t *d_weights, uint32_t *d_subject,
                          uint32_t *d_dist, uint32_t *d_taxon, uint32_t *d_depth, uint32_t *d_ties, smafa_table_entry *d_entries, uint64_t cap,
                          unsigned long long *d_totals) {
    auto &J = db->join;
    if (qs->nq >= (1ull << 31))  // (the device radix sort counts its items in an int)
        return set_error(SMAFA_ERR_INVALID, "%s: the call takes fewer than 2^31 reads (this set: %llu)", who, (unsigned long long)qs->nq);
    const uint32_t m = (uint32_t)qs->nq;
    const uint64_t n = db->n;
    JoinCall c{db};
    RC_TRY(join_begin(c, d_totals, 6, 0));
    RC_TRY(J.parent.ensure(((size_t)m + 1u) * 24u));
    unsigned long long *const best = J.parent.as<unsigned long long>();
    uint32_t *const depth = reinterpret_cast<uint32_t *>(best + m), *const ties = depth + m, *const mark = ties + m, *const sum = mark + m + 1u;
    const dim3 block(256);
    RC_TRY(timed_pass(c, &J.count_ms, "classify: best[], depth[], ties[] and the totals initialised", [&] {
        hipLaunchKernelGGL(classify::start_kernel, list_grid(std::max<uint64_t>(m, 6)), block, 0, db->stream, best, depth, ties, (uint64_t)m, n_ranks,
                           d_totals);
    }));
    if (m == 0) {
        RC_TRY(timed_sync(c));
        note_call_kernel(db, "classify::start_kernel");
        db->call_ms += (float)J.count_ms;
        db->call_timed = true;
        return SMAFA_OK;
    }
    // ---- the spans: each read's rows within its smallest distance + slack, their minimum by (dist, subject), then their agreement
    const uint32_t k_tight = slack ? 0u : 1u;
    uint64_t span = db->assign_span, room = std::min<uint64_t>(assign_first_room(span, db->assign_rows_max), db->hits_cap());
    unsigned long long listed = 0;
    bool agreeing = false;  // an agree pass between ev[0] and ev[1] whose time is not read yet: read behind the next wait
    const auto book_agree = [&] {
        float ms = 0.f;
        if (agreeing && hipEventElapsedTime(&ms, J.ev[0], J.ev[1]) == hipSuccess) J.filter_ms += ms;
        agreeing = false;
    };
    for (uint64_t q0 = 0; q0 < m;) {
        const uint64_t q1 = std::min<uint64_t>(m, q0 + span);
        RC_TRY(scan_range(db, qs, (uint32_t)q0, (uint32_t)q1, max_div, k_tight, db->hits.as<smafa_hit>(), room, db->count.as<unsigned long long>()));
        unsigned long long count = 0;
        HIP_TRY(hipMemcpyAsync(&count, db->count.p, sizeof count, hipMemcpyDeviceToHost, db->stream));
        RC_TRY(timed_sync(c));  // (with it end the passes over the span before)
        book_agree();
        const float before = db->call_ms;
        note_call_scan(db);
        J.scan_ms += db->call_ms - before;
        log_line(3, "classify: reads %llu..%llu: %llu rows (room %llu)", (unsigned long long)q0, (unsigned long long)q1, count, (unsigned long long)room);
        const PieceRule rule = assign_span_rule(count, room, db->assign_rows_max, q1 - q0);
        if (rule.verdict != kPieceTake) J.rescans++;
        if (rule.verdict == kPieceFail)
            return set_error(SMAFA_ERR_NOMEM, "%s: %llu reads have more rows within %s %u than the row list may hold (%llu rows did not fit %llu)", who,
                             (unsigned long long)(q1 - q0), slack ? "the bound" : "their smallest distance within", max_div, count,
                             (unsigned long long)room);
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
            RC_TRY(timed_pass(c, &J.link_ms, "classify: the span's rows to best[]", [&] {
                hipLaunchKernelGGL(assign::best_kernel, list_grid(count), block, 0, db->stream, db->hits.as<smafa_hit>(), count, m, best);
            }));
            // behind it on the same stream, timed apart (filter_ms) by the two events the table's passes use later
            HIP_TRY(hipEventRecord(J.ev[0], db->stream));
            hipLaunchKernelGGL(classify::agree_kernel, list_grid(count), block, 0, db->stream, db->hits.as<smafa_hit>(), count, m, best, slack,
                               d_lineage, (uint32_t)n, n_ranks, depth, ties);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(J.ev[1], db->stream));
            db->call_launches++;
            agreeing = true;
            listed += count;
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
    RC_TRY(timed_sync(c));  // (the last span's passes are booked here: the events are used again below)
    book_agree();
    HIP_TRY(hipEventRecord(J.ev[0], db->stream));
    if (stored) HIP_TRY(hipMemsetAsync(d_entries, 0, stored * sizeof(smafa_table_entry), db->stream));
    hipLaunchKernelGGL(classify::key_kernel, reads, block, 0, db->stream, best, depth, ties, m, d_lineage, n_ranks, d_samples, n_samples, sample_bits,
                       d_weights, d_subject, d_dist, d_taxon, d_depth, d_ties, ka, va, d_totals);
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, sort_bytes, ka, kb, va, vb, (int)m, 0, key_bits, db->stream));
    hipLaunchKernelGGL(assign::heads_kernel, row_grid(m + 1u), block, 0, db->stream, kb, m, sample_bits, mark);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(db->sort_tmp.p, sum_bytes, mark, sum, m + 1u, db->stream));
    hipLaunchKernelGGL(assign::fold_kernel, reads, block, 0, db->stream, kb, vb, mark, sum, m, sample_bits, d_entries, (unsigned long long)cap,
                       d_totals);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[1], db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    float table_ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&table_ms, J.ev[0], J.ev[1]));
    J.flatten_ms = table_ms;
    db->call_ms += (float)(J.count_ms + J.link_ms + J.filter_ms + J.flatten_ms);
    db->call_launches += 5u;  // (the sort's and the sum's launches count as one each)
    db->call_timed = true;    // (scan_range cleared it)
    note_call_kernel(db, "classify::start_kernel");  // (behind the scan family's, which the spans have listed)
    if (listed) note_call_kernel(db, "assign::best_kernel");
    if (listed) note_call_kernel(db, "classify::agree_kernel");
    note_call_kernel(db, "classify::key_kernel");
    note_call_kernel(db, "assign::heads_kernel");
    note_call_kernel(db, "assign::fold_kernel");
    log_line(2, "classification of %u reads against %llu rows within %u, slack %u, %u ranks, %u samples: %u scans (%u repeated) %.3f ms, best "
             "%.3f ms, agree %.3f ms over %llu rows, keys, sort and sums %.3f ms", m, (unsigned long long)n, max_div, slack, n_ranks, n_samples,
             J.blocks + J.rescans, J.rescans, J.scan_ms, J.link_ms, J.filter_ms, listed, J.flatten_ms);
    trim({&db->hits, &db->scratch, &J.parent});
    trim_together(db->keys_a, {&db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp});
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
    if (n_queries > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "%s: too many reads in one call", who);
    RC_TRY(validate_codes(db, query_codes, n_queries));
    if (samples)
        for (uint64_t q = 0; q < n_queries; q++)
            if (samples[q] >= n_samples)
                return set_error(SMAFA_ERR_INVALID, "%s: samples[%llu] is %u, n_samples is %u", who, (unsigned long long)q, samples[q], n_samples);
    const uint64_t n = db->n, m = n_queries, room = std::min<uint64_t>(cap, m);  // no more entries than reads
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
    std::fill(totals, totals + 6, (uint64_t)0);
    const HostForm h{db};
    auto &J = db->join;
    // the entries on their way out, the lineage, samples and weights on their way in, the five per-read arrays on their way out:
    // 16 B per entry, 4 B x n_ranks per subject, 4 B x 7 per read
    RC_TRY(h.stage(std::max<uint64_t>(room * sizeof(smafa_table_entry) + n * n_ranks * 4u + m * 28u, 1), 6));
    smafa_table_entry *const d_entries = J.out.as<smafa_table_entry>();
    uint32_t *const d_lineage = reinterpret_cast<uint32_t *>(d_entries + room), *const d_samples = d_lineage + n * n_ranks, *const d_weights = d_samples + m;
    uint32_t *const d_subject = d_weights + m, *const d_dist = d_subject + m, *const d_taxon = d_dist + m, *const d_depth = d_taxon + m;
    uint32_t *const d_ties = d_depth + m;
    struct Reads {  // the call's own query set
        smafa_qset qs;
        ~Reads() {
            for (DevBuf *b : {&qs.qrec, &qs.thr, &qs.cnt}) b->release();
        }
    } reads;
    RC_TRY(qset_fill(&reads.qs, db, query_codes, m));
    if (n) HIP_TRY(hipMemcpyAsync(d_lineage, lineage, n * n_ranks * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    if (samples && m) HIP_TRY(hipMemcpyAsync(d_samples, samples, m * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    if (weights && m) HIP_TRY(hipMemcpyAsync(d_weights, weights, m * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    RC_TRY(classify_reads(db, &reads.qs, who, max_div, slack, n ? d_lineage : nullptr, n_ranks, samples ? d_samples : nullptr, n_samples,
                          weights ? d_weights : nullptr, subject ? d_subject : nullptr, dist ? d_dist : nullptr, taxon ? d_taxon : nullptr,
                          depth ? d_depth : nullptr, ties ? d_ties : nullptr, room ? d_entries : nullptr, room, h.cnt()));
    uint64_t got[6] = {0, 0, 0, 0, 0, 0};
    RC_TRY(h.fetch(got, h.cnt(), sizeof got));
    RC_TRY(h.wait());  // (a wait of its own: the number of entries decides the rest)
    std::copy(got, got + 6, totals);
    if (got[0] > cap)
        return set_error(SMAFA_ERR_CAPACITY, "%s: entry buffer too small: %llu entries needed, capacity %llu", who, (unsigned long long)got[0],
                         (unsigned long long)cap);
    RC_TRY(h.fetch(entries, d_entries, got[0] * sizeof(smafa_table_entry)));
    RC_TRY(h.fetch(subject, d_subject, m * sizeof(uint32_t)));
    RC_TRY(h.fetch(dist, d_dist, m * sizeof(uint32_t)));
    RC_TRY(h.fetch(taxon, d_taxon, m * sizeof(uint32_t)));
    RC_TRY(h.fetch(depth, d_depth, m * sizeof(uint32_t)));
    RC_TRY(h.fetch(ties, d_ties, m * sizeof(uint32_t)));
    RC_TRY(h.wait());
    trim({&J.out});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_classify");
}
#undef RC_TRY

// read_table.hip.h — the frame of a READ-TABLE call: a call that scans a query set of the caller's span by span, keeps one best
// row per read and tabulates the reads per (label, sample).  The abundance table (assign_abi.hip.h) and the LCA classification
// (classify_abi.hip.h) are the two there are.  Not a consumer of the join, but inside its call frame (join_begin, the timed passes,
// so that smafa_last_call_* and smafa_last_scan_ms report the call).  A call supplies its init kernel, what it does with a span's
// list, its key kernel, its kernel notes and its level-2 line; the frame holds
//   read_table_begin   the 2^31 check, join_begin, J.parent carved, the init pass, the exit of a call without reads
//   read_table_spans   the span loop under engine.h's span rule (assign_first_room, assign_span_rule): one host wait per scan
//   read_table_tail    keys, the sort, the heads and their numbers, the sums — enqueued at once and waited for once
// and, for the host forms, read_codes_args (what they check of the reads) and read_table_host (the staging of the caller's arrays
// in J.out, the call's own query set, the capacity protocol).
// Included once by engine.hip, inside extern "C", behind self_join_abi.hip.h (self_args, HostForm).
#pragma once

extern "C++" {  // (templates)

// One call's state.  J.parent holds best[] (8 B per read), the call's own `words` arrays (4 B per read each), mark[] and its sums
// (4 B x 2 per read, m + 1 of each); the sort's double buffers are the handle's keys_a / keys_b (8 B per read), idx_a / idx_b (4 B
// per read) and the shared sort_tmp.  pos_of[], the kept list and the index are not touched.
struct ReadTable {
    JoinCall c;
    smafa_qset *qs;
    const char *who;
    uint32_t m = 0;  // the reads
    unsigned long long *best = nullptr;
    uint32_t *words = nullptr, *mark = nullptr, *sum = nullptr;
};

// takes: what the call says of its limit; what: the init pass's trace text; init: its launch, which may use t's pointers.  A call
// without reads (t.m == 0) has ended when this returns: the caller returns.
template <class Init>
static int read_table_begin(ReadTable &t, const char *takes, unsigned long long *d_totals, size_t n_totals, uint32_t words, const char *what,
                            const char *init_name, Init init) {
    smafa_db *db = t.c.db;
    auto &J = db->join;
    if (t.qs->nq >= (1ull << 31))  // (the device radix sort counts its items in an int)
        return set_error(SMAFA_ERR_INVALID, "%s: %s (this set: %llu)", t.who, takes, (unsigned long long)t.qs->nq);
    t.m = (uint32_t)t.qs->nq;
    RC_TRY(join_begin(t.c, d_totals, n_totals, 0));
    RC_TRY(J.parent.ensure(((size_t)t.m + 1u) * (16u + 4u * words)));
    t.best = J.parent.as<unsigned long long>();
    t.words = reinterpret_cast<uint32_t *>(t.best + t.m), t.mark = t.words + (size_t)words * t.m, t.sum = t.mark + t.m + 1u;
    RC_TRY(timed_pass(t.c, &J.count_ms, what, init));
    if (t.m) return SMAFA_OK;
    RC_TRY(timed_sync(t.c));
    note_call_kernel(db, init_name);
    db->call_ms += (float)J.count_ms;
    db->call_timed = true;
    return SMAFA_OK;
}

// The spans: each scanned with max_num_hits = k (1: the tightening mode, a count above the room only says "did not fit"; 0: the
// fixed bound, counted exactly) into `room` rows of the handle's row list.  take(count) enqueues the call's kernels over a list
// that fits and holds rows; a span that grows or is halved has run none of them.  tag: the call in the level-3 line; rows_where:
// which rows the scan lists, for the text of a span that cannot fit.
template <class Take>
static int read_table_spans(ReadTable &t, uint32_t max_div, uint32_t k, const char *tag, const char *rows_where, Take take) {
    smafa_db *db = t.c.db;
    auto &J = db->join;
    uint64_t span = db->assign_span, room = std::min<uint64_t>(assign_first_room(span, db->assign_rows_max), db->hits_cap());
    for (uint64_t q0 = 0; q0 < t.m;) {
        const uint64_t q1 = std::min<uint64_t>(t.m, q0 + span);
        RC_TRY(scan_range(db, t.qs, (uint32_t)q0, (uint32_t)q1, max_div, k, db->hits.as<smafa_hit>(), room, db->count.as<unsigned long long>()));
        unsigned long long count = 0;
        HIP_TRY(hipMemcpyAsync(&count, db->count.p, sizeof count, hipMemcpyDeviceToHost, db->stream));
        RC_TRY(timed_sync(t.c));  // (with it end the passes over the span before)
        const float before = db->call_ms;
        note_call_scan(db);
        J.scan_ms += db->call_ms - before;
        log_line(3, "%s: reads %llu..%llu: %llu rows (room %llu)", tag, (unsigned long long)q0, (unsigned long long)q1, count, (unsigned long long)room);
        const PieceRule rule = assign_span_rule(count, room, db->assign_rows_max, q1 - q0);
        if (rule.verdict != kPieceTake) J.rescans++;
        if (rule.verdict == kPieceFail)
            return set_error(SMAFA_ERR_NOMEM, "%s: %llu reads have more rows %s %u than the row list may hold (%llu rows did not fit %llu)", t.who,
                             (unsigned long long)(q1 - q0), rows_where, max_div, count, (unsigned long long)room);
        if (rule.verdict == kPieceGrow) {
            room = std::min<uint64_t>(db->assign_rows_max, room * 2);
            RC_TRY(db->hits.ensure(room * sizeof(smafa_hit)));
            continue;  // the same reads once more
        }
        if (rule.verdict == kPieceHalve) {
            span = rule.piece;
            continue;  // their first half
        }
        if (count) RC_TRY(take(count));
        J.blocks++;
        q0 = q1;
    }
    return SMAFA_OK;
}

// The table.  keys(ka, va, sample_bits) launches the call's key kernel: one (key, weight) pair per read from best[] and the call's
// words.  before_events: what a call that has used ev[0] / ev[1] over its spans does in front of their use here (the
// classification: a wait of its own); the one wait at the end books the last span's pass where nothing has.
template <class Keys>
static int read_table_tail(ReadTable &t, uint32_t n_samples, smafa_table_entry *d_entries, uint64_t cap, unsigned long long *d_totals, Keys keys,
                           const std::function<int()> &before_events = nullptr) {
    smafa_db *db = t.c.db;
    auto &J = db->join;
    const uint32_t m = t.m;
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
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, sum_bytes, t.mark, t.sum, m + 1u, db->stream));
    RC_TRY(db->sort_tmp.ensure(std::max(sort_bytes, sum_bytes)));
    const uint64_t stored = std::min<uint64_t>(cap, m);  // no more entries than reads
    const dim3 block(256);
    if (before_events) RC_TRY(before_events());
    HIP_TRY(hipEventRecord(J.ev[0], db->stream));
    if (stored) HIP_TRY(hipMemsetAsync(d_entries, 0, stored * sizeof(smafa_table_entry), db->stream));
    keys(ka, va, sample_bits);
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, sort_bytes, ka, kb, va, vb, (int)m, 0, key_bits, db->stream));
    hipLaunchKernelGGL(assign::heads_kernel, row_grid(m + 1u), block, 0, db->stream, kb, m, sample_bits, t.mark);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(db->sort_tmp.p, sum_bytes, t.mark, t.sum, m + 1u, db->stream));
    hipLaunchKernelGGL(assign::fold_kernel, row_grid(m), block, 0, db->stream, kb, vb, t.mark, t.sum, m, sample_bits, d_entries,
                       (unsigned long long)cap, d_totals);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[1], db->stream));
    RC_TRY(timed_sync(t.c));
    float table_ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&table_ms, J.ev[0], J.ev[1]));
    J.flatten_ms = table_ms;
    db->call_ms += (float)(J.count_ms + J.link_ms + J.filter_ms + J.flatten_ms);  // (filter_ms: 0 since join_begin where no call books it)
    db->call_launches += 5u;  // (the sort's and the sum's launches count as one each)
    db->call_timed = true;    // (scan_range cleared it)
    trim({&db->hits, &db->scratch, &J.parent});
    trim_together(db->keys_a, {&db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp});
    return SMAFA_OK;
}

// ---- the host forms
// what both check of their reads behind the call's own argument checks, in this order: their number, their codes, their samples
static int read_codes_args(const char *who, smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, const uint32_t *samples,
                           uint32_t n_samples) {
    if (n_queries > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "%s: too many reads in one call", who);
    RC_TRY(validate_codes(db, query_codes, n_queries));
    if (samples)
        for (uint64_t q = 0; q < n_queries; q++)
            if (samples[q] >= n_samples)
                return set_error(SMAFA_ERR_INVALID, "%s: samples[%llu] is %u, n_samples is %u", who, (unsigned long long)q, samples[q], n_samples);
    return SMAFA_OK;
}

// One of the caller's arrays as the host form stages it in J.out: uploaded in front of the call, or fetched behind it.
struct Staged {
    const void *in;
    void *out;
    uint64_t bytes;
    void *dev = nullptr;  // its place in J.out; nullptr where the caller gave no array
    template <class T>
    T *as() const {
        return static_cast<T *>(dev);
    }
};
static Staged staged_in(const void *from, uint64_t bytes) { return {from, nullptr, bytes}; }
static Staged staged_out(void *to, uint64_t bytes) { return {nullptr, to, bytes}; }

// The host form of a read-table call, behind every check: totals[] zeroed, J.out staged — the entries (min(cap, m): no more
// entries than reads), then `arrays` in their order, 8-byte elements first —, the reads packed into a query set of the call's own,
// the arrays uploaded, call(query set, d_entries, room, d_totals); then the totals fetched by a wait of their own (the number of
// entries decides the rest), SMAFA_ERR_CAPACITY with the totals alone, or the entries and the arrays fetched.
template <size_t N, class Call>
static int read_table_host(const char *who, smafa_db *db, const uint8_t *query_codes, uint64_t m, Staged (&arrays)[N], smafa_table_entry *entries,
                           uint64_t cap, uint64_t *totals, size_t n_totals, Call call) {
    std::fill(totals, totals + n_totals, (uint64_t)0);
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t room = std::min<uint64_t>(cap, m);
    uint64_t bytes = room * sizeof(smafa_table_entry);
    for (const Staged &a : arrays) bytes += a.bytes;
    RC_TRY(h.stage(std::max<uint64_t>(bytes, 1), n_totals));
    smafa_table_entry *const d_entries = J.out.as<smafa_table_entry>();
    char *at = reinterpret_cast<char *>(d_entries + room);
    for (Staged &a : arrays) {
        a.dev = a.in || a.out ? at : nullptr;
        at += a.bytes;
    }
    struct Reads {  // the call's own query set
        smafa_qset qs;
        ~Reads() {
            for (DevBuf *b : {&qs.qrec, &qs.thr, &qs.cnt}) b->release();
        }
    } reads;
    RC_TRY(qset_fill(&reads.qs, db, query_codes, m));
    for (const Staged &a : arrays)
        if (a.in && a.bytes) HIP_TRY(hipMemcpyAsync(a.dev, a.in, a.bytes, hipMemcpyHostToDevice, db->stream));
    RC_TRY(call(&reads.qs, room ? d_entries : nullptr, room, h.cnt()));
    std::vector<uint64_t> got(n_totals, 0);
    RC_TRY(h.fetch(got.data(), h.cnt(), n_totals * sizeof(uint64_t)));
    RC_TRY(h.wait());  // (a wait of its own: the number of entries decides the rest)
    std::copy(got.begin(), got.end(), totals);
    if (got[0] > cap)
        return set_error(SMAFA_ERR_CAPACITY, "%s: entry buffer too small: %llu entries needed, capacity %llu", who, (unsigned long long)got[0],
                         (unsigned long long)cap);
    RC_TRY(h.fetch(entries, d_entries, got[0] * sizeof(smafa_table_entry)));
    for (const Staged &a : arrays) RC_TRY(h.fetch(a.out, a.dev, a.bytes));
    RC_TRY(h.wait());
    trim({&J.out});
    return SMAFA_OK;
}

}  // extern "C++"

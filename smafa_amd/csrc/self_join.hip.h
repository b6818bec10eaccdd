// self_join.hip.h — host code of the self-join of a resident store.  Two drivers walk the store and know no consumer: join_pass (every
// row against the rows behind it) and delta_pass (the rows appended since a mark against the whole store).  Each cuts its spans
// its own way and runs every span through join_span, which scans the span's blocks piece by piece (join_pieces).  Twelve calls
// consume the pieces: join_pairs, join_components, join_levels, join_density, join_peaks, join_chimeras, join_neighbours, join_forest,
// join_reach_forest and join_stable (the reach forest's passes, then its own) over join_pass, delta_pairs and delta_components
// over delta_pass.  A call is a JoinCall between join_begin and join_finish with one
// or more JoinConsumers: timed_consumer (a kernel per piece), watching (that, gated on a device counter read at every wait),
// keeping_consumer (that, with J.kept grown by the gate).  Their C ABI is self_join_abi.hip.h.
// What the calls share behind the join: read_ctl (the totals of J.ctl and the wait that brings them), kept_plan and kept_piece (the
// kept list read once, or the store joined again), join_flatten (the last launch, waited for), and for the two forests span_classes
// (the weight classes one after another, over either list form) and star_roots.  What their kernels share is piece.hip.h.
// Included once by engine.hip, inside namespace smafa, behind smafa_db and scan_range.
#pragma once

// one call's state on the host
struct JoinCall {
    smafa_db *db;
    bool no_scans = false;  // one row, or a bound no two rows can exceed: nothing to scan (a scan would list all n^2 pairs to learn "one set")
    bool nothing = false;   // join_begin: too few rows for any work, the zeroed counters are the result
    bool inverted = false;  // this call launched inverse_order_kernel
    bool delta = false;     // a delta call: its records come from smafa_dl::gather_records_kernel
    double *slot = nullptr;      // the timed pass whose events are not read yet: the J.*_ms it is booked to ...
    const char *what = nullptr;  // ... and its level-3 trace text (nullptr: none)
    unsigned long long ctl_seen = 0;  // J.ctl[0] as a watching consumer last read it, in front of a piece's wait: what the call's kernels
                                      // counted there over the pieces before the one just scanned — pairs kept (density, peaks, forests),
                                      // entries appended (neighbours), labels that are none (components update)
};

// a piece's finished list: rows (record of the piece, subject, distance) of block records p0 + b + S * k, k < R
struct JoinPiece {
    const smafa_hit *list;
    unsigned long long count;  // > 0, and all of them in the list
    uint32_t p0, S, R;
    const uint32_t *order;  // position -> subject of the list's queries (nullptr: the list names subjects already)
};

// What a call does with the pieces of one join.  A new consumer supplies `take` (timed_consumer: from its launch) — and whatever
// it wants in front of and behind the join — and never touches join_pass.
struct JoinConsumer {
    std::function<int(const JoinPiece &)> take;  // enqueues the kernel that reads the piece's list
    std::function<int()> before_wait;            // optional: enqueued in front of the one host wait of every piece
    bool used = false;                           // some piece was taken: the kernel belongs on the call's list
};

static dim3 row_grid(uint32_t n) { return dim3((n + 255u) / 256u); }
static dim3 list_grid(unsigned long long count) { return dim3((uint32_t)std::min<uint64_t>(2048, (count + 255) / 256)); }

// A timed pass on the join's stream: timed_begin, the launches, timed_end — or timed_pass around a single launch.  The slot of J
// the time belongs to is given with the launch; the events are read later, after a wait that the call needs anyway
// (timed_sync) — never by a wait of their own.
static int timed_begin(JoinCall &c, double *slot, const char *what) {
    smafa_db *db = c.db;
    auto &J = db->join;
    c.slot = slot, c.what = what;
    HIP_TRY(hipEventRecord(J.ev[2], db->stream));
    return SMAFA_OK;
}
static int timed_end(JoinCall &c, uint32_t launches = 1) {
    smafa_db *db = c.db;
    auto &J = db->join;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[3], db->stream));
    db->call_launches += launches;
    return SMAFA_OK;
}
template <class Launch>
static int timed_pass(JoinCall &c, double *slot, const char *what, Launch launch) {
    RC_TRY(timed_begin(c, slot, what));
    launch();
    return timed_end(c);
}

// the consumer whose pieces go to one launch each, timed into `slot`
template <class Launch>
static JoinConsumer timed_consumer(JoinCall &c, double *slot, const char *what, Launch launch) {
    return {[&c, slot, what, launch](const JoinPiece &p) { return timed_pass(c, slot, what, [&] { launch(p); }); }, nullptr};
}
static int consume(JoinConsumer &k, const JoinPiece &p) {
    k.used = true;
    return k.take(p);
}

// a wait of the call's, and the time of the pass before, which has finished by the time the wait returns
static int timed_sync(JoinCall &c) {
    smafa_db *db = c.db;
    HIP_TRY(hipStreamSynchronize(db->stream));
    float ms = 0.f;
    if (c.slot && hipEventElapsedTime(&ms, db->join.ev[2], db->join.ev[3]) == hipSuccess) {
        *c.slot += ms;
        if (c.what) log_line(3, "%s, %.3f ms", c.what, ms);
    }
    c.slot = nullptr, c.what = nullptr;
    return SMAFA_OK;
}

// the first `words` totals of J.ctl for the host, and the wait that brings them
static int read_ctl(JoinCall &c, unsigned long long *out, size_t words) {
    HIP_TRY(hipMemcpyAsync(out, c.db->join.ctl.p, words * sizeof *out, hipMemcpyDeviceToHost, c.db->stream));
    return timed_sync(c);
}

// What every call starts with: the statistics of the call before forgotten, `counters` zeros behind d_count, and — unless
// the store has fewer than min_rows rows (c.nothing) — the re-sort (once, in front: positions are final for the whole join),
// the events and the scratch list.
static int join_begin(JoinCall &c, unsigned long long *d_count, size_t counters, uint32_t min_rows) {
    smafa_db *db = c.db;
    auto &J = db->join;
    db->call_kernels.clear();
    db->call_ms = 0.f;
    db->call_launches = db->call_scans = db->last_launches = 0;
    db->timed = false;
    J.rec_ms = J.scan_ms = J.filter_ms = J.link_ms = J.flatten_ms = J.count_ms = J.select_ms = 0.0;
    J.blocks = J.rescans = J.joins = J.jump_rounds = 0;
    J.kept_stuck = false;
    RC_TRY(use_device(db));
    HIP_TRY(hipMemsetAsync(d_count, 0, counters * sizeof(unsigned long long), db->stream));
    db->call_timed = true;
    c.nothing = db->n < min_rows;
    if (c.nothing) return SMAFA_OK;
    if (!c.no_scans) RC_TRY(maybe_resort(db));
    for (hipEvent_t &e : J.ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    RC_TRY(db->count.ensure(sizeof(unsigned long long)));
    return !c.no_scans && db->hits_cap() < (1ull << 22) ? db->hits.ensure((1ull << 22) * sizeof(smafa_hit)) : SMAFA_OK;
}

// pos_of[] for the consumers with the exactly-once rule (position(query) < position(subject)): kept while the store stays as it is
static int join_positions(JoinCall &c) {
    smafa_db *db = c.db;
    auto &J = db->join;
    if (J.valid && J.generation == db->generation && J.n == db->n && J.resorts == db->resorts) return SMAFA_OK;
    J.valid = false;
    RC_TRY(J.pos_of.ensure((size_t)db->n * sizeof(uint32_t)));
    hipLaunchKernelGGL(smafa_join::inverse_order_kernel, row_grid((uint32_t)db->n), dim3(256), 0, db->stream, db->d_order, (uint32_t)db->n,
                       J.pos_of.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    J.generation = db->generation, J.n = db->n, J.resorts = db->resorts;
    J.valid = c.inverted = true;
    db->call_launches++;
    return SMAFA_OK;
}

// The scans of one block: records [q0, q_end) of the set in db->join_q against the wave tiles from tile_begin on, into the
// handle's scratch list, `piece` records per scan, each finished list handed to the consumer as `shape` with its list and
// count filled in.  The host waits for each piece's scan to learn its row count, and join_piece_rule (engine.h) says what
// follows: a piece that overflowed the scratch list is scanned again with the list grown to that count (exact at any
// capacity; a truncated list never reaches a consumer), or cut in half once the list would pass join_scratch_max rows; the
// reduced piece size is kept — by the caller, across its blocks — until a piece's count falls under a quarter of that
// ceiling.  rec_timed: the time of the records' pass (ev[0]..ev[1]) has been booked; where: the block, for the level-3 trace.
static int join_pieces(JoinCall &c, uint32_t scan_div, JoinConsumer &consumer, uint64_t q0, const uint64_t q_end, uint64_t &piece,
                       JoinPiece shape, uint32_t tile_begin, bool &rec_timed, const char *where) {
    smafa_db *db = c.db;
    auto &J = db->join;
    smafa_qset *qs = &db->join_q;
    while (q0 < q_end) {
        const uint64_t q1 = std::min<uint64_t>(q_end, q0 + piece);
        RC_TRY(scan_range(db, qs, (uint32_t)q0, (uint32_t)q1, scan_div, 0, db->hits.as<smafa_hit>(), db->hits_cap(),
                        db->count.as<unsigned long long>(), tile_begin));
        unsigned long long count = 0;
        HIP_TRY(hipMemcpyAsync(&count, db->count.p, sizeof count, hipMemcpyDeviceToHost, db->stream));
        if (consumer.before_wait) RC_TRY(consumer.before_wait());
        RC_TRY(timed_sync(c));  // (with it ends the consumer's pass over the piece before)
        const float before = db->call_ms;
        note_call_scan(db);
        const double scan_ms = db->call_ms - before;
        J.scan_ms += scan_ms;
        float ms = 0.f;
        if (!rec_timed && hipEventElapsedTime(&ms, J.ev[0], J.ev[1]) == hipSuccess) J.rec_ms += ms;
        rec_timed = true;
        log_line(3, "self-join: %s, records %llu..%llu: %llu rows, scan %.3f ms", where, (unsigned long long)q0, (unsigned long long)q1,
                 count, scan_ms);
        const PieceRule rule = join_piece_rule(count, db->hits_cap(), db->join_scratch_max, q1 - q0, piece, db->join_block);
        piece = rule.piece;
        if (rule.verdict != kPieceTake) J.rescans++;
        if (rule.verdict == kPieceFail)
            // (not SMAFA_ERR_CAPACITY: that code tells the caller of smafa_db_self_hits to grow ITS buffer and call again)
            return set_error(SMAFA_ERR_NOMEM,
                             "self-join: %llu rows of the store have %llu rows within %u of them, more than the scratch list may "
                             "hold (%llu rows)", (unsigned long long)(q1 - q0), count, scan_div, (unsigned long long)db->join_scratch_max);
        if (rule.verdict == kPieceGrow) RC_TRY(db->hits.ensure(count * sizeof(smafa_hit)));
        if (rule.verdict != kPieceTake) continue;  // the same rows, or their first half, once more
        shape.list = db->hits.as<smafa_hit>(), shape.count = count;
        if (count) RC_TRY(consume(consumer, shape));
        J.blocks++;
        q0 = q1;
    }
    return SMAFA_OK;
}

// How a driver cut one span: nq records in `padded` zeroed record slots (padded as qset_fill pads: whole 64-record chunks plus
// one), scanned as S blocks from wave tile tile_begin on, every piece shaped `shape`; block b is traced as "<what> <at>, block b of S".
struct JoinSpan {
    uint64_t nq, padded;
    uint32_t S;
    JoinPiece shape;
    uint32_t tile_begin;
    const char *what;
    uint64_t at;
};

// One span of either driver: the set in db->join_q gets the span's records — records(qrec) launches the one kernel that writes
// them, timed ev[0]..ev[1] —, then block b = 0 .. S - 1 is scanned over its records range(b) = {q0, q_end} through join_pieces, and
// a wait ends the span.  `piece` is the caller's: the reduced piece size outlives the span.
template <class Records, class Range>
static int join_span(JoinCall &c, uint32_t scan_div, JoinConsumer &consumer, uint64_t &piece, const JoinSpan &span, Records records,
                     Range range) {
    smafa_db *db = c.db;
    auto &J = db->join;
    smafa_qset *qs = &db->join_q;
    qs->nq = span.nq;
    qs->serial = g_qset_serial.fetch_add(1);
    RC_TRY(qs->qrec.ensure(span.padded * db->QS * sizeof(uint32_t)));
    RC_TRY(qs->thr.ensure(span.padded * sizeof(uint32_t)));
    HIP_TRY(hipEventRecord(J.ev[0], db->stream));
    HIP_TRY(hipMemsetAsync(qs->qrec.p, 0, span.padded * db->QS * sizeof(uint32_t), db->stream));
    records(qs->qrec.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[1], db->stream));
    db->call_launches++;
    bool rec_timed = false;
    for (uint32_t b = 0; b < span.S; b++) {
        const std::pair<uint64_t, uint64_t> q = range(b);
        char where[64];
        snprintf(where, sizeof where, "%s %llu, block %u of %u", span.what, (unsigned long long)span.at, b, span.S);
        RC_TRY(join_pieces(c, scan_div, consumer, q.first, q.second, piece, span.shape, span.tile_begin, rec_timed, where));
    }
    return timed_sync(c);  // the span's records are overwritten next
}

// The driver: every pair of the store's rows within scan_div of each other, once or twice, as the lists of PIECES to `consumer`.
// The store is walked in SPANS of join_stride x join_block consecutive positions.  A span's rows become query records on
// the device (store_records_kernel), dealt round-robin into join_stride BLOCKS: block b holds the span's positions b,
// b + S, b + 2S, ...  Per block the fixed-bound scan runs its records against the wave tiles from the span's first one to the
// end of the store — tiles in front of the span could only repeat pairs an earlier span has found — into the handle's
// scratch list, and the consumer's kernel reads that list behind the scan, on the same stream (join_pieces).
// Why interleaved: the store is sorted by filter bits, so a block of CONSECUTIVE positions is 65 536 rows whose surviving work
// sits in a few workgroups (profiles/r07_self_join.txt, stride 1 against 16).
static int join_pass(JoinCall &c, uint32_t scan_div, JoinConsumer &consumer) {
    smafa_db *db = c.db;
    db->join_q.db = db;
    const uint64_t span_rows = db->join_block * db->join_stride;
    uint64_t piece = db->join_block;  // rows per scan
    db->join.joins++;
    for (uint64_t p0 = 0; p0 < db->n; p0 += span_rows) {
        const uint64_t p1 = std::min<uint64_t>(db->n, p0 + span_rows), m = p1 - p0;
        const uint32_t S = (uint32_t)((m + db->join_block - 1) / db->join_block);  // blocks of this span
        const uint32_t R = (uint32_t)((m + S - 1) / S);                            // rows of its fullest block
        // (a short block's last record slot stays zero too)
        const uint64_t padded = std::max<uint64_t>(((uint64_t)S * R + 63) / 64 * 64, 64) + 64;
        const uint32_t t0 = (uint32_t)(p0 / kWaveTile), t1 = (uint32_t)((p1 - 1) / kWaveTile) + 1u;
        const JoinPiece shape{nullptr, 0, (uint32_t)p0, S, R, db->d_order};
        const JoinSpan span{/* nq */ (uint64_t)S * R, padded, S, shape, /* tile_begin */ t0, "span at", /* at */ p0};
        RC_TRY(join_span(c, scan_div, consumer, piece, span,
                         [&](uint32_t *qrec) {
                             hipLaunchKernelGGL(smafa_join::store_records_kernel, dim3(t1 - t0), dim3(256), 0, db->stream,
                                                reinterpret_cast<const uint4 *>(db->d_planes), db->P, db->PQ, db->W, db->QS, (uint32_t)p0,
                                                (uint32_t)p1, S, R, qrec);
                         },
                         [&](uint32_t b) {  // positions b, b + S, ... of the span
                             return std::pair<uint64_t, uint64_t>((uint64_t)b * R, (uint64_t)b * R + (m - b + S - 1) / S);
                         }));
    }
    return SMAFA_OK;
}

// The driver of the delta join: every pair within scan_div that a NEW row — subject numbers first_row .. n-1 — forms with any
// row of the store, new or old, as the lists of pieces to `consumer`; a pair of two new rows comes twice, once from each
// side, the self-pairs come too.  The new rows are walked in subject-number order — the order they were appended in — in
// spans of join_stride x join_block rows, cut into blocks of join_block consecutive ones.  A span's rows, wherever the
// sort has put them, become query records on the device (gather_records_kernel through pos_of[], which the caller has
// made current), and every block is scanned against ALL tiles: the same scans as the full join's, chosen by the same
// scan_plan.h, and an index probe where a current block index serves the bound.  A piece is shaped {p0 = the span's first
// row, counted from first_row, S = 1, R = 0xffffffff, order = J.rows}: list query r is J.rows[p0 + r] for the consumers
// of the full join too, unchanged.  The piece protocol is join_pieces', the reduced piece size carried across the blocks.
static int delta_pass(JoinCall &c, uint32_t first_row, uint32_t scan_div, JoinConsumer &consumer) {
    smafa_db *db = c.db;
    auto &J = db->join;
    db->join_q.db = db;
    const uint64_t new_rows = db->n - first_row, span_rows = db->join_block * db->join_stride;
    uint64_t piece = db->join_block;  // rows per scan
    RC_TRY(J.rows.ensure(new_rows * sizeof(uint32_t)));
    J.joins++;
    for (uint64_t a0 = 0; a0 < new_rows; a0 += span_rows) {
        const uint64_t m = std::min<uint64_t>(span_rows, new_rows - a0);
        const uint32_t S = (uint32_t)((m + db->join_block - 1) / db->join_block);  // blocks of this span
        const uint64_t padded = std::max<uint64_t>((m + 63) / 64 * 64, 64) + 64;
        const JoinPiece shape{nullptr, 0, (uint32_t)a0, 1u, 0xffffffffu, J.rows.as<uint32_t>()};
        const JoinSpan span{/* nq */ m, padded, S, shape, /* tile_begin */ 0u, "new rows from", /* at */ first_row + a0};
        RC_TRY(join_span(c, scan_div, consumer, piece, span,
                         [&](uint32_t *qrec) {
                             hipLaunchKernelGGL(smafa_dl::gather_records_kernel, list_grid(m * db->P * db->W), dim3(256), 0, db->stream,
                                                db->d_planes, J.pos_of.as<uint32_t>(), db->P, db->PQ, db->W, db->QS,
                                                (uint32_t)(first_row + a0), (uint32_t)m, qrec, J.rows.as<uint32_t>() + a0);
                         },
                         [&](uint32_t b) {  // join_block consecutive rows
                             const uint64_t q0 = (uint64_t)b * db->join_block;
                             return std::pair<uint64_t, uint64_t>(q0, std::min<uint64_t>(m, q0 + db->join_block));
                         }));
    }
    return SMAFA_OK;
}

// What every call ends with: its stage times in smafa_last_scan_ms, and the kernels of the shared path in front of its own
static void join_finish(JoinCall &c) {
    smafa_db *db = c.db;
    const auto &J = db->join;
    db->call_ms += (float)(J.rec_ms + J.filter_ms + J.count_ms + J.link_ms + J.flatten_ms + J.select_ms);
    db->call_timed = true;  // (scan_range cleared it)
    if (!c.no_scans) note_call_kernel(db, c.delta ? "smafa_dl::gather_records_kernel" : "smafa_join::store_records_kernel");
    if (c.inverted) note_call_kernel(db, "smafa_join::inverse_order_kernel");
}

// ---- the kept pair list of the density and peaks calls: what the counting join kept, so that the linking pass need not join again
static uint64_t kept_room(const smafa_db *db) { return std::min<uint64_t>(db->join.kept.cap / sizeof(smafa_hit), db->density_keep_max); }

// room in J.kept for `rows` rows, at most density_keep_max of them; the first `live` rows are carried over
static int grow_kept(smafa_db *db, uint64_t rows, uint64_t live) {
    DevBuf &K = db->join.kept;
    rows = std::min<uint64_t>(rows, db->density_keep_max);
    if (rows * sizeof(smafa_hit) <= K.cap) return SMAFA_OK;
    const uint64_t want = std::min<uint64_t>(db->density_keep_max, std::max<uint64_t>(rows, K.cap / sizeof(smafa_hit) * 2));
    DevBuf bigger;  // (a bare hipMalloc: a failure here is no failure of the call and leaves no text in smafa_last_error())
    if (hipMalloc(&bigger.p, want * sizeof(smafa_hit)) == hipSuccess) bigger.cap = want * sizeof(smafa_hit);
    if (!bigger.p) {
        // no room for a larger list: the one there is stays as it is and overflows — counted, not stored — and the call
        // falls back to the second join, which needs no list and gives the same bytes
        (void)hipGetLastError();
        db->join.kept_stuck = true;
        log_line(2, "density: no memory for a kept pair list of %llu rows; the store will be joined twice", (unsigned long long)want);
        return SMAFA_OK;
    }
    hipError_t e = hipSuccess;
    if (live) e = hipMemcpyAsync(bigger.p, K.p, live * sizeof(smafa_hit), hipMemcpyDeviceToDevice, db->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) {
        bigger.release();
        return set_error(SMAFA_ERR_DEVICE, "density: moving the kept pair list failed: %s", hipGetErrorString(e));
    }
    K.release();
    K = bigger;
    return SMAFA_OK;
}

// ---- a consumer that watches J.ctl[0], a total its own kernel raises
static int read_watched(JoinCall &c) {
    HIP_TRY(hipMemcpyAsync(&c.ctl_seen, c.db->join.ctl.p, sizeof c.ctl_seen, hipMemcpyDeviceToHost, c.db->stream));
    return SMAFA_OK;
}
// `k` with the total read back into c.ctl_seen in front of every piece's wait (every pass in front of the piece's scan has ended
// with it: exact as of the pieces before), and gate(that total, the piece) in front of every take — it makes room for what the
// piece may add, or fails the call (count <= the scratch capacity: a truncated list was scanned again).
template <class Gate>
static JoinConsumer watching(JoinCall &c, JoinConsumer k, Gate gate) {
    k.before_wait = [&c] { return read_watched(c); };
    k.take = [&c, gate, timed = k.take](const JoinPiece &p) {
        RC_TRY(gate(c.ctl_seen, p));
        return timed(p);
    };
    return k;
}

// A consumer whose kernel also moves pairs to J.kept: watching the kept total, the list given room for whatever the piece keeps
// on top of that, while the knob allows it.
template <class Launch>
static JoinConsumer keeping_consumer(JoinCall &c, double *slot, const char *what, Launch launch) {
    return watching(c, timed_consumer(c, slot, what, launch), [&c](unsigned long long kept, const JoinPiece &p) {
        return c.db->join.kept_stuck ? SMAFA_OK : grow_kept(c.db, kept + p.count, std::min<uint64_t>(kept, kept_room(c.db)));
    });
}

// Every count is final and `total` pairs were kept or counted over.  None: there is nothing to link.  All of them in J.kept: ONE
// launch of the linking kernel over that list (kept_piece) replaces a join.  Else the store is joined a second time with the
// linking kernel reading each piece's raw list — no list needed, the same bytes.
enum KeptPlan { kKeptNothing, kKeptOnce, kKeptJoinAgain };
static KeptPlan kept_plan(const smafa_db *db, unsigned long long total, const char *who, const char *verb) {
    if (total == 0) return kKeptNothing;
    if (total <= kept_room(db)) return kKeptOnce;
    log_line(3, "%s: %llu pairs, the kept list holds %llu: joining once more to %s", who, total, (unsigned long long)kept_room(db), verb);
    return kKeptJoinAgain;
}
static JoinPiece kept_piece(const smafa_db *db, unsigned long long total) { return {db->join.kept.as<smafa_hit>(), total, 0u, 1u, 1u, nullptr}; }

// smafa_db_self_launch: every unordered pair within max_div, once.  join_filter_kernel moves the rows of a piece's list with
// position(query) < position(subject) to the caller's list.
static int join_pairs(smafa_db *db, uint32_t max_div, smafa_hit *d_hits, uint64_t cap, unsigned long long *d_count) {
    auto &J = db->join;
    JoinCall c{db};
    RC_TRY(join_begin(c, d_count, 1, 2));
    if (c.nothing) return SMAFA_OK;
    RC_TRY(join_positions(c));
    JoinConsumer filter = timed_consumer(c, &J.filter_ms, nullptr, [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_join::join_filter_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R,
                           p.order, J.pos_of.as<uint32_t>(), d_hits, (unsigned long long)cap, d_count);
    });
    RC_TRY(join_pass(c, max_div, filter));
    join_finish(c);
    if (filter.used) note_call_kernel(db, "smafa_join::join_filter_kernel");
    log_line(2, "self-join of %u rows at bound %u: %u scans (%u of them repeats), records %.3f ms, scans %.3f ms, filter %.3f ms",
             (uint32_t)db->n, max_div, J.blocks + J.rescans, J.rescans, J.rec_ms, J.scan_ms, J.filter_ms);
    return SMAFA_OK;
}

// the one launch behind the last pass of a linking call (the kernel boundary makes every hook visible), waited for
template <class Launch>
static int join_flatten(JoinCall &c, Launch launch) {
    RC_TRY(timed_sync(c));
    RC_TRY(timed_pass(c, &c.db->join.flatten_ms, nullptr, launch));
    return timed_sync(c);
}

// smafa_db_self_components_launch (components.hip.h): link_rows_kernel unites the two subjects of every row in J.parent — no
// pos_of[], no filter, no rows for the caller — and after the last piece flatten_labels_kernel writes labels[i] = the smallest
// subject number of i's component and counts the representatives into *d_count.
static int join_components(smafa_db *db, uint32_t max_div, uint32_t *d_labels, unsigned long long *d_count) {
    auto &J = db->join;
    const bool all_near = max_div >= db->L;
    JoinCall c{db, db->n < 2 || all_near};
    RC_TRY(join_begin(c, d_count, 1, 1));
    if (c.nothing) return SMAFA_OK;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(J.parent.ensure((size_t)n * sizeof(uint32_t)));
    RC_TRY(timed_begin(c, &J.link_ms, "components: parent[] initialised"));
    if (all_near)  // parent[i] = i — or 0 everywhere where every row is within the bound of row 0
        HIP_TRY(hipMemsetAsync(J.parent.p, 0, (size_t)n * sizeof(uint32_t), db->stream));
    else
        hipLaunchKernelGGL(smafa_cc::init_labels_kernel, row_grid(n), dim3(256), 0, db->stream, J.parent.as<uint32_t>(), n);
    RC_TRY(timed_end(c, all_near ? 0u : 1u));
    JoinConsumer link = timed_consumer(c, &J.link_ms, "components: parent[] linked with a piece's rows", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_cc::link_rows_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R, p.order,
                           J.parent.as<uint32_t>());
    });
    if (!c.no_scans) RC_TRY(join_pass(c, max_div, link));
    RC_TRY(join_flatten(c, [&] {
        hipLaunchKernelGGL(smafa_cc::flatten_labels_kernel, row_grid(n), dim3(256), 0, db->stream, J.parent.as<uint32_t>(), n, d_labels, d_count);
    }));
    join_finish(c);
    if (!all_near) note_call_kernel(db, "smafa_cc::init_labels_kernel");
    if (link.used) note_call_kernel(db, "smafa_cc::link_rows_kernel");
    note_call_kernel(db, "smafa_cc::flatten_labels_kernel");
    log_line(2, "components of %u rows at bound %u: %u scans (%u of them repeats), records %.3f ms, scans %.3f ms, link %.3f ms, "
             "flatten %.3f ms", n, max_div, J.blocks + J.rescans, J.rescans, J.rec_ms, J.scan_ms, J.link_ms, J.flatten_ms);
    return SMAFA_OK;
}

// smafa_db_self_since_launch (delta.hip.h): every unordered pair within max_div whose larger subject number is >= first_row,
// once.  delta_filter_kernel keeps the rows of a piece's list whose subject number is below their query's.
// first_row <= n
static int delta_pairs(smafa_db *db, uint32_t first_row, uint32_t max_div, smafa_hit *d_hits, uint64_t cap, unsigned long long *d_count) {
    auto &J = db->join;
    JoinCall c{db, first_row >= db->n};  // no new row: no pair
    c.delta = true;
    RC_TRY(join_begin(c, d_count, 1, 2));
    if (c.nothing || c.no_scans) return SMAFA_OK;
    RC_TRY(join_positions(c));
    JoinConsumer filter = timed_consumer(c, &J.filter_ms, nullptr, [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_dl::delta_filter_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.order,
                           d_hits, (unsigned long long)cap, d_count);
    });
    RC_TRY(delta_pass(c, first_row, max_div, filter));
    join_finish(c);
    if (filter.used) note_call_kernel(db, "smafa_dl::delta_filter_kernel");
    log_line(2, "delta self-join of %u rows from row %u at bound %u: %u scans (%u of them repeats), gather %.3f ms, scans %.3f ms, "
             "filter %.3f ms", (uint32_t)db->n, first_row, max_div, J.blocks + J.rescans, J.rescans, J.rec_ms, J.scan_ms, J.filter_ms);
    return SMAFA_OK;
}

// smafa_db_self_components_update_launch (delta.hip.h, components.hip.h): d_labels holds, in its first first_row entries, the
// labels of the store's first first_row rows at this bound, and leaves as the labels of the whole store.  seed_parents_kernel
// makes parent[] of them — and counts the entries that cannot be such labels —, link_rows_kernel unites the two subjects of
// every row of the delta join's pieces, and flatten_labels_kernel writes the labels and counts the representatives: two sets of
// old rows can only have become one through a new row, and every pair with a new row is in the delta join.  The count of
// bad entries is read at every piece's wait and in front of the flatten launch, which does not run — d_labels is not
// written — once it is non-zero.
// first_row <= n
static int delta_components(smafa_db *db, uint32_t first_row, uint32_t max_div, uint32_t *d_labels, unsigned long long *d_count) {
    auto &J = db->join;
    const bool all_near = max_div >= db->L;
    JoinCall c{db, db->n < 2 || all_near || first_row >= db->n};
    c.delta = true;
    RC_TRY(join_begin(c, d_count, 1, 1));
    if (c.nothing) return SMAFA_OK;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(J.parent.ensure((size_t)n * sizeof(uint32_t)));
    RC_TRY(J.ctl.ensure(sizeof(unsigned long long)));
    RC_TRY(timed_begin(c, &J.link_ms, "components update: parent[] seeded"));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, sizeof(unsigned long long), db->stream));
    if (all_near)  // every row is within the bound of row 0
        HIP_TRY(hipMemsetAsync(J.parent.p, 0, (size_t)n * sizeof(uint32_t), db->stream));
    else
        hipLaunchKernelGGL(smafa_dl::seed_parents_kernel, row_grid(n), dim3(256), 0, db->stream, d_labels, first_row, n,
                           J.parent.as<uint32_t>(), J.ctl.as<unsigned long long>());
    RC_TRY(timed_end(c, all_near ? 0u : 1u));
    const unsigned long long &bad = c.ctl_seen;
    const auto bad_labels = [&] {
        return set_error(SMAFA_ERR_INVALID, "components update: %llu of the first %u labels are no labels of a store of %u rows (a label is "
                         "at most its row's number, and its own label)", bad, first_row, first_row);
    };
    JoinConsumer link = timed_consumer(c, &J.link_ms, "components update: parent[] linked with a piece's rows", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_cc::link_rows_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R, p.order,
                           J.parent.as<uint32_t>());
    });
    link = watching(c, link, [&](unsigned long long, const JoinPiece &) { return bad ? bad_labels() : SMAFA_OK; });
    if (!c.no_scans) {
        RC_TRY(join_positions(c));
        RC_TRY(delta_pass(c, first_row, max_div, link));
    }
    RC_TRY(read_watched(c));
    RC_TRY(timed_sync(c));
    if (bad) return bad_labels();
    RC_TRY(timed_pass(c, &J.flatten_ms, nullptr, [&] {
        hipLaunchKernelGGL(smafa_cc::flatten_labels_kernel, row_grid(n), dim3(256), 0, db->stream, J.parent.as<uint32_t>(), n, d_labels, d_count);
    }));
    RC_TRY(timed_sync(c));
    join_finish(c);
    if (!all_near) note_call_kernel(db, "smafa_dl::seed_parents_kernel");
    if (link.used) note_call_kernel(db, "smafa_cc::link_rows_kernel");
    note_call_kernel(db, "smafa_cc::flatten_labels_kernel");
    log_line(2, "components update of %u rows from row %u at bound %u: %u scans (%u of them repeats), gather %.3f ms, scans %.3f ms, "
             "seed + link %.3f ms, flatten %.3f ms", n, first_row, max_div, J.blocks + J.rescans, J.rescans, J.rec_ms, J.scan_ms, J.link_ms,
             J.flatten_ms);
    return SMAFA_OK;
}

// smafa_db_self_levels_launch (levels.hip.h): d_labels is (max_div + 1) x n, d_count as many counters, J.parent one union-find per
// SCANNED level (E = min(max_div, L - 1) + 1 of them; the levels above are all zeros and need no scan).  The join runs once at
// bound E - 1 and hook_levels_kernel unites the subjects of a row at every level from its distance upwards;
// flatten_levels_kernel writes every level in one launch.
static int join_levels(smafa_db *db, uint32_t max_div, uint32_t *d_labels, unsigned long long *d_count) {
    auto &J = db->join;
    const uint32_t n_levels = max_div + 1u, E = std::min(n_levels, std::max<uint32_t>(db->L, 1u)), scan_div = E - 1u;
    JoinCall c{db, db->n < 2};
    RC_TRY(join_begin(c, d_count, n_levels, 1));
    if (c.nothing) return SMAFA_OK;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(J.parent.ensure((size_t)n * E * sizeof(uint32_t)));
    RC_TRY(timed_pass(c, &J.link_ms, "levels: parent[] initialised", [&] {
        hipLaunchKernelGGL(smafa_lv::init_levels_kernel, row_grid(n), dim3(256), 0, db->stream, J.parent.as<uint32_t>(), n, E);
    }));
    JoinConsumer hook = timed_consumer(c, &J.link_ms, "levels: parent[] linked with a piece's rows", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_lv::hook_levels_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R, p.order,
                           J.parent.as<uint32_t>(), n, E);
    });
    if (!c.no_scans) RC_TRY(join_pass(c, scan_div, hook));
    RC_TRY(join_flatten(c, [&] {
        hipLaunchKernelGGL(smafa_lv::flatten_levels_kernel, row_grid(n), dim3(256), 0, db->stream, J.parent.as<uint32_t>(), n, E, n_levels,
                           d_labels, d_count);
    }));
    join_finish(c);
    note_call_kernel(db, "smafa_lv::init_levels_kernel");
    if (hook.used) note_call_kernel(db, "smafa_lv::hook_levels_kernel");
    note_call_kernel(db, "smafa_lv::flatten_levels_kernel");
    log_line(2, "levels 0..%u of %u rows, joined at bound %u: %u scans (%u of them repeats), records %.3f ms, scans %.3f ms, "
             "link %.3f ms, flatten %.3f ms", max_div, n, scan_div, J.blocks + J.rescans, J.rescans, J.rec_ms, J.scan_ms, J.link_ms, J.flatten_ms);
    return SMAFA_OK;
}

// smafa_db_self_density_launch (density.hip.h): d_labels is n labels, d_count three counters, J.parent holds parent[], degree[]
// and attach[].  The join runs at max_div with count_keep_kernel per piece (the exactly-once rule, so pos_of[] as for the plain
// join), which raises both degrees of every kept pair and moves the pair to J.kept while that has room; the kept total then
// decides (kept_plan) how link_cores_kernel gets the pairs.  No core row at all: no link.  min_pts <= 1 without degrees:
// nothing to count, the one join links directly, as components.
// min_pts >= 1; d_degrees: n entries, or nullptr
static int join_density(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t *d_degrees, uint32_t *d_labels, unsigned long long *d_count) {
    auto &J = db->join;
    const bool counting = min_pts > 1u || d_degrees, all_near = max_div >= db->L;
    JoinCall c{db, db->n < 2 || all_near};
    RC_TRY(join_begin(c, d_count, 3, 1));
    if (c.nothing) return SMAFA_OK;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(J.parent.ensure((size_t)n * 3u * sizeof(uint32_t)));
    RC_TRY(J.ctl.ensure(2 * sizeof(unsigned long long)));
    uint32_t *const parent = J.parent.as<uint32_t>(), *const degree = parent + n, *const attach = parent + 2 * (size_t)n;
    RC_TRY(timed_begin(c, counting ? &J.count_ms : &J.link_ms, "density: parent[] initialised"));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, 2 * sizeof(unsigned long long), db->stream));
    // every row within the bound of every other: degrees n - 1, one set
    hipLaunchKernelGGL(smafa_dn::init_density_kernel, row_grid(n), dim3(256), 0, db->stream, degree, parent, attach, n,
                       all_near ? n - 1u : 0u, all_near ? 1u : 0u);
    RC_TRY(timed_end(c));
    JoinConsumer count = keeping_consumer(c, &J.count_ms, "density: parent[] untouched, a piece's rows counted", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_dn::count_keep_kernel, list_grid(p.count), dim3(256), 0,
                           db->stream, p.list, p.count, p.p0, p.S, p.R, p.order, J.pos_of.as<uint32_t>(), degree, min_pts,
                           J.kept.as<smafa_hit>(), (unsigned long long)kept_room(db), J.ctl.as<unsigned long long>());
    });
    JoinConsumer link = timed_consumer(c, &J.link_ms, "density: parent[] linked with a piece's rows", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_dn::link_cores_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R, p.order,
                           degree, min_pts, parent, attach);
    });
    if (!c.no_scans && counting) {
        RC_TRY(join_positions(c));
        RC_TRY(join_pass(c, max_div, count));
        unsigned long long ctl[2] = {0, 0};  // every degree is final: the kept total; "some row is core"
        RC_TRY(read_ctl(c, ctl, 2));
        // (no core row: nothing to link, every row keeps the set and the attach[] it was given)
        const KeptPlan plan = min_pts > 1u && !ctl[1] ? kKeptNothing : kept_plan(db, ctl[0], "density", "link");
        if (plan == kKeptOnce) RC_TRY(consume(link, kept_piece(db, ctl[0])));
        if (plan == kKeptJoinAgain) RC_TRY(join_pass(c, max_div, link));
    } else if (!c.no_scans) {
        RC_TRY(join_pass(c, max_div, link));
    }
    RC_TRY(join_flatten(c, [&] {
        hipLaunchKernelGGL(smafa_dn::flatten_density_kernel, row_grid(n), dim3(256), 0, db->stream, parent, degree, attach, n, min_pts,
                           d_labels, d_degrees, d_count);
    }));
    join_finish(c);
    note_call_kernel(db, "smafa_dn::init_density_kernel");
    if (count.used) note_call_kernel(db, "smafa_dn::count_keep_kernel");
    if (link.used) note_call_kernel(db, "smafa_dn::link_cores_kernel");
    note_call_kernel(db, "smafa_dn::flatten_density_kernel");
    log_line(2, "density of %u rows at bound %u, min_pts %u: %u scans (%u of them repeats) in %u join%s, records %.3f ms, scans %.3f ms, "
             "count/keep %.3f ms, link %.3f ms, flatten %.3f ms", n, max_div, min_pts, J.blocks + J.rescans, J.rescans, J.joins,
             J.joins == 1 ? "" : "s", J.rec_ms, J.scan_ms, J.count_ms, J.link_ms, J.flatten_ms);
    return SMAFA_OK;
}

// settle_kernel behind the climb, then pointer doubling until a round changes nothing; without a climb every label is its own
// row or the crown: flat already
static int peaks_settle(JoinCall &c, bool crowned, bool climbed, uint32_t *d_labels, uint32_t *d_parents, uint32_t *d_weights,
                        unsigned long long *d_count) {
    smafa_db *db = c.db;
    auto &J = db->join;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(join_flatten(c, [&] {
        hipLaunchKernelGGL(smafa_pk::settle_kernel, row_grid(n), dim3(256), 0,
                           db->stream, J.parent.as<unsigned long long>(), J.parent.as<uint32_t>() + 2 * (size_t)n, n,
                           crowned ? J.ctl.as<unsigned long long>() + 2 : (const unsigned long long *)nullptr, d_labels, d_parents,
                           d_weights, d_count);
    }));
    for (uint32_t changed = climbed ? 1u : 0u; changed; J.jump_rounds++) {
        if (J.jump_rounds == 33u) return set_error(SMAFA_ERR_DEVICE, "peaks: parent[] is no forest (33 jump rounds did not flatten it)");
        uint32_t *const d_changed = reinterpret_cast<uint32_t *>(J.ctl.as<unsigned long long>() + 3);
        HIP_TRY(hipMemsetAsync(d_changed, 0, sizeof(uint32_t), db->stream));
        RC_TRY(timed_pass(c, &J.flatten_ms, nullptr, [&] {
            hipLaunchKernelGGL(smafa_pk::jump_kernel, row_grid(n), dim3(256), 0, db->stream, d_labels, n, d_changed);
        }));
        HIP_TRY(hipMemcpyAsync(&changed, d_changed, sizeof changed, hipMemcpyDeviceToHost, db->stream));
        RC_TRY(timed_sync(c));
    }
    return SMAFA_OK;
}

// smafa_db_self_peaks_launch (peaks.hip.h): d_labels is n labels, d_count one counter, J.parent holds best[] (the 8-byte one
// first) and weight[].  The join runs at max_div with weigh_keep_kernel per piece (the exactly-once rule), which raises both
// weights of every kept pair within the radius and moves every kept pair to J.kept while that has room; the kept total then
// decides (kept_plan) how climb_kernel gets the pairs.  settle_kernel writes parents, weights and the peak count, and jump_kernel
// rounds flatten the labels.  max_div >= seq_len (crowned: no two rows can exceed the bound, the pairs are needed for the
// weights alone): the join, if any, runs at the radius and only counts — nothing is kept or climbed — and crown_kernel finds
// the one peak.
// radius <= max_div; d_parents, d_weights: n entries each, or nullptr
static int join_peaks(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t *d_labels, uint32_t *d_parents, uint32_t *d_weights,
                      unsigned long long *d_count) {
    auto &J = db->join;
    const bool crowned = max_div >= db->L;
    const uint32_t scan_div = crowned ? radius : max_div;
    JoinCall c{db, db->n < 2 || scan_div >= db->L};
    RC_TRY(join_begin(c, d_count, 1, 1));
    if (c.nothing) return SMAFA_OK;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(J.parent.ensure((size_t)n * 3u * sizeof(uint32_t)));
    RC_TRY(J.ctl.ensure(4 * sizeof(unsigned long long)));
    unsigned long long *const best = J.parent.as<unsigned long long>();
    uint32_t *const weight = J.parent.as<uint32_t>() + 2 * (size_t)n;
    RC_TRY(timed_begin(c, &J.count_ms, "peaks: weight[] initialised"));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, 4 * sizeof(unsigned long long), db->stream));
    // every row within the radius of every other: weights n
    hipLaunchKernelGGL(smafa_pk::init_peaks_kernel, row_grid(n), dim3(256), 0, db->stream, best, weight, n, scan_div >= db->L ? n : 1u, 0u);
    RC_TRY(timed_end(c));
    const auto launch_weigh = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_pk::weigh_keep_kernel, list_grid(p.count), dim3(256), 0,
                           db->stream, p.list, p.count, p.p0, p.S, p.R, p.order, J.pos_of.as<uint32_t>(), weight, radius,
                           J.kept.as<smafa_hit>(), crowned ? 0ull : (unsigned long long)kept_room(db), J.ctl.as<unsigned long long>());
    };
    const auto launch_climb = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_pk::climb_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R, p.order,
                           weight, best);
    };
    const char *const weighed = "peaks: a piece's rows weighed", *const climbed = "peaks: a piece's rows climbed";
    // at a crowned bound nothing is kept
    JoinConsumer weigh = crowned ? timed_consumer(c, &J.count_ms, weighed, launch_weigh) : keeping_consumer(c, &J.count_ms, weighed, launch_weigh);
    JoinConsumer climb = timed_consumer(c, &J.link_ms, climbed, launch_climb);
    if (!c.no_scans) {
        RC_TRY(join_positions(c));
        RC_TRY(join_pass(c, scan_div, weigh));
    }
    unsigned long long kept_total = 0;
    RC_TRY(read_ctl(c, &kept_total, 1));
    // every weight is final: the rows' own keys — or the crown — and the climb over the kept list, if that has every pair, in ONE
    // timed pass (its trace text: the last kind of pass that ran)
    const KeptPlan plan = crowned ? kKeptNothing : kept_plan(db, kept_total, "peaks", "climb");
    RC_TRY(timed_begin(c, &J.link_ms, plan == kKeptOnce ? climbed : weigh.used ? weighed : "peaks: weight[] initialised"));
    if (crowned)
        hipLaunchKernelGGL(smafa_pk::crown_kernel, row_grid(n), dim3(256), 0, db->stream, weight, n, J.ctl.as<unsigned long long>() + 2);
    else
        hipLaunchKernelGGL(smafa_pk::init_peaks_kernel, row_grid(n), dim3(256), 0, db->stream, best, weight, n, 0u, 1u);
    HIP_TRY(hipGetLastError());
    climb.used = plan == kKeptOnce;
    if (climb.used) launch_climb(kept_piece(db, kept_total));
    RC_TRY(timed_end(c, climb.used ? 2u : 1u));
    if (plan == kKeptJoinAgain) RC_TRY(join_pass(c, scan_div, climb));
    RC_TRY(peaks_settle(c, crowned, climb.used, d_labels, d_parents, d_weights, d_count));
    join_finish(c);
    note_call_kernel(db, "smafa_pk::init_peaks_kernel");
    if (weigh.used) note_call_kernel(db, "smafa_pk::weigh_keep_kernel");
    if (climb.used) note_call_kernel(db, "smafa_pk::climb_kernel");
    if (crowned) note_call_kernel(db, "smafa_pk::crown_kernel");
    note_call_kernel(db, "smafa_pk::settle_kernel");
    if (J.jump_rounds) note_call_kernel(db, "smafa_pk::jump_kernel");
    log_line(2, "peaks of %u rows at bound %u, radius %u: %u scans (%u of them repeats) in %u join%s, records %.3f ms, scans %.3f ms, "
             "weigh/keep %.3f ms, climb %.3f ms, settle+jump %.3f ms in %u jump round%s", n, max_div, radius, J.blocks + J.rescans,
             J.rescans, J.joins, J.joins == 1 ? "" : "s", J.rec_ms, J.scan_ms, J.count_ms, J.link_ms, J.flatten_ms, J.jump_rounds,
             J.jump_rounds == 1 ? "" : "s");
    return SMAFA_OK;
}

// smafa_db_self_peaks_weighted_launch: join_peaks with the caller's weights (peaks.hip.h) — a call of its own beside it, with the
// same passes and the same kernels: init_peaks_kernel in mode 2 where it runs in mode 0 there, weigh_keep_kernel with the weights as
// its last argument; keys, the kept list, the climb, the settle pass and the jump rounds are join_peaks's.  ctl[1] takes the sum of the weights, read
// behind the seed launch: past 2^32 - 1 the call fails before anything is weighed.  A radius no two rows can exceed: every weight
// is that sum (init_peaks_kernel, mode 0).
// radius <= max_div; d_weights_in: n entries; d_parents, d_weights: n entries each, or nullptr
static int join_peaks_weighted(smafa_db *db, const char *who, uint32_t max_div, uint32_t radius, const uint32_t *d_weights_in, uint32_t *d_labels,
                               uint32_t *d_parents, uint32_t *d_weights, unsigned long long *d_count) {
    auto &J = db->join;
    const bool crowned = max_div >= db->L;
    const uint32_t scan_div = crowned ? radius : max_div;
    JoinCall c{db, db->n < 2 || scan_div >= db->L};
    RC_TRY(join_begin(c, d_count, 1, 1));
    if (c.nothing) return SMAFA_OK;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(J.parent.ensure((size_t)n * 3u * sizeof(uint32_t)));
    RC_TRY(J.ctl.ensure(4 * sizeof(unsigned long long)));
    unsigned long long *const best = J.parent.as<unsigned long long>();
    uint32_t *const weight = J.parent.as<uint32_t>() + 2 * (size_t)n;
    RC_TRY(timed_begin(c, &J.count_ms, "peaks: weight[] seeded"));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, 4 * sizeof(unsigned long long), db->stream));
    hipLaunchKernelGGL(smafa_pk::init_peaks_kernel, row_grid(n), dim3(256), 0, db->stream, best, weight, n, 0u, 2u, d_weights_in,
                       J.ctl.as<unsigned long long>() + 1);
    RC_TRY(timed_end(c));
    unsigned long long sum = 0;
    HIP_TRY(hipMemcpyAsync(&sum, J.ctl.as<unsigned long long>() + 1, sizeof sum, hipMemcpyDeviceToHost, db->stream));
    RC_TRY(timed_sync(c));
    if (sum > 0xffffffffull) return set_error(SMAFA_ERR_INVALID, "%s: the weights sum to %llu, a weight holds at most 4294967295", who, sum);
    if (scan_div >= db->L)  // every row within the radius of every other: every weight is the sum
        RC_TRY(timed_pass(c, &J.count_ms, "peaks: weight[] initialised", [&] {
            hipLaunchKernelGGL(smafa_pk::init_peaks_kernel, row_grid(n), dim3(256), 0, db->stream, best, weight, n, (uint32_t)sum, 0u);
        }));
    const auto launch_weigh = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_pk::weigh_keep_kernel, list_grid(p.count), dim3(256), 0,
                           db->stream, p.list, p.count, p.p0, p.S, p.R, p.order, J.pos_of.as<uint32_t>(), weight, radius,
                           J.kept.as<smafa_hit>(), crowned ? 0ull : (unsigned long long)kept_room(db), J.ctl.as<unsigned long long>(),
                           d_weights_in);
    };
    const auto launch_climb = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_pk::climb_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R, p.order,
                           weight, best);
    };
    const char *const weighed = "peaks: a piece's rows weighed", *const climbed = "peaks: a piece's rows climbed";
    JoinConsumer weigh = crowned ? timed_consumer(c, &J.count_ms, weighed, launch_weigh) : keeping_consumer(c, &J.count_ms, weighed, launch_weigh);
    JoinConsumer climb = timed_consumer(c, &J.link_ms, climbed, launch_climb);
    if (!c.no_scans) {
        RC_TRY(join_positions(c));
        RC_TRY(join_pass(c, scan_div, weigh));
    }
    unsigned long long kept_total = 0;
    RC_TRY(read_ctl(c, &kept_total, 1));
    const KeptPlan plan = crowned ? kKeptNothing : kept_plan(db, kept_total, "peaks", "climb");
    RC_TRY(timed_begin(c, &J.link_ms, plan == kKeptOnce ? climbed : weigh.used ? weighed : "peaks: weight[] seeded"));
    if (crowned)
        hipLaunchKernelGGL(smafa_pk::crown_kernel, row_grid(n), dim3(256), 0, db->stream, weight, n, J.ctl.as<unsigned long long>() + 2);
    else
        hipLaunchKernelGGL(smafa_pk::init_peaks_kernel, row_grid(n), dim3(256), 0, db->stream, best, weight, n, 0u, 1u);
    HIP_TRY(hipGetLastError());
    climb.used = plan == kKeptOnce;
    if (climb.used) launch_climb(kept_piece(db, kept_total));
    RC_TRY(timed_end(c, climb.used ? 2u : 1u));
    if (plan == kKeptJoinAgain) RC_TRY(join_pass(c, scan_div, climb));
    RC_TRY(peaks_settle(c, crowned, climb.used, d_labels, d_parents, d_weights, d_count));
    join_finish(c);
    note_call_kernel(db, "smafa_pk::init_peaks_kernel");
    if (weigh.used) note_call_kernel(db, "smafa_pk::weigh_keep_kernel");
    if (climb.used) note_call_kernel(db, "smafa_pk::climb_kernel");
    if (crowned) note_call_kernel(db, "smafa_pk::crown_kernel");
    note_call_kernel(db, "smafa_pk::settle_kernel");
    if (J.jump_rounds) note_call_kernel(db, "smafa_pk::jump_kernel");
    log_line(2, "weighted peaks of %u rows at bound %u, radius %u: %u scans (%u of them repeats) in %u join%s, records %.3f ms, scans %.3f ms, "
             "weigh/keep %.3f ms, climb %.3f ms, settle+jump %.3f ms in %u jump round%s, %llu pairs kept", n, max_div, radius, J.blocks + J.rescans,
             J.rescans, J.joins, J.joins == 1 ? "" : "s", J.rec_ms, J.scan_ms, J.count_ms, J.link_ms, J.flatten_ms, J.jump_rounds,
             J.jump_rounds == 1 ? "" : "s", kept_total);
    return SMAFA_OK;
}

// smafa_db_self_chimeras_launch (chimera.hip.h): d_flags is n flags, d_count one counter, J.parent holds left[] and right[] (8 B
// each per subject) and weight[] (4 B) behind them.  Phase 1 is the peaks call's: the join with smafa_pk::weigh_keep_kernel per
// piece, which raises both weights of every kept pair within the radius and moves every kept pair to J.kept while that has room.
// With d_weights_in the pairs are kept all the same and the caller's weights are copied over the counted ones behind the join.
// The kept total then decides (kept_plan) how chimera::offer_sides_kernel gets the pairs, and chimera::verdict_kernel writes the
// outputs and the count.  max_div >= seq_len: every other row is a candidate parent, and the join runs AT seq_len, as the pairs
// call runs it — it lists every pair, those with no column in common included, which offer length 0 like any other.  Counted
// weights at a radius >= seq_len are all n: no row has a parent and nothing is scanned.
// radius <= max_div; min_fold >= 1; d_weights_in and the five arrays behind d_flags: n entries each, or nullptr
static int join_chimeras(smafa_db *db, uint32_t max_div, uint32_t radius, uint32_t min_fold, const uint32_t *d_weights_in, uint32_t *d_flags,
                         uint32_t *d_left_parent, uint32_t *d_left_len, uint32_t *d_right_parent, uint32_t *d_right_len,
                         uint32_t *d_weights, unsigned long long *d_count) {
    auto &J = db->join;
    const bool all_heavy = !d_weights_in && radius >= db->L;
    const uint32_t scan_div = std::min(max_div, db->L);
    JoinCall c{db, db->n < 2 || all_heavy};
    RC_TRY(join_begin(c, d_count, 1, 1));
    if (c.nothing) return SMAFA_OK;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(J.parent.ensure((size_t)n * 5u * sizeof(uint32_t)));
    RC_TRY(J.ctl.ensure(4 * sizeof(unsigned long long)));
    unsigned long long *const left = J.parent.as<unsigned long long>(), *const right = left + n;
    uint32_t *const weight = J.parent.as<uint32_t>() + 4 * (size_t)n;
    RC_TRY(timed_begin(c, &J.count_ms, "chimeras: weight[] initialised"));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, 4 * sizeof(unsigned long long), db->stream));
    hipLaunchKernelGGL(smafa_pk::init_peaks_kernel, row_grid(n), dim3(256), 0, db->stream, left, weight, n, all_heavy ? n : 1u, 0u);
    RC_TRY(timed_end(c));
    const uint32_t perm_words = 32u * db->W <= chimera::kPermLdsWords ? 32u * db->W : 0u;
    const auto launch_weigh = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_pk::weigh_keep_kernel, list_grid(p.count), dim3(256), 0,
                           db->stream, p.list, p.count, p.p0, p.S, p.R, p.order, J.pos_of.as<uint32_t>(), weight, radius,
                           J.kept.as<smafa_hit>(), (unsigned long long)kept_room(db), J.ctl.as<unsigned long long>());
    };
    const auto launch_offer = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(chimera::offer_sides_kernel, list_grid(p.count), dim3(256), perm_words * sizeof(uint32_t), db->stream, p.list,
                           p.count, p.p0, p.S, p.R, p.order, J.pos_of.as<uint32_t>(), weight, min_fold, db->d_planes, db->P, db->W, db->L,
                           db->d_perm.as<uint32_t>(), perm_words, left, right);
    };
    const char *const weighed = "chimeras: a piece's rows weighed", *const offered = "chimeras: a piece's rows offered";
    JoinConsumer weigh = keeping_consumer(c, &J.count_ms, weighed, launch_weigh);
    JoinConsumer offer = timed_consumer(c, &J.link_ms, offered, launch_offer);
    if (!c.no_scans) {
        RC_TRY(join_positions(c));
        RC_TRY(join_pass(c, scan_div, weigh));
    }
    unsigned long long kept_total = 0;
    RC_TRY(read_ctl(c, &kept_total, 1));
    // every counted weight is final: the caller's weights over them, the empty slots, and the offers over the kept list, if that has
    // every pair, in ONE timed pass
    const KeptPlan plan = kept_plan(db, kept_total, "chimeras", "offer");
    RC_TRY(timed_begin(c, &J.link_ms, plan == kKeptOnce ? offered : "chimeras: left[] and right[] initialised"));
    if (d_weights_in) HIP_TRY(hipMemcpyAsync(weight, d_weights_in, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, db->stream));
    hipLaunchKernelGGL(chimera::init_sides_kernel, row_grid(n), dim3(256), 0, db->stream, left, right, n);
    HIP_TRY(hipGetLastError());
    offer.used = plan == kKeptOnce;
    if (offer.used) launch_offer(kept_piece(db, kept_total));
    RC_TRY(timed_end(c, offer.used ? 2u : 1u));
    if (plan == kKeptJoinAgain) RC_TRY(join_pass(c, scan_div, offer));
    RC_TRY(join_flatten(c, [&] {
        hipLaunchKernelGGL(chimera::verdict_kernel, row_grid(n), dim3(256), 0, db->stream, left, right, weight, n, db->L, d_flags, d_left_parent,
                           d_left_len, d_right_parent, d_right_len, d_weights, d_count);
    }));
    join_finish(c);
    note_call_kernel(db, "smafa_pk::init_peaks_kernel");
    if (weigh.used) note_call_kernel(db, "smafa_pk::weigh_keep_kernel");
    note_call_kernel(db, "chimera::init_sides_kernel");
    if (offer.used) note_call_kernel(db, "chimera::offer_sides_kernel");
    note_call_kernel(db, "chimera::verdict_kernel");
    log_line(2, "chimeras of %u rows at bound %u, radius %u, fold %u%s: %u scans (%u of them repeats) in %u join%s, records %.3f ms, "
             "scans %.3f ms, weigh/keep %.3f ms, offers %.3f ms, verdict %.3f ms, %llu pairs kept", n, max_div, radius, min_fold,
             d_weights_in ? ", weights given" : "", J.blocks + J.rescans, J.rescans, J.joins, J.joins == 1 ? "" : "s", J.rec_ms, J.scan_ms,
             J.count_ms, J.link_ms, J.flatten_ms, kept_total);
    return SMAFA_OK;
}
// ---- the entry list of the neighbours call (neighbours.hip.h): two entries per kept pair, 8 B each — and 4 B more, the rows,
// in a second list behind them where the order takes two sorts (apart)
static uint32_t *entry_rows(const smafa_db *db) { return reinterpret_cast<uint32_t *>(db->join.entries.as<unsigned long long>() + db->join.entries_cap); }

// Room in J.entries for `want` entries; the first `live` are carried over.  Grown as grow_kept grows J.kept — doubling, a bare
// hipMalloc — but a list that cannot grow has no second join to fall back on: the call fails, and the handle stays usable.
static int grow_entries(smafa_db *db, uint64_t want, uint64_t live, bool apart) {
    auto &J = db->join;
    if (want <= J.entries_cap) return SMAFA_OK;
    const size_t each = apart ? 12u : 8u;
    const uint64_t room = std::max<uint64_t>(want, J.entries_cap * 2);
    DevBuf bigger;
    if (hipMalloc(&bigger.p, room * each) != hipSuccess) {
        (void)hipGetLastError();
        return set_error(SMAFA_ERR_NOMEM, "neighbours: no memory for a list of %llu entries (%llu bytes)", (unsigned long long)room,
                         (unsigned long long)(room * each));
    }
    bigger.cap = room * each;
    hipError_t e = hipSuccess;
    if (live) e = hipMemcpyAsync(bigger.p, J.entries.p, live * 8u, hipMemcpyDeviceToDevice, db->stream);
    if (live && apart && e == hipSuccess)
        e = hipMemcpyAsync(bigger.as<unsigned long long>() + room, entry_rows(db), live * 4u, hipMemcpyDeviceToDevice, db->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) {
        bigger.release();
        return set_error(SMAFA_ERR_DEVICE, "neighbours: moving the entry list failed: %s", hipGetErrorString(e));
    }
    J.entries.release();
    J.entries = bigger;
    J.entries_cap = room;
    J.growths++;
    return SMAFA_OK;
}

constexpr unsigned long long kSortItemsMax = 0x7fffffffull;  // the device radix sort counts its items in an int

// smafa_db_self_neighbours_launch (neighbours.hip.h): d_offsets is n + 1 offsets, d_neighbours and d_dists (or nullptr) cap
// entries each, d_total one counter.  The join runs at min(max_div, seq_len) — also where no two rows can exceed the bound: the
// distances still differ — with mirror_pack_kernel per piece (the exactly-once rule, so pos_of[]), which appends both directions
// of every kept pair to J.entries; in front of every piece's pass the list gets room for two entries per row of the piece's
// list on top of the total read back in front of the piece's wait.  Behind the join: the sort (neighbour_key_rule: one sort of
// the entries as keys, or two stable sorts with the rows apart), row_bounds_kernel, with a cut cut_degrees_kernel and an
// exclusive sum, the total — with a cut read back, the one wait the cut costs — and, where it fits cap, emit_kernel.  No entry
// at all: the offsets are zeroed and nothing else runs.
// k: SMAFA_NONE = no cut
static int join_neighbours(smafa_db *db, uint32_t max_div, uint32_t k, unsigned long long *d_offsets, uint32_t *d_neighbours,
                           uint32_t *d_dists, uint64_t cap, unsigned long long *d_total) {
    auto &J = db->join;
    JoinCall c{db};
    RC_TRY(join_begin(c, d_total, 1, 2));
    const size_t offsets_bytes = (size_t)(db->n + 1) * sizeof(unsigned long long);
    if (c.nothing) {  // no row, or one: {0}, or {0, 0}
        HIP_TRY(hipMemsetAsync(d_offsets, 0, offsets_bytes, db->stream));
        return SMAFA_OK;
    }
    const uint32_t n = (uint32_t)db->n, scan_div = std::min(max_div, db->L);
    const bool cut = k != SMAFA_NONE;
    NeighbourKey key = neighbour_key_rule(n, max_div, db->L);
    if (db->neighbour_two_sorts) key.sorts = 2u;
    const bool apart = key.sorts == 2u;
    const uint32_t shift = apart ? 0u : 32u + key.dist_bits;
    const dim3 bounds_grid((uint32_t)(((uint64_t)n + 256u) / 256u));  // n + 1 threads
    // The buffer is kept across calls, its division is not: a call with the rows apart places them behind entries_cap 8-byte
    // entries, so a buffer that an earlier call filled at 8 B per entry serves this one at cap / 12 entries, and the other way round.
    J.entries_cap = J.entries.cap / (apart ? 12u : 8u);
    J.growths = 0;
    RC_TRY(J.ctl.ensure(2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, 2 * sizeof(unsigned long long), db->stream));
    RC_TRY(join_positions(c));
    JoinConsumer pack = timed_consumer(c, &J.filter_ms, "neighbours: a piece's rows mirrored and packed", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_nb::mirror_pack_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R,
                           p.order, J.pos_of.as<uint32_t>(), shift, J.entries.as<unsigned long long>(), apart ? entry_rows(db) : (uint32_t *)nullptr,
                           (unsigned long long)J.entries_cap, J.ctl.as<unsigned long long>());
    });
    const auto too_many = [](unsigned long long entries) {
        return set_error(SMAFA_ERR_NOMEM, "neighbours: %llu entries before the cut, the device sort orders at most %llu", entries, kSortItemsMax);
    };
    pack = watching(c, pack, [&](unsigned long long seen, const JoinPiece &p) {
        if (seen > kSortItemsMax) return too_many(seen);  // (exact so far, and it only grows)
        return grow_entries(db, seen + 2 * p.count, seen, apart);
    });
    RC_TRY(join_pass(c, scan_div, pack));
    unsigned long long entries = 0, total = 0;
    RC_TRY(read_ctl(c, &entries, 1));
    if (entries > kSortItemsMax) return too_many(entries);
    const unsigned long long *sorted = nullptr, *lower = d_offsets;
    const uint32_t *rows = nullptr;
    if (entries) {
        // ---- the order
        const int count = (int)entries, low_bits = (int)(32u + key.dist_bits), row_bits = (int)key.row_bits;
        unsigned long long *const list = J.entries.as<unsigned long long>();
        RC_TRY(db->keys_a.ensure(entries * sizeof(unsigned long long)));
        unsigned long long *const ka = db->keys_a.as<unsigned long long>();
        size_t tmp_bytes = 0, tmp_second = 0;
        if (!apart) {
            HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, list, ka, count, 0, low_bits + row_bits, db->stream));
            RC_TRY(db->sort_tmp.ensure(tmp_bytes));
            RC_TRY(timed_begin(c, &J.count_ms, "neighbours: entries sorted as keys"));
            HIP_TRY(hipcub::DeviceRadixSort::SortKeys(db->sort_tmp.p, tmp_bytes, list, ka, count, 0, low_bits + row_bits, db->stream));
            sorted = ka;
        } else {
            RC_TRY(db->keys_b.ensure(entries * sizeof(unsigned long long)));
            RC_TRY(db->idx_a.ensure(entries * sizeof(uint32_t)));
            RC_TRY(db->idx_b.ensure(entries * sizeof(uint32_t)));
            unsigned long long *const kb = db->keys_b.as<unsigned long long>();
            uint32_t *const ra = db->idx_a.as<uint32_t>(), *const rb = db->idx_b.as<uint32_t>();
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, list, ka, entry_rows(db), ra, count, 0, low_bits, db->stream));
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_second, ra, rb, ka, kb, count, 0, row_bits, db->stream));
            tmp_bytes = std::max(tmp_bytes, tmp_second);
            RC_TRY(db->sort_tmp.ensure(tmp_bytes));
            RC_TRY(timed_begin(c, &J.count_ms, "neighbours: entries sorted by (dist, neighbour), then by row"));
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, tmp_bytes, list, ka, entry_rows(db), ra, count, 0, low_bits, db->stream));
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, tmp_bytes, ra, rb, ka, kb, count, 0, row_bits, db->stream));
            sorted = kb, rows = rb;
        }
        RC_TRY(timed_end(c, key.sorts));
        RC_TRY(timed_sync(c));
        // ---- where the rows begin, the cut, the total
        if (cut) {
            RC_TRY(J.parent.ensure(((size_t)n + 1u) * 2u * sizeof(unsigned long long)));
            unsigned long long *const lo = J.parent.as<unsigned long long>(), *const deg = lo + ((size_t)n + 1u);
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, deg, d_offsets, (uint64_t)n + 1u, db->stream));
            RC_TRY(db->sort_tmp.ensure(tmp_bytes));
            RC_TRY(timed_begin(c, &J.link_ms, "neighbours: rows bounded, degrees cut and summed"));
            hipLaunchKernelGGL(smafa_nb::row_bounds_kernel, bounds_grid, dim3(256), 0, db->stream, sorted, rows, shift, entries, n, lo);
            hipLaunchKernelGGL(smafa_nb::cut_degrees_kernel, bounds_grid, dim3(256), 0, db->stream, lo, n, k, deg);
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(db->sort_tmp.p, tmp_bytes, deg, d_offsets, (uint64_t)n + 1u, db->stream));
            lower = lo;
        } else {
            RC_TRY(timed_begin(c, &J.link_ms, "neighbours: rows bounded"));
            hipLaunchKernelGGL(smafa_nb::row_bounds_kernel, bounds_grid, dim3(256), 0, db->stream, sorted, rows, shift, entries, n, d_offsets);
        }
        HIP_TRY(hipMemcpyAsync(d_total, d_offsets + n, sizeof total, hipMemcpyDeviceToDevice, db->stream));
        RC_TRY(timed_end(c, cut ? 3u : 1u));
        total = entries;
        if (cut) HIP_TRY(hipMemcpyAsync(&total, d_offsets + n, sizeof total, hipMemcpyDeviceToHost, db->stream));
        RC_TRY(timed_sync(c));
    } else {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, offsets_bytes, db->stream));
    }
    const bool fits = total <= cap;
    if (entries && fits) {
        RC_TRY(timed_pass(c, &J.flatten_ms, "neighbours: entries emitted", [&] {
            hipLaunchKernelGGL(smafa_nb::emit_kernel, list_grid(entries), dim3(256), 0, db->stream, sorted, rows, shift, entries, lower,
                               d_offsets, k, (unsigned long long)cap, d_neighbours, d_dists);
        }));
        RC_TRY(timed_sync(c));
    }
    join_finish(c);
    if (pack.used) note_call_kernel(db, "smafa_nb::mirror_pack_kernel");
    if (entries) note_call_kernel(db, "smafa_nb::row_bounds_kernel");
    if (entries && cut) note_call_kernel(db, "smafa_nb::cut_degrees_kernel");
    if (entries && fits) note_call_kernel(db, "smafa_nb::emit_kernel");
    log_line(2, "neighbours of %u rows at bound %u, cut %s: %u scans (%u of them repeats), records %.3f ms, scans %.3f ms, pack %.3f ms, "
             "sort %.3f ms (%u sort%s), bounds %.3f ms, emit %.3f ms, %llu entries, %llu listed, %u growths", n, max_div, cut ? std::to_string(k).c_str() : "none",
             J.blocks + J.rescans, J.rescans, J.rec_ms, J.scan_ms, J.filter_ms, J.count_ms, entries ? key.sorts : 0u,
             entries && key.sorts == 1u ? "" : "s", J.link_ms, J.flatten_ms, entries, total, J.growths);
    if (!fits)
        return set_error(SMAFA_ERR_CAPACITY, "neighbour lists too small: %llu entries needed, capacity %llu", total, (unsigned long long)cap);
    return SMAFA_OK;
}

// The span phase of the two forests (`who`: "forest" or "reach", for the texts): the weight classes 0 .. E - 1 one after another,
// a kernel boundary between two classes.  only_dist is the caller's, the class that launch_span and `span` (the consumer made of
// it) handle.  kKeptOnce: E launches over the kept list in one timed pass; kKeptJoinAgain: the store joined once more PER CLASS,
// at bound t with the raw piece lists spanned at only_dist = t (every pair of class t is within t).  Behind class t the running
// edge total is copied into level_ends[t] on the stream — behind the class's last launch, in front of the next class's first.
// A wait ends the phase.
template <class Launch>
static int span_classes(JoinCall &c, const char *who, uint32_t E, unsigned long long kept_total, KeptPlan plan, JoinConsumer &span,
                        Launch launch_span, uint32_t &only_dist, unsigned long long *d_level_ends, const unsigned long long *n_edges) {
    smafa_db *db = c.db;
    const auto end_class = [&] {
        HIP_TRY(hipMemcpyAsync(d_level_ends + only_dist, n_edges, sizeof(unsigned long long), hipMemcpyDeviceToDevice, db->stream));
        return SMAFA_OK;
    };
    char what[64];  // (read by the wait below, which forgets it)
    snprintf(what, sizeof what, "%s: the kept list spanned, class by class", who);
    if (plan == kKeptOnce) {
        RC_TRY(timed_begin(c, &db->join.link_ms, what));
        for (only_dist = 0; only_dist < E; only_dist++) {
            launch_span(kept_piece(db, kept_total));
            RC_TRY(end_class());
        }
        RC_TRY(timed_end(c, E));
        span.used = true;
    } else if (plan == kKeptJoinAgain) {
        log_line(2, "%s: %llu pairs, the kept list holds %llu: the store is joined once more per class, at the bounds 0 .. %u", who,
                 kept_total, (unsigned long long)kept_room(db), E - 1u);
        for (only_dist = 0; only_dist < E; only_dist++) {
            RC_TRY(join_pass(c, only_dist, span));
            RC_TRY(end_class());
        }
    }
    return timed_sync(c);
}

// Bounds no two rows can exceed, behind the last class: star_roots_kernel hangs every surviving root under row 0 and fills
// level_ends[L ..], waited for.
static int star_roots(JoinCall &c, const char *what, const uint32_t *parent, smafa_hit *d_edges, unsigned long long *n_edges,
                      unsigned long long *d_level_ends, uint32_t n_levels) {
    smafa_db *db = c.db;
    const uint32_t n = (uint32_t)db->n;
    RC_TRY(timed_pass(c, &db->join.flatten_ms, what, [&] {
        hipLaunchKernelGGL(smafa_sf::star_roots_kernel, row_grid(n), dim3(256), 0, db->stream, parent, n, db->L, d_edges,
                           (unsigned long long)(n - 1u), n_edges, d_level_ends, n_levels);
    }));
    return timed_sync(c);
}

// smafa_db_self_forest_launch (forest.hip.h): d_edges is n - 1 rows, d_level_ends max_div + 1 counters, J.parent one union-find,
// J.ctl the kept total and the running edge total.  The join runs ONCE at bound E - 1 (E = min(max_div, L - 1) + 1 scanned
// classes, as join_levels) with keep_pairs_kernel per piece (the exactly-once rule, so pos_of[]), which only moves the kept
// pairs to J.kept; the kept total then decides (kept_plan) how span_edges_kernel gets them: E launches over the kept list, one
// per weight class — Kruskal by class, a kernel boundary between two classes — or, where the list could not hold every
// pair, the store joined once more PER CLASS, at bound t with the raw piece lists spanned at only_dist = t (the slow path: the
// sum of the joins at 0 .. E - 1).  Behind class t the running edge total is copied into level_ends[t] on the stream.
// max_div >= L: star_roots_kernel hangs every surviving root under row 0 and fills level_ends[L ..].
static int join_forest(smafa_db *db, uint32_t max_div, smafa_hit *d_edges, unsigned long long *d_level_ends) {
    auto &J = db->join;
    const uint32_t n_levels = max_div + 1u, E = std::min(n_levels, std::max<uint32_t>(db->L, 1u)), scan_div = E - 1u;
    const bool all_near = max_div >= db->L;
    JoinCall c{db};
    RC_TRY(join_begin(c, d_level_ends, n_levels, 2));
    if (c.nothing) return SMAFA_OK;  // no row, or one: no edge, every level ends at 0
    const uint32_t n = (uint32_t)db->n;
    const unsigned long long room = n - 1u;
    RC_TRY(J.parent.ensure((size_t)n * sizeof(uint32_t)));
    RC_TRY(J.ctl.ensure(2 * sizeof(unsigned long long)));
    uint32_t *const parent = J.parent.as<uint32_t>();
    unsigned long long *const n_edges = J.ctl.as<unsigned long long>() + 1;
    RC_TRY(timed_begin(c, &J.link_ms, "forest: parent[] initialised"));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, 2 * sizeof(unsigned long long), db->stream));
    hipLaunchKernelGGL(smafa_sf::init_forest_kernel, row_grid(n), dim3(256), 0, db->stream, parent, n);
    RC_TRY(timed_end(c));
    RC_TRY(join_positions(c));
    JoinConsumer keep = keeping_consumer(c, &J.count_ms, "forest: parent[] untouched, a piece's rows kept", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_sf::keep_pairs_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R,
                           p.order, J.pos_of.as<uint32_t>(), J.kept.as<smafa_hit>(), (unsigned long long)kept_room(db),
                           J.ctl.as<unsigned long long>());
    });
    uint32_t only_dist = 0;  // the class the span launches handle
    const auto launch_span = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_sf::span_edges_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R,
                           p.order, parent, only_dist, d_edges, room, n_edges);
    };
    JoinConsumer span = timed_consumer(c, &J.link_ms, "forest: a class of a piece's rows spanned", launch_span);
    RC_TRY(join_pass(c, scan_div, keep));
    unsigned long long kept_total = 0;
    RC_TRY(read_ctl(c, &kept_total, 1));
    RC_TRY(span_classes(c, "forest", E, kept_total, kept_plan(db, kept_total, "forest", "span"), span, launch_span, only_dist, d_level_ends,
                        n_edges));
    if (all_near) RC_TRY(star_roots(c, "forest: the surviving roots hung under row 0", parent, d_edges, n_edges, d_level_ends, n_levels));
    join_finish(c);
    note_call_kernel(db, "smafa_sf::init_forest_kernel");
    if (keep.used) note_call_kernel(db, "smafa_sf::keep_pairs_kernel");
    if (span.used) note_call_kernel(db, "smafa_sf::span_edges_kernel");
    if (all_near) note_call_kernel(db, "smafa_sf::star_roots_kernel");
    log_line(2, "forest of %u rows up to bound %u, joined at bound %u: %u scans (%u of them repeats) in %u join%s, records %.3f ms, "
             "scans %.3f ms, keep %.3f ms, span %.3f ms, star %.3f ms, %llu pairs kept", n, max_div, scan_div, J.blocks + J.rescans, J.rescans,
             J.joins, J.joins == 1 ? "" : "s", J.rec_ms, J.scan_ms, J.count_ms, J.link_ms, J.flatten_ms, kept_total);
    return SMAFA_OK;
}

// smafa_db_self_reach_forest_launch (reach.hip.h): join_forest with an edge's weight max(dist, core[a], core[b]).  d_edges is n - 1
// rows, d_level_ends max_div + 1 counters, d_cores n entries or nullptr; J.parent one union-find and core[] behind it, J.hist the
// tallies (E per subject, zeroed here), J.ctl the kept total, the rows that are not sparse and the running edge total.  The join
// runs ONCE at bound E - 1 with tally_keep_kernel per piece (the exactly-once rule, so pos_of[]): the kept pairs move to J.kept
// and are tallied per end and distance.  core_dist_kernel then makes core[] of the tallies; fewer than two rows that are not
// sparse: no edge.  Else the kept total decides (kept_plan) how span_reach_kernel gets the pairs: E launches over the kept list,
// one per weight class, or the store joined once more per class at bound t with the raw piece lists spanned at only_dist = t (every
// pair of weight t is within t).  max_div >= L and n >= min_pts: a row still sparse behind class L - 1 has core exactly L, and
// star_roots_kernel hangs every surviving root under row 0 at weight L.  One path for every min_pts >= 1.
// The call is reach_passes between join_begin and join_finish, and reach_notes: join_stable runs the same passes in front of its own.
struct ReachRun {
    uint32_t scan_div = 0;
    bool all_near = false, tallied = false, spanned = false;
    unsigned long long kept_total = 0, dense = 0;
};

// n >= 2, behind join_begin
static int reach_passes(JoinCall &c, uint32_t max_div, uint32_t min_pts, smafa_hit *d_edges, unsigned long long *d_level_ends,
                        uint32_t *d_cores, ReachRun &run) {
    smafa_db *db = c.db;
    auto &J = db->join;
    const uint32_t n_levels = max_div + 1u, E = std::min(n_levels, std::max<uint32_t>(db->L, 1u)), scan_div = E - 1u;
    const bool all_near = max_div >= db->L && db->n >= min_pts;
    const uint32_t n = (uint32_t)db->n;
    const unsigned long long room = n - 1u;
    RC_TRY(J.parent.ensure((size_t)n * 2u * sizeof(uint32_t)));
    RC_TRY(J.hist.ensure((size_t)n * E * sizeof(uint32_t)));
    RC_TRY(J.ctl.ensure(3 * sizeof(unsigned long long)));
    uint32_t *const parent = J.parent.as<uint32_t>(), *const core = parent + n, *const hist = J.hist.as<uint32_t>();
    unsigned long long *const n_dense = J.ctl.as<unsigned long long>() + 1, *const n_edges = n_dense + 1;
    RC_TRY(timed_begin(c, &J.link_ms, "reach: parent[] initialised, the tallies zeroed"));
    HIP_TRY(hipMemsetAsync(J.ctl.p, 0, 3 * sizeof(unsigned long long), db->stream));
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)n * E * sizeof(uint32_t), db->stream));
    hipLaunchKernelGGL(smafa_sf::init_forest_kernel, row_grid(n), dim3(256), 0, db->stream, parent, n);
    RC_TRY(timed_end(c));
    RC_TRY(join_positions(c));
    JoinConsumer tally = keeping_consumer(c, &J.count_ms, "reach: parent[] untouched, a piece's rows tallied and kept", [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_mr::tally_keep_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R,
                           p.order, J.pos_of.as<uint32_t>(), J.kept.as<smafa_hit>(), (unsigned long long)kept_room(db),
                           J.ctl.as<unsigned long long>(), hist, E);
    });
    uint32_t only_dist = 0;  // the class the span launches handle
    const auto launch_span = [&](const JoinPiece &p) {
        hipLaunchKernelGGL(smafa_mr::span_reach_kernel, list_grid(p.count), dim3(256), 0, db->stream, p.list, p.count, p.p0, p.S, p.R,
                           p.order, core, parent, only_dist, d_edges, room, n_edges);
    };
    JoinConsumer span = timed_consumer(c, &J.link_ms, "reach: a class of a piece's rows spanned", launch_span);
    RC_TRY(join_pass(c, scan_div, tally));
    RC_TRY(timed_pass(c, &J.filter_ms, "reach: the core distances", [&] {
        hipLaunchKernelGGL(smafa_mr::core_dist_kernel, row_grid(n), dim3(256), 0, db->stream, hist, n, E, min_pts,
                           all_near ? db->L : SMAFA_NONE, core, d_cores, n_dense);
    }));
    unsigned long long totals[2] = {0, 0};  // every tally is final: the kept total; the rows that are not sparse
    RC_TRY(read_ctl(c, totals, 2));
    const unsigned long long kept_total = totals[0];
    // (fewer than two rows that are not sparse: no pair has a weight)
    const KeptPlan plan = totals[1] < 2 ? kKeptNothing : kept_plan(db, kept_total, "reach", "span");
    RC_TRY(span_classes(c, "reach", E, kept_total, plan, span, launch_span, only_dist, d_level_ends, n_edges));
    if (all_near) RC_TRY(star_roots(c, "reach: the surviving roots hung under row 0", parent, d_edges, n_edges, d_level_ends, n_levels));
    run = {scan_div, all_near, tally.used, span.used, kept_total, totals[1]};
    return SMAFA_OK;
}

// behind join_finish: the kernels of the reach forest's passes, in launch order
static void reach_notes(const smafa_db *db, const ReachRun &run) {
    note_call_kernel(db, "smafa_sf::init_forest_kernel");
    if (run.tallied) note_call_kernel(db, "smafa_mr::tally_keep_kernel");
    note_call_kernel(db, "smafa_mr::core_dist_kernel");
    if (run.spanned) note_call_kernel(db, "smafa_mr::span_reach_kernel");
    if (run.all_near) note_call_kernel(db, "smafa_sf::star_roots_kernel");
}

static int join_reach_forest(smafa_db *db, uint32_t max_div, uint32_t min_pts, smafa_hit *d_edges, unsigned long long *d_level_ends,
                             uint32_t *d_cores) {
    auto &J = db->join;
    JoinCall c{db};
    RC_TRY(join_begin(c, d_level_ends, (size_t)max_div + 1u, 2));
    if (c.nothing) {  // no row, or one: no edge, every level ends at 0; the one row is core at 0 where it alone is enough
        if (d_cores && db->n) HIP_TRY(hipMemsetAsync(d_cores, min_pts <= 1u ? 0 : 0xff, db->n * sizeof(uint32_t), db->stream));
        return SMAFA_OK;
    }
    ReachRun run;
    RC_TRY(reach_passes(c, max_div, min_pts, d_edges, d_level_ends, d_cores, run));
    join_finish(c);
    reach_notes(db, run);
    log_line(2, "reach forest of %u rows up to bound %u at min_pts %u, joined at bound %u: %u scans (%u of them repeats) in %u join%s, "
             "records %.3f ms, scans %.3f ms, tally %.3f ms, cores %.3f ms, span %.3f ms, star %.3f ms, %llu pairs kept, %llu rows not sparse",
             (uint32_t)db->n, max_div, min_pts, run.scan_div, J.blocks + J.rescans, J.rescans, J.joins, J.joins == 1 ? "" : "s", J.rec_ms,
             J.scan_ms, J.count_ms, J.filter_ms, J.link_ms, J.flatten_ms, run.kept_total, run.dense);
    return SMAFA_OK;
}

// smafa_db_self_stable_launch (stable.hip.h): the reach forest's passes into the handle's own buffers, then HDBSCAN's selection over
// its edges and cores, plane by plane.  J.stable holds, in this order: the forest's level ends (max_div + 1 counters) and the
// chosen total; two halves {run[], sum[] (8 B per subject each), size[] (4 B)} for the plane in hand and the one below; kids[];
// the root planes and the flag planes (4 B per subject and plane each); the forest's edges (n - 1 rows).  The planes are
// min(max_div, L) + 1: the scanned classes and, where max_div >= L, the class L that star_roots_kernel fills, which counts
// max_div - L + 1 times in a stability — nothing is allocated or launched per level above L.  parent[] is made fresh once and the
// classes are united one after another, four launches a plane (three for plane 0: nothing lies below it), then excess_kernel, one
// choose_kernel per plane from the last one down and assign_kernel: 5 x planes + 2 launches whatever the store holds, no host
// loop over rows, edges or clusters, and one wait at the end, for the chosen total — the only value of this stage that crosses to the host.
// min_pts >= 1, min_size >= 1; d_joined, d_cores: n entries each, or nullptr; n_clusters: the caller's, on the host
static int join_stable(smafa_db *db, uint32_t max_div, uint32_t min_pts, uint32_t min_size, uint32_t *d_labels, uint32_t *d_joined,
                       uint32_t *d_cores, uint64_t *n_clusters) {
    auto &J = db->join;
    const uint32_t n = (uint32_t)db->n, L = std::max<uint32_t>(db->L, 1u), planes = std::min(max_div, L) + 1u;
    const unsigned long long mult = max_div >= L ? (unsigned long long)(max_div - L) + 1ull : 1ull;  // of the last plane
    const size_t n_levels = (size_t)max_div + 1u, room = n ? n - 1u : 0u;
    const size_t half = (size_t)n * 16u + ((size_t)n * 4u + 7u) / 8u * 8u, plane = (size_t)n * sizeof(uint32_t);
    RC_TRY(use_device(db));
    RC_TRY(J.stable.ensure((n_levels + 1u) * 8u + 2u * half + plane + 2u * planes * plane + room * sizeof(smafa_hit)));
    unsigned long long *const level_ends = J.stable.as<unsigned long long>(), *const chosen = level_ends + n_levels;
    char *const halves = reinterpret_cast<char *>(chosen + 1);
    uint32_t *const kids = reinterpret_cast<uint32_t *>(halves + 2u * half), *const root = kids + n, *const flag = root + (size_t)planes * n;
    smafa_hit *const edges = reinterpret_cast<smafa_hit *>(flag + (size_t)planes * n);
    const auto run_of = [&](uint32_t t) { return reinterpret_cast<unsigned long long *>(halves + (t & 1u) * half); };
    const auto size_of = [&](uint32_t t) { return reinterpret_cast<uint32_t *>(run_of(t) + 2u * (size_t)n); };
    JoinCall c{db};
    RC_TRY(join_begin(c, level_ends, n_levels, 2));
    if (c.nothing) {  // no row: nothing; one row: a cluster of its own where it alone is enough, noise elsewhere; cores as the reach forest's
        const bool one = n == 1u && min_pts <= 1u && min_size <= 1u;
        if (n) HIP_TRY(hipMemsetAsync(d_labels, one ? 0 : 0xff, sizeof(uint32_t), db->stream));
        if (n && d_joined) HIP_TRY(hipMemsetAsync(d_joined, one ? 0 : 0xff, sizeof(uint32_t), db->stream));
        if (n && d_cores) HIP_TRY(hipMemsetAsync(d_cores, min_pts <= 1u ? 0 : 0xff, sizeof(uint32_t), db->stream));
        *n_clusters = one ? 1u : 0u;
        return SMAFA_OK;
    }
    ReachRun run;
    RC_TRY(reach_passes(c, max_div, min_pts, edges, level_ends, d_cores, run));
    // (as reach_passes left them: the union-find, to be made fresh; core[] behind it; the running edge total, final)
    uint32_t *const parent = J.parent.as<uint32_t>(), *const core = parent + n;
    const unsigned long long *const n_edges = J.ctl.as<unsigned long long>() + 2;
    const dim3 rows = row_grid(n), block(256);
    RC_TRY(timed_begin(c, &J.select_ms, "stable: the forest's classes united, counted and chosen from"));
    HIP_TRY(hipMemsetAsync(chosen, 0, sizeof(unsigned long long), db->stream));
    hipLaunchKernelGGL(smafa_sf::init_forest_kernel, rows, block, 0, db->stream, parent, n);
    for (uint32_t t = 0; t < planes; t++) {
        unsigned long long *const run_t = run_of(t), *const sum_t = run_t + n, *const run_b = run_of(t + 1u), *const sum_b = run_b + n;
        uint32_t *const size_t_ = size_of(t), *const size_b = size_of(t + 1u), *const root_t = root + (size_t)t * n;
        uint32_t *const flag_t = flag + (size_t)t * n;
        HIP_TRY(hipMemsetAsync(sum_t, 0, half - (size_t)n * 8u, db->stream));  // sum[] and size[] of this half
        hipLaunchKernelGGL(smafa_st::unite_class_kernel, rows, block, 0, db->stream, edges, n_edges, (unsigned long long)room, n, t, parent);
        hipLaunchKernelGGL(smafa_st::snapshot_kernel, rows, block, 0, db->stream, parent, core, n, t, root_t, size_t_, kids);
        if (t) hipLaunchKernelGGL(smafa_st::census_kernel, rows, block, 0, db->stream, size_b, root_t, n, min_size, kids);
        hipLaunchKernelGGL(smafa_st::adopt_kernel, rows, block, 0, db->stream, root_t, size_t_, size_b, kids, n, min_size,
                           t + 1u == planes ? mult : 1ull, t ? 1u : 0u, run_b, sum_b, run_t, sum_t, t ? flag_t - n : flag_t, flag_t);
    }
    hipLaunchKernelGGL(smafa_st::excess_kernel, rows, block, 0, db->stream, run_of(planes - 1u), run_of(planes - 1u) + n, n,
                       flag + (size_t)(planes - 1u) * n);
    for (uint32_t t = planes; t-- > 0;) {
        const bool last = t + 1u == planes;
        hipLaunchKernelGGL(smafa_st::choose_kernel, rows, block, 0, db->stream, last ? (const uint32_t *)nullptr : root + (size_t)(t + 1u) * n,
                           last ? (const uint32_t *)nullptr : flag + (size_t)(t + 1u) * n, n, flag + (size_t)t * n, chosen);
    }
    hipLaunchKernelGGL(smafa_st::assign_kernel, rows, block, 0, db->stream, root, flag, core, n, planes, d_labels, d_joined);
    RC_TRY(timed_end(c, 5u * planes + 2u));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, chosen, sizeof total, hipMemcpyDeviceToHost, db->stream));
    RC_TRY(timed_sync(c));
    *n_clusters = total;
    join_finish(c);
    reach_notes(db, run);
    note_call_kernel(db, "smafa_st::unite_class_kernel");
    note_call_kernel(db, "smafa_st::snapshot_kernel");
    if (planes > 1u) note_call_kernel(db, "smafa_st::census_kernel");
    note_call_kernel(db, "smafa_st::adopt_kernel");
    note_call_kernel(db, "smafa_st::excess_kernel");
    note_call_kernel(db, "smafa_st::choose_kernel");
    note_call_kernel(db, "smafa_st::assign_kernel");
    log_line(2, "stable clusters of %u rows up to bound %u at min_pts %u, min_cluster_size %u, joined at bound %u: %u scans (%u of them "
             "repeats) in %u join%s, records %.3f ms, scans %.3f ms, tally %.3f ms, cores %.3f ms, span %.3f ms, star %.3f ms, select %.3f ms "
             "over %u planes, %llu pairs kept, %llu rows not sparse, %llu clusters", n, max_div, min_pts, min_size, run.scan_div,
             J.blocks + J.rescans, J.rescans, J.joins, J.joins == 1 ? "" : "s", J.rec_ms, J.scan_ms, J.count_ms, J.filter_ms, J.link_ms,
             J.flatten_ms, J.select_ms, planes, run.kept_total, run.dense, total);
    return SMAFA_OK;
}

// ---- consensus (consensus.hip.h).  Not a consumer of the join: the call reads labels the caller holds and the store's own planes.
// It shares the join's call frame (join_begin / timed passes / join_finish, so that smafa_last_call_* and smafa_last_scan_ms report
// it) and scans nothing.  Two phases with ONE host read between them: the bad-row word and K gate everything that writes to the
// caller's arrays.  J.parent holds the bad-row word, mark[] and dense[] (8 B per subject); the sort's double buffers are the handle's
// keys_a / keys_b / idx_a / idx_b (16 B per position) and the shared sort_tmp; J.cons holds seg_begin[] and the slots (12 B per
// group), the records (4 x P x W B per group) and one table per window of consensus_chunk sorted entries — never K x L x alphabet
// counters.  pos_of[], the kept list and the index are not touched.
// who: the entry point, for the texts; d_nearest, d_div: or nullptr; n_clusters: the caller's, on the host
static int join_consensus(smafa_db *db, const char *who, const uint32_t *d_labels, uint32_t *d_ids, uint32_t *d_sizes, uint8_t *d_codes,
                          uint32_t *d_nearest, uint32_t *d_div, uint64_t cap, uint64_t *n_clusters) {
    auto &J = db->join;
    const uint64_t n_pos64 = (db->n + kWaveTile - 1) / kWaveTile * kWaveTile;
    if (n_pos64 >= (1ull << 31))  // (the device radix sort counts its items in an int)
        return set_error(SMAFA_ERR_INVALID, "%s: the consensus takes stores of fewer than 2^31 positions (this one: %llu)", who,
                         (unsigned long long)n_pos64);
    const uint32_t n = (uint32_t)db->n, n_pos = (uint32_t)n_pos64, P = db->P, W = db->W, L = db->L;
    RC_TRY(use_device(db));
    RC_TRY(J.parent.ensure(8u + 2u * ((size_t)n + 1u) * sizeof(uint32_t)));
    uint32_t *const bad = J.parent.as<uint32_t>(), *const mark = bad + 2, *const dense = mark + n + 1u;
    JoinCall c{db, true};
    RC_TRY(join_begin(c, J.parent.as<unsigned long long>(), 1, 1));
    if (c.nothing) {  // an empty store: no cluster, nothing else written
        *n_clusters = 0;
        return SMAFA_OK;
    }
    const dim3 rows = row_grid(n), block(256);
    // ---- groups: which values occur, their dense numbers, K — and the smallest row with an illegal label
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, mark, dense, n + 1u, db->stream));
    RC_TRY(db->sort_tmp.ensure(tmp_bytes));
    RC_TRY(timed_begin(c, &J.count_ms, "consensus: groups marked and numbered"));
    HIP_TRY(hipMemsetAsync(bad, 0xff, sizeof(uint32_t), db->stream));
    HIP_TRY(hipMemsetAsync(mark, 0, ((size_t)n + 1u) * sizeof(uint32_t), db->stream));
    hipLaunchKernelGGL(consensus::mark_groups_kernel, rows, block, 0, db->stream, d_labels, n, mark, bad);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(db->sort_tmp.p, tmp_bytes, mark, dense, n + 1u, db->stream));
    RC_TRY(timed_end(c, 2));
    uint32_t bad_row = SMAFA_NONE, K = 0;
    HIP_TRY(hipMemcpyAsync(&bad_row, bad, sizeof bad_row, hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(hipMemcpyAsync(&K, dense + n, sizeof K, hipMemcpyDeviceToHost, db->stream));
    RC_TRY(timed_sync(c));
    join_finish(c);
    note_call_kernel(db, "consensus::mark_groups_kernel");
    if (bad_row != SMAFA_NONE) {
        uint32_t value = 0;
        HIP_TRY(hipMemcpyAsync(&value, d_labels + bad_row, sizeof value, hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        return set_error(SMAFA_ERR_INVALID, "%s: labels[%u] is %u, neither SMAFA_NONE nor the number of one of the store's %u subjects", who,
                         bad_row, value, n);
    }
    *n_clusters = K;
    if (K > cap)
        return set_error(SMAFA_ERR_CAPACITY, "%s: cluster arrays too small: %u clusters, capacity %llu", who, K, (unsigned long long)cap);
    if (K == 0) {  // every row unlabelled
        if (d_div) HIP_TRY(hipMemsetAsync(d_div, 0xff, (size_t)n * sizeof(uint32_t), db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        return SMAFA_OK;
    }
    // ---- the rest, enqueued at once and waited for once
    const uint32_t chunk = (uint32_t)db->consensus_chunk, n_windows = (uint32_t)(((uint64_t)n + chunk - 1u) / chunk);
    const size_t table_words = (size_t)consensus::kCodes * 32u * W, rec_words = (size_t)P * W;
    const size_t slots_at = 0, seg_at = slots_at + (size_t)K * 8u, recs_at = (seg_at + ((size_t)K + 1u) * 4u + 7u) / 8u * 8u;
    const size_t tables_at = recs_at + (size_t)K * rec_words * 4u, tables_bytes = (size_t)n_windows * table_words * 4u;
    RC_TRY(J.cons.ensure(tables_at + tables_bytes));
    for (DevBuf *b : {&db->keys_a, &db->keys_b, &db->idx_a, &db->idx_b}) RC_TRY(b->ensure((size_t)n_pos * sizeof(uint32_t)));
    unsigned long long *const slots = reinterpret_cast<unsigned long long *>(J.cons.as<char>() + slots_at);
    uint32_t *const seg_begin = reinterpret_cast<uint32_t *>(J.cons.as<char>() + seg_at);
    uint32_t *const recs = reinterpret_cast<uint32_t *>(J.cons.as<char>() + recs_at);
    uint32_t *const tables = reinterpret_cast<uint32_t *>(J.cons.as<char>() + tables_at);
    uint32_t *const ka = db->keys_a.as<uint32_t>(), *const kb = db->keys_b.as<uint32_t>();
    uint32_t *const ia = db->idx_a.as<uint32_t>(), *const ib = db->idx_b.as<uint32_t>();
    int key_bits = 1;
    while (key_bits < 32 && (1ull << key_bits) <= K) key_bits++;  // the keys are 0 .. K
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, ka, kb, ia, ib, (int)n_pos, 0, key_bits, db->stream));
    RC_TRY(db->sort_tmp.ensure(tmp_bytes));
    const uint32_t *const perm = db->d_perm.as<uint32_t>();
    const uint8_t *const tab = db->d_tab.as<uint8_t>();
    const bool measured = d_nearest || d_div;
    HIP_TRY(hipEventRecord(J.ev[0], db->stream));
    hipLaunchKernelGGL(consensus::group_ids_kernel, rows, block, 0, db->stream, mark, dense, n, d_ids);
    hipLaunchKernelGGL(consensus::group_keys_kernel, row_grid(n_pos), block, 0, db->stream, d_labels, db->d_order, dense, n, n_pos, K, ka, ia);
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, tmp_bytes, ka, kb, ia, ib, (int)n_pos, 0, key_bits, db->stream));
    hipLaunchKernelGGL(consensus::segment_bounds_kernel, row_grid(n_pos), block, 0, db->stream, kb, n_pos, K, seg_begin);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[1], db->stream));
    HIP_TRY(hipMemsetAsync(tables, 0, tables_bytes, db->stream));
    const dim3 tally_grid((n_windows + consensus::kWavesPerBlock - 1u) / consensus::kWavesPerBlock);
    const auto by_planes = [&](auto planes_c) {
        constexpr int PS = decltype(planes_c)::value;
        hipLaunchKernelGGL(consensus::tally_vote_kernel<PS>, tally_grid, block, 0, db->stream, db->d_planes, kb, ib, seg_begin, K, chunk, n_windows,
                           L, W, perm, tab, tables, recs, d_codes);
        if (n_windows > 1u)
            hipLaunchKernelGGL(consensus::vote_tables_kernel<PS>, dim3(n_windows - 1u), dim3(64), 0, db->stream, kb, seg_begin, K, chunk, L, W, perm,
                               tab, tables, recs, d_codes);
    };
    if (P == 5) by_planes(ic<5>{});
    else if (P == 3) by_planes(ic<3>{});
    else by_planes(ic<2>{});
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[2], db->stream));
    if (d_div) HIP_TRY(hipMemsetAsync(d_div, 0xff, (size_t)n * sizeof(uint32_t), db->stream));
    if (d_nearest) HIP_TRY(hipMemsetAsync(slots, 0xff, (size_t)K * 8u, db->stream));
    if (measured)
        hipLaunchKernelGGL(consensus::measure_kernel, rows, block, 0, db->stream, db->d_planes, kb, ib, seg_begin, K, P, W, recs, db->d_order, d_div,
                           d_nearest ? slots : (unsigned long long *)nullptr);
    hipLaunchKernelGGL(consensus::finish_groups_kernel, row_grid(K), block, 0, db->stream, seg_begin, slots, K, d_sizes, d_nearest);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(J.ev[3], db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    float sort_ms = 0.f, vote_ms = 0.f, measure_ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&sort_ms, J.ev[0], J.ev[1]));
    HIP_TRY(hipEventElapsedTime(&vote_ms, J.ev[1], J.ev[2]));
    HIP_TRY(hipEventElapsedTime(&measure_ms, J.ev[2], J.ev[3]));
    J.filter_ms = sort_ms, J.link_ms = vote_ms, J.flatten_ms = measure_ms;
    db->call_ms += sort_ms + vote_ms + measure_ms;
    db->call_launches += 6u + (n_windows > 1u ? 1u : 0u) + (measured ? 1u : 0u);  // (the scan's and the sort's launches count as one each)
    char name[64];
    note_call_kernel(db, "consensus::group_ids_kernel");
    note_call_kernel(db, "consensus::group_keys_kernel");
    note_call_kernel(db, "consensus::segment_bounds_kernel");
    snprintf(name, sizeof name, "consensus::tally_vote_kernel<%u>", P);
    note_call_kernel(db, name);
    snprintf(name, sizeof name, "consensus::vote_tables_kernel<%u>", P);
    if (n_windows > 1u) note_call_kernel(db, name);
    if (measured) note_call_kernel(db, "consensus::measure_kernel");
    note_call_kernel(db, "consensus::finish_groups_kernel");
    size_t scratch = J.parent.cap + J.cons.cap + db->sort_tmp.cap;
    for (const DevBuf *b : {&db->keys_a, &db->keys_b, &db->idx_a, &db->idx_b}) scratch += b->cap;
    log_line(2, "consensus of %u groups among %u rows, windows of %u: groups %.3f ms, sort %.3f ms, tally and vote %.3f ms, measure %.3f ms, "
             "scratch %zu B", K, n, chunk, J.count_ms, J.filter_ms, J.link_ms, J.flatten_ms, scratch);
    trim({&J.cons, &J.parent});
    trim_together(db->keys_a, {&db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp});
    return SMAFA_OK;
}

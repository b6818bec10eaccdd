// scan_host.hip.h — host code of the scan paths: one scan of a resident query set (scan_range: the fixed-bound form scan_fixed
// and the tightening form scan_kth), rows ordered and fetched to the host (fetch_rows), and the host-buffer call over them
// (scan_to_host: the near-hit ladder, the loose path, the final k-th cut).  What these decide — the ladder, the index rent, the
// first step's probe, the planner of the later steps, the order of work of a tightening scan — is kth_plan.h's; this file runs it.
// Included once by engine.hip, inside namespace smafa, behind smafa_db, launch_tiles and the index functions, in front of
// self_join.hip.h (whose scans go through scan_range).
#pragma once

// Build the block index for an automatic mode.  (a build that fails — no room for another 8 B x blocks + a row copy per subject —
// is not the scan's failure: the scan kernels answer, and the automatic modes do not try again until the store changes)
static void buy_index(smafa_db *db, uint32_t blocks) {
    if (index_build(db, blocks) == SMAFA_OK) return;
    log_line(1, "block index not built (%s): scanning as before", smafa_last_error());
    index_drop(db);
    db->index_failed_generation = db->generation + 1u;
}

static IndexSite index_site(const smafa_db *db) {
    const bool current = index_current(db);
    return {db->index_mode, db->n, db->index_min_rows, db->W, db->L, (uint32_t)kIndexMaxWords, (uint32_t)kIndexMaxBlocks,
            current, current ? db->index.B : 0u, db->index_failed_generation == db->generation + 1u};
}

// rent or buy (kth_plan.h): the scan is charged; true once the rent paid since the store last changed equals the index's price
static bool index_rent_paid(smafa_db *db, uint64_t nq, double rate, uint32_t blocks) {
    if (db->index_debt_generation != db->generation) db->index_debt_ms = 0.0, db->index_debt_generation = db->generation;
    db->index_debt_ms += index_rent_charge(nq, db->n, db->P * db->W, rate);
    return index_rent_due(db->index_debt_ms, blocks, db->n);
}

// k_tight = 0 of scan_range: ONE launch, or the index's probes.
static int scan_fixed(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t thr0, uint32_t n_tiles, smafa_hit *d_hits,
                      uint64_t cap, unsigned long long *d_count, uint32_t tile_begin) {
    const uint32_t nq = q_end - q_begin;
    // A store with a current block index answers a tight fixed bound from it: bound + 1 probes per query instead of a
    // pass over every tile (index.hip.h).  Mode 2 builds the index the first time such a scan arrives; mode 3 rents first.
    const IndexSite site = index_site(db);
    if (fixed_bound_wants_index(site, db->knobs, nq, thr0)) {
        const bool build = db->index_mode == 2 || index_rent_paid(db, nq, kRentFixedBound, thr0 + 1u);
        if (build && !site.failed) buy_index(db, thr0 + 1u);
    }
    uint8_t probe_block[kIndexMaxBlocks];
    if (index_plan(db, thr0, nq, probe_block)) {
        hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(64), 0, db->stream, (uint32_t *)d_count, 0u, (uint64_t)2);
        HIP_TRY(hipEventRecord(db->ev0, db->stream));
        RC_TRY(index_probe(db, qs, q_begin, q_end, thr0, probe_block, d_hits, cap, d_count));
        HIP_TRY(hipEventRecord(db->ev1, db->stream));
        db->timed = true;
        return SMAFA_OK;
    }
    // A handful of queries against a big store is a grid of many short-lived workgroups: there the ticket every workgroup
    // takes at its end (to find the last one, which publishes the total) costs more than a tiny fill kernel in front of the launch —
    // the rows are then reserved straight from *d_count (one-query pass over the 50M store: 65 -> 57 us streaming,
    // 22.4 -> 18.5 us with the zone level; profiles/r03_stream_nt.txt).  Big batches keep the one-launch form.
    const bool own = nq <= 64u;
    if (own) hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(64), 0, db->stream, (uint32_t *)d_count, 0u, (uint64_t)2);
    HIP_TRY(hipEventRecord(db->ev0, db->stream));
    RC_TRY(launch_tiles(db, qs, q_begin, q_end, tile_begin, n_tiles, 0, thr0, d_hits, cap, own ? nullptr : d_count, false, own ? d_count : nullptr));
    HIP_TRY(hipEventRecord(db->ev1, db->stream));
    db->timed = true;
    return SMAFA_OK;
}

// cnt[q][*] = 0 for the scan's queries
static int zero_kth_counts(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t nq) {
    const size_t cnt_stride = db->L + 1;
    RC_TRY(qs->cnt.ensure(std::max<uint64_t>(qs->nq, 64) * cnt_stride * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(qs->cnt.as<uint32_t>() + (size_t)q_begin * cnt_stride, 0, (size_t)nq * cnt_stride * sizeof(uint32_t), db->stream));
    return SMAFA_OK;
}

// bounds from the counts so far: each query's k-th smallest distance among the pairs counted
static void launch_kth_bounds(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t nq, uint32_t k_tight) {
    hipLaunchKernelGGL(kth_from_counts_kernel, dim3((nq + 255) / 256), dim3(256), 0, db->stream, qs->cnt.as<uint32_t>(), db->L + 1, k_tight,
                       qs->thr.as<uint32_t>(), q_begin, nq);
}

// kth_seed_kernel over the first `tiles` wave tiles: the seed bound alone (d_cnt == NULL), or every pair counted into d_cnt
static int launch_kth_hist(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t k_tight, uint32_t thr0, uint32_t tiles,
                           uint32_t *d_cnt) {
    const uint32_t n_chunks = (q_end - q_begin + kSeedQueries - 1) / kSeedQueries;
    const uint32_t n_groups = kth_hist_groups(d_cnt != nullptr, tiles, n_chunks, (uint32_t)db->n_cu, db->kth_groups);
    const dim3 grid(n_chunks * n_groups), block(256);
    const uint4 *planes = reinterpret_cast<const uint4 *>(db->d_planes);
    const uint32_t *qrec = qs->qrec.as<uint32_t>();
    uint32_t *thr = qs->thr.as<uint32_t>();
    auto launch = [&](auto ps, auto pq, auto w) {
        constexpr int PS = decltype(ps)::value, PQ = decltype(pq)::value, W = decltype(w)::value;
        note_kernel(db, "smafa::kth_seed_kernel<%d, %d, %d>", PS, PQ, W);
        hipLaunchKernelGGL((kth_seed_kernel<PS, PQ, W>), grid, block, 0, db->stream, planes, qrec, db->QS, db->P, db->PQ, db->W, tiles,
                           (uint32_t)db->n, q_begin, q_end, n_chunks, n_groups, k_tight, thr0, thr, d_cnt, db->L + 1);
        return true;
    };
    if (!for_shape(db->shape(), launch)) launch(ic<0>{}, ic<0>{}, ic<0>{});  // more than four words per plane: the any-shape form
    // (the call's list names the counting form as a marker of its own, after the template-id — as scan_wide_kernel's zone level)
    if (d_cnt) {
        const std::string id = db->plan_kernel;
        note_kernel(db, "%s (sample counts)", id.c_str());
    }
    HIP_TRY(hipGetLastError());
    return SMAFA_OK;
}

// k_tight >= 1 of scan_range: the steps of kth_schedule (kth_plan.h), one after the other on the handle's stream.  Rows are
// appended to a scratch list while the bounds are still running; the filter pass then keeps the ones within the final bounds.
static int scan_kth(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t k_tight, uint32_t thr0, uint32_t n_tiles,
                    smafa_hit *d_hits, uint64_t cap, unsigned long long *d_count) {
    const uint32_t nq = q_end - q_begin;
    unsigned long long *d_ctr = db->ctrs.as<unsigned long long>();
    const bool count_first = kth_count_first(k_tight, db->count_first_k, db->shape(), db->knobs, thr0);
    const uint32_t sample_tiles = kth_sample_tiles(count_first, db->kth_sample_div, db->kth_sample_min_tiles, n_tiles, k_tight);
    const uint64_t scratch_rows = kth_scratch_rows(count_first, sample_tiles, nq, k_tight, cap);
    if (scratch_rows) RC_TRY(db->scratch.ensure(scratch_rows * sizeof(smafa_hit)));
    smafa_hit *d_scratch = db->scratch.as<smafa_hit>();
    HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(unsigned long long), db->stream));
    hipLaunchKernelGGL(fill_u32_kernel, dim3((nq + 255) / 256), dim3(256), 0, db->stream, qs->thr.as<uint32_t>() + q_begin, thr0, (uint64_t)nq);
    HIP_TRY(hipEventRecord(db->ev0, db->stream));
    const KthSchedule plan = kth_schedule(n_tiles, k_tight, count_first, sample_tiles, kth_hist_seed(k_tight, db->L, (uint32_t)kSeedBins, db->kth_hist_seed));
    for (uint32_t i = 0; i < plan.n; i++) {
        const uint32_t t0 = plan.step[i].tile_begin, t1 = plan.step[i].tile_end;
        switch (plan.step[i].kind) {
        case KthStep::ZeroCounts: RC_TRY(zero_kth_counts(db, qs, q_begin, nq)); break;
        case KthStep::SeedHist: RC_TRY(launch_kth_hist(db, qs, q_begin, q_end, k_tight, thr0, t1, nullptr)); break;
        case KthStep::SampleHist: RC_TRY(launch_kth_hist(db, qs, q_begin, q_end, k_tight, thr0, t1, qs->cnt.as<uint32_t>())); break;
        case KthStep::SeedScan:
        case KthStep::Count: RC_TRY(launch_tiles(db, qs, q_begin, q_end, t0, t1, k_tight, thr0, nullptr, 0, nullptr)); break;
        case KthStep::CountAppend: RC_TRY(launch_tiles(db, qs, q_begin, q_end, t0, t1, k_tight, thr0, d_scratch, scratch_rows, nullptr)); break;
        case KthStep::BoundsFromCounts: launch_kth_bounds(db, qs, q_begin, nq, k_tight); break;
        case KthStep::FixedAppendScratch: RC_TRY(launch_tiles(db, qs, q_begin, q_end, t0, t1, 0, thr0, d_scratch, scratch_rows, nullptr, true)); break;
        case KthStep::FixedAppendCaller:
            RC_TRY(launch_tiles(db, qs, q_begin, q_end, t0, t1, 0, thr0, d_hits, cap, d_count, true));
            HIP_TRY(hipEventRecord(db->ev1, db->stream));
            db->timed = true;
            break;
        case KthStep::Filter:
            HIP_TRY(hipEventRecord(db->ev1, db->stream));  // smafa_last_scan_ms: the scan kernels, not the filter pass below
            db->timed = true;
            HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), db->stream));
            hipLaunchKernelGGL(filter_rows_kernel, dim3((uint32_t)std::min<uint64_t>(1024, (scratch_rows + 255) / 256)), dim3(256), 0,
                               db->stream, d_scratch, d_ctr, (unsigned long long)scratch_rows, d_hits, (unsigned long long)cap,
                               d_count, qs->thr.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(unsigned long long), db->stream));  // counters are zero between scans
            break;
        }
    }
    return SMAFA_OK;
}

// Scan queries [q_begin, q_end) of a resident set against the whole store; rows and their count stay on
// the device.
// k_tight = 0: ONE launch (up to 64 queries: a one-workgroup kernel zeroes *d_count first and nobody takes a ticket), fixed
// bound max_div: the kernel appends straight into the caller's list and — big batches — its last
// workgroup publishes the total in *d_count (which may exceed cap: the rows past it are dropped, the count is exact).
// k_tight >= 1: the bound of each query is lowered to its running k-th smallest distance while the scan proceeds.
// Workgroups of one launch run side by side and would all start from the loose initial bound, so the store is walked
// in segments that grow 8x per launch (bounds tighten between launches), after a seed launch over the first segment
// that only lowers the bounds and appends nothing.  Rows are appended to a scratch list while the bounds are still
// running; filter_rows_kernel then keeps the ones within the final bounds.
// tile_begin (fixed-bound form only): the scan kernels start at that wave tile — the self-join's triangular cut; an index
// probe has no tile range and answers over the whole store.
static int scan_range(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t max_div,
                      uint32_t k_tight, smafa_hit *d_hits, uint64_t cap, unsigned long long *d_count, uint32_t tile_begin = 0) {
    const uint32_t nq = q_end - q_begin;
    db->last_launches = 0;
    db->timed = false;
    db->call_timed = false;
    if (nq == 0 || db->n == 0) {
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), db->stream));
        return SMAFA_OK;
    }
    int prc = maybe_resort(db);
    if (prc) return prc;
    const uint32_t thr0 = std::min<uint32_t>(max_div, db->L);  // a distance never exceeds seq_len
    const uint32_t n_tiles = (uint32_t)((db->n + kWaveTile - 1) / kWaveTile);
    if (k_tight == 0) return scan_fixed(db, qs, q_begin, q_end, thr0, n_tiles, d_hits, cap, d_count, tile_begin);
    return scan_kth(db, qs, q_begin, q_end, k_tight, thr0, n_tiles, d_hits, cap, d_count);
}

// the stream has just been synchronised after a scan_range: fold its kernel time into the call's totals
static void note_call_scan(smafa_db *db) {
    db->call_scans++;
    db->call_launches += db->last_launches;
    float ms = 0.f;
    if (db->timed && hipEventElapsedTime(&ms, db->ev0, db->ev1) == hipSuccess) db->call_ms += ms;
    db->life_ms += ms;
    db->life_launches += db->last_launches;
}

// One scan of a host-buffer call: scan_range into the handle's row list, the row count back on the host (it may exceed
// hits_cap(): the rows past it were dropped, the count is exact), the scan booked to the call's totals.
static int scan_counted(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t max_div, uint32_t k_tight,
                        unsigned long long *count) {
    RC_TRY(scan_range(db, qs, q_begin, q_end, max_div, k_tight, db->hits.as<smafa_hit>(), db->hits_cap(), db->count.as<unsigned long long>()));
    HIP_TRY(hipMemcpyAsync(count, db->count.p, sizeof *count, hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    note_call_scan(db);
    return SMAFA_OK;
}

static bool hit_less(const smafa_hit &x, const smafa_hit &y) {
    if (x.query != y.query) return x.query < y.query;
    if (x.dist != y.dist) return x.dist < y.dist;
    return x.subject < y.subject;
}

// ---- ordering rows on the device: (query, dist, subject) packed into one 64-bit radix key -------------
__global__ void rows_to_keys_kernel(const smafa_hit *rows, uint64_t n, uint32_t q_begin, uint32_t dist_bits,
                                    unsigned long long *keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const smafa_hit h = rows[i];
    keys[i] = ((unsigned long long)(h.query - q_begin) << (32 + dist_bits)) | ((unsigned long long)h.dist << 32) | h.subject;
}

__global__ void keys_to_rows_kernel(const unsigned long long *keys, uint64_t n, uint32_t q_begin, uint32_t dist_bits,
                                    smafa_hit *rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    smafa_hit h;
    h.subject = (uint32_t)k;
    h.dist = (uint32_t)(k >> 32) & ((1u << dist_bits) - 1u);
    h.query = (uint32_t)(k >> (32 + dist_bits)) + q_begin;
    rows[i] = h;
}

// Sort db->hits[0..count) by (query, dist, subject) in place with a device radix sort; returns false (and leaves
// the rows untouched) when the key does not fit 64 bits — the caller then orders them on the host.
static int sort_rows_on_device(smafa_db *db, uint64_t count, uint32_t q_begin, uint32_t q_end, bool *sorted,
                               smafa_hit *rows = nullptr) {
    *sorted = false;
    if (!rows) rows = db->hits.as<smafa_hit>();  // (the self-join orders its own list)
    uint32_t dist_bits = 1;
    while ((1u << dist_bits) <= db->L) dist_bits++;
    uint32_t q_bits = 1;
    while (q_bits < 32 && (1ull << q_bits) < (uint64_t)(q_end - q_begin)) q_bits++;
    if (dist_bits + q_bits > 32 || count > 0x7fffffffull) return SMAFA_OK;
    int rc = db->keys_a.ensure(count * sizeof(unsigned long long));
    if (!rc) rc = db->keys_b.ensure(count * sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long *ka = db->keys_a.as<unsigned long long>(), *kb = db->keys_b.as<unsigned long long>();
    const uint32_t blocks = (uint32_t)((count + 255) / 256);
    hipLaunchKernelGGL(rows_to_keys_kernel, dim3(blocks), dim3(256), 0, db->stream, rows, count, q_begin, dist_bits, ka);
    size_t tmp_bytes = 0;
    const int end_bit = (int)(32 + dist_bits + q_bits);
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, ka, kb, (int)count, 0, end_bit, db->stream));
    rc = db->sort_tmp.ensure(tmp_bytes);
    if (rc) return rc;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(db->sort_tmp.p, tmp_bytes, ka, kb, (int)count, 0, end_bit, db->stream));
    hipLaunchKernelGGL(keys_to_rows_kernel, dim3(blocks), dim3(256), 0, db->stream, kb, count, q_begin, dist_bits, rows);
    HIP_TRY(hipGetLastError());
    *sorted = true;
    return SMAFA_OK;
}

// Append db->hits[0..count) — rows of queries [q_begin, q_end) — to `out`, ordered by (query, dist, subject).
static int fetch_rows(smafa_db *db, uint64_t count, uint32_t q_begin, uint32_t q_end, std::vector<smafa_hit> &out) {
    if (count == 0) return SMAFA_OK;
    bool sorted = false;
    if (count >= 4096) {  // small lists are cheaper to order on the host
        int rc = sort_rows_on_device(db, count, q_begin, q_end, &sorted);
        if (rc) return rc;
    }
    const double t0 = now_seconds();
    HIP_TRY(hipStreamSynchronize(db->stream));
    const double t1 = now_seconds();
    const size_t old = out.size();
    out.resize(old + count);
    const double t2 = now_seconds();
    HIP_TRY(hipMemcpyAsync(out.data() + old, db->hits.p, count * sizeof(smafa_hit), hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    const double t3 = now_seconds();
    if (!sorted) std::sort(out.begin() + old, out.end(), hit_less);  // each range ordered => `out` ordered
    if (count >= (1u << 20))
        log_line(2, "%llu rows: scan + device sort %.2f ms, host buffer %.2f ms, copy back %.2f ms", (unsigned long long)count,
                 (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3);
    return SMAFA_OK;
}

// Collect all qualifying rows of queries [q_begin, q_end) into `out` (host).  First the plain bound when there
// is one (rows within max_div are usually few); if they do not fit, tighten to the k-th smallest distance; if
// that still does not fit, halve the query range.  Ranges are visited in ascending query order and each is
// ordered by (query, dist, subject) — on the device when it is big enough to matter — so `out` is ordered.
static int collect_range(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t max_div,
                         uint32_t max_num_hits, std::vector<smafa_hit> &out) {
    const uint32_t k_tight = max_num_hits == SMAFA_NONE ? 0u : max_num_hits;
    unsigned long long count = 0;
    bool done = false;
    for (int attempt = 0; attempt < 2 && !done; attempt++) {
        uint32_t k;
        if (attempt == 0) {
            if (max_div == SMAFA_NONE && k_tight) continue;  // no bound at all: go straight to tightening
            k = 0;
        } else {
            if (!k_tight) break;
            k = k_tight;
            // counting first, the scan returns k rows per query plus ties: make room for them up front (up to 64M rows)
            if (kth_count_first(k, db->count_first_k, db->shape(), db->knobs, std::min<uint32_t>(max_div, db->L))) {
                const uint64_t want = std::min<uint64_t>((uint64_t)(q_end - q_begin) * ((uint64_t)k + 64u), 1ull << 26);
                if (db->hits_cap() < want) {
                    int erc = db->hits.ensure(want * sizeof(smafa_hit));
                    if (erc) return erc;
                }
            }
        }
        RC_TRY(scan_counted(db, qs, q_begin, q_end, max_div, k, &count));
        done = count <= db->hits_cap();
    }
    if (!done) {
        // a fixed-bound scan reports its exact total: make room for it and scan once more (up to 128M rows = 1.5 GB)
        if (!k_tight && count <= (1ull << 27)) {
            int rc = db->hits.ensure(count * sizeof(smafa_hit));
            if (rc) return rc;
            return collect_range(db, qs, q_begin, q_end, max_div, max_num_hits, out);
        }
        if (q_end - q_begin > 1) {
            const uint32_t mid = q_begin + (q_end - q_begin) / 2;
            int rc = collect_range(db, qs, q_begin, mid, max_div, max_num_hits, out);
            if (rc) return rc;
            return collect_range(db, qs, mid, q_end, max_div, max_num_hits, out);
        }
        // one query with more rows than the buffer: it can have at most one row per subject
        int rc = db->hits.ensure(std::max<uint64_t>(count, db->n) * sizeof(smafa_hit));
        if (rc) return rc;
        return collect_range(db, qs, q_begin, q_end, max_div, max_num_hits, out);
    }
    return fetch_rows(db, count, q_begin, q_end, out);
}

// ---- the host-buffer call: near-hit ladder, loose path, k-th cut (the rules and their measurements: kth_plan.h) ------------
// Every stride-th of `ns` code rows as a query set of their own (scratch_q3), asked for every pair within `bound`
// (a plain fixed-bound launch, not the tightening form with its seed and growing segments: up to a dozen small launches
// cost a 256-query sample 0.9 ms where this costs 0.4).  *count > hits_cap(): too dense to look at, no rows.
static int sample_rows(smafa_db *db, const uint8_t *codes, uint32_t stride, uint32_t ns, uint32_t bound, unsigned long long *count,
                       std::vector<smafa_hit> &rows) {
    std::vector<uint8_t> sample((size_t)ns * db->L);
    for (uint32_t i = 0; i < ns; i++) memcpy(&sample[(size_t)i * db->L], codes + (size_t)i * stride * db->L, db->L);
    RC_TRY(qset_fill(&db->scratch_q3, db, sample.data(), ns));
    RC_TRY(scan_counted(db, &db->scratch_q3, 0, ns, bound, 0, count));
    return *count <= db->hits_cap() ? fetch_rows(db, *count, 0, ns, rows) : SMAFA_OK;
}

// one call's walk down the ladder
struct Ladder {
    smafa_db *db;
    uint32_t k_mode, limit;  // the call's k, and its own bound min(max_div, L)
    LadderBounds bounds;
    bool run_step[kLadderMax] = {true, true, true, true};
    bool planned = false;              // the later steps have been chosen (plan_later)
    uint32_t index_step = UINT32_MAX;  // position in the ladder of the step the index answers
    // the open batch
    std::vector<uint32_t> ids;        // open queries: position in the current batch -> the caller's number (empty: same)
    std::vector<uint8_t> open_codes;  // ... and their code rows
    const uint8_t *cur;               // code rows of the current batch: the caller's, then open_codes
    uint32_t cur_n;
    smafa_qset *qs;
    std::vector<smafa_hit> done;  // rows of the finished queries (the caller's query numbers), ordered
};

static void merge_done(Ladder &l, std::vector<smafa_hit> &more) {  // both ordered, disjoint queries
    if (l.done.empty()) {
        l.done.swap(more);
        return;
    }
    std::vector<smafa_hit> all(l.done.size() + more.size());
    std::merge(l.done.begin(), l.done.end(), more.begin(), more.end(), all.begin(), hit_less);
    l.done.swap(all);
}

// choose the steps from `from` on from a sample of the open batch (choose_later_steps)
static int plan_later(Ladder &l, size_t from) {
    smafa_db *db = l.db;
    l.planned = true;
    const LaterSteps later = later_steps(l.bounds, from, l.limit);
    if (!later.any) return SMAFA_OK;
    const uint32_t ns = planner_sample(l.cur_n);
    unsigned long long count = 0;
    std::vector<smafa_hit> rows;
    RC_TRY(sample_rows(db, l.cur, l.cur_n / ns, ns, l.bounds[later.last], &count, rows));
    std::vector<uint32_t> kth(ns, UINT32_MAX);  // k-th smallest distance of each sample query within the last bound
    if (count > db->hits_cap()) std::fill(kth.begin(), kth.end(), 0u);  // too dense to look at: every step will finish plenty
    for (size_t i = 0; i < rows.size();) {
        size_t j = i;
        while (j < rows.size() && rows[j].query == rows[i].query) j++;
        if (j - i >= l.k_mode) kth[rows[i].query] = rows[i + l.k_mode - 1].dist;
        i = j;
    }
    const LaterChoice best = choose_later_steps(kth.data(), ns, l.bounds, from, later.last, ladder_cols(db->L));
    for (size_t t = from; t < l.bounds.n; t++) l.run_step[t] = t <= later.last && ((best.mask >> (t - from)) & 1u);
    std::string chosen;
    for (size_t t = 0; t + from <= later.last; t++)
        if ((best.mask >> t) & 1u) chosen += " " + std::to_string(l.bounds[from + t]);
    log_line(2, "near-hit plan from a sample of %u open queries: further steps at bounds [%s ] -> %.2f of the loose path's cost",
             ns, chosen.c_str(), best.cost);
    return SMAFA_OK;
}

// ask the first step of a sample of the batch (first_step_probed); where it finishes too few, skip it and plan the rest
static int probe_first_step(Ladder &l) {
    const uint32_t ns = kProbeSample;
    unsigned long long count = 0;
    std::vector<smafa_hit> rows;
    RC_TRY(sample_rows(l.db, l.cur, l.cur_n / ns, ns, l.bounds[0], &count, rows));
    uint32_t finished = ns;  // (too dense to look at: the step will finish plenty)
    if (count <= l.db->hits_cap()) {
        std::vector<uint32_t> have(ns, 0);
        for (const smafa_hit &h : rows) have[h.query]++;
        finished = 0;
        for (uint32_t v : have) finished += v >= l.k_mode;
    }
    if (!first_step_probe_skips(finished, ns)) return SMAFA_OK;
    l.run_step[0] = false;
    log_line(2, "near-hit probe: %u of %u sampled queries finish at bound %u: the step is skipped", finished, ns, l.bounds[0]);
    return plan_later(l, 1);
}

// the open batch becomes the queries at positions `open` (ascending) of the current one, as a query set of its own
static int compact_open(Ladder &l, const std::vector<uint32_t> &open) {
    const size_t L = l.db->L;
    std::vector<uint32_t> next_ids(open.size());
    std::vector<uint8_t> next_codes(open.size() * L);
    for (size_t i = 0; i < open.size(); i++) {
        next_ids[i] = l.ids.empty() ? open[i] : l.ids[open[i]];
        memcpy(&next_codes[i * L], l.cur + (size_t)open[i] * L, L);
    }
    l.ids.swap(next_ids);
    l.open_codes.swap(next_codes);
    l.cur = l.open_codes.data();
    l.cur_n = (uint32_t)open.size();
    if (l.cur_n == 0) return SMAFA_OK;
    RC_TRY(qset_fill(&l.db->scratch_q2, l.db, l.cur, l.cur_n));
    l.qs = &l.db->scratch_q2;
    return SMAFA_OK;
}

// After a step: the later steps are planned now where that is due (plans_later_now: not planned yet, at least 2048 open, a
// later step exists) and the ladder goes on; otherwise it goes on only where `otherwise` says so.
static int plan_or_stop(Ladder &l, size_t step, bool otherwise, bool *go_on) {
    *go_on = otherwise;
    if (!plans_later_now(l.planned, l.cur_n, step, l.bounds.n)) return SMAFA_OK;
    *go_on = true;
    return plan_later(l, step + 1);  // (the sample is drawn from the open batch)
}

// One step of the ladder over the open batch.  *go_on: the ladder continues with the next step.
static int run_ladder_step(Ladder &l, size_t step, bool *go_on) {
    smafa_db *db = l.db;
    const uint32_t bound = l.bounds[step], cur_n = l.cur_n;
    *go_on = false;
    if (l.limit <= bound || (step > 0 && bound <= l.bounds[step - 1])) return SMAFA_OK;
    *go_on = true;
    if (!l.run_step[step]) return SMAFA_OK;
    unsigned long long count = 0;
    // the step itself runs in the tightening mode (bound lowered to each query's k-th distance as the scan
    // proceeds), so on dense stores only the rows within the final bound come back, not every pair within it
    // (the index's step is a fixed-bound scan: every pair within the bound, from bound + 1 probes per query)
    RC_TRY(scan_counted(db, l.qs, 0, cur_n, bound, step == l.index_step ? 0u : l.k_mode, &count));
    if (count > db->hits_cap()) {
        *go_on = step == l.index_step;  // (more rows than the buffer holds: the tightening steps take over)
        return SMAFA_OK;                // too dense to look at: the full path decides
    }
    if (count == 0) return plan_or_stop(l, step, false, go_on);  // nobody within this bound: do the later steps pay?
    std::vector<smafa_hit> near;
    RC_TRY(fetch_rows(db, count, 0, cur_n, near));
    std::vector<uint32_t> have(cur_n, 0);
    for (const smafa_hit &h : near) have[h.query]++;
    std::vector<uint32_t> open;  // positions in the current batch that still need an answer, ascending
    for (uint32_t q = 0; q < cur_n; q++)
        if (have[q] < l.k_mode) open.push_back(q);
    if (open.size() == cur_n) return plan_or_stop(l, step, false, go_on);
    std::vector<smafa_hit> fin;
    fin.reserve(near.size());
    for (smafa_hit h : near)
        if (have[h.query] >= l.k_mode) {
            if (!l.ids.empty()) h.query = l.ids[h.query];  // ascending map: the order is kept
            fin.push_back(h);
        }
    merge_done(l, fin);
    log_line(2, "near-hit step at bound %u finished %u of %u queries", bound, cur_n - (uint32_t)open.size(), cur_n);
    const bool paid = step_paid(cur_n - open.size(), cur_n, step + 1 < l.bounds.n ? l.bounds[step + 1] : 0u);
    RC_TRY(compact_open(l, open));
    if (l.cur_n == 0) {
        *go_on = false;
        return SMAFA_OK;
    }
    return plan_or_stop(l, step, l.planned || paid, go_on);  // (a small batch: round 2's rule of thumb)
}

// drop rows above the k-th smallest distance of their query (the device bound only tightens); `out` is ordered
static void cut_at_kth(std::vector<smafa_hit> &out, uint32_t k) {
    size_t w = 0, i = 0;
    while (i < out.size()) {
        size_t j = i;
        while (j < out.size() && out[j].query == out[i].query) j++;
        const size_t cnt = j - i;
        const uint32_t kth = cnt >= k ? out[i + k - 1].dist : UINT32_MAX;
        for (size_t t = i; t < j && out[t].dist <= kth; t++) out[w++] = out[t];
        i = j;
    }
    out.resize(w);
}

// The index in front of the ladder: rent or buy for calls WITHOUT a usable bound (mode 3), then the largest bound a current
// index serves this batch in place of the ladder's steps up to it (ladder_with_index).
static void ladder_index(Ladder &l, uint64_t n_queries) {
    smafa_db *db = l.db;
    const IndexSite site = index_site(db);
    if (loose_call_pays_rent(site, db->knobs, db->two_phase, l.k_mode, n_queries, l.limit, l.bounds[0])) {
        const uint32_t want = index_blocks_wanted(db->alphabet == SMAFA_ALPHABET_AA, db->P, db->n, db->L, (uint32_t)kIndexMaxBlocks);
        if (loose_call_wants_index(site, want, l.bounds[0]) && index_rent_paid(db, n_queries, kRentLoose, want)) buy_index(db, want);
    }
    if (l.k_mode >= 1 && n_queries > 64) {
        uint8_t blocks[kIndexMaxBlocks];
        uint32_t d = index_current(db) ? db->index.B : 0u;
        while (d > 0 && !index_plan(db, d - 1u, (uint32_t)n_queries, blocks)) d--;
        if (d > 0 && ladder_with_index(l.bounds, d - 1u, l.limit)) l.index_step = 0;
    }
}

int scan_to_host(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div,
                 uint32_t max_num_hits, std::vector<smafa_hit> &out) {
    out.clear();
    db->call_ms = 0.f;
    db->call_launches = db->call_scans = 0;
    if (n_queries == 0) return SMAFA_OK;
    if (n_queries > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "too many queries in one batch");
    int rc = use_device(db);
    if (rc) return rc;
    rc = db->count.ensure(sizeof(unsigned long long));
    if (!rc && db->hits_cap() < (1ull << 22)) rc = db->hits.ensure((1ull << 22) * sizeof(smafa_hit));  // 4M rows = 48 MiB
    if (rc) return rc;
    rc = validate_codes(db, query_codes, n_queries);
    if (rc) return rc;
    rc = qset_fill(&db->scratch_q, db, query_codes, n_queries);
    if (rc) return rc;
    Ladder l{db, max_num_hits == SMAFA_NONE ? 0u : max_num_hits, std::min<uint32_t>(max_div, db->L), ladder_bounds(db->L, db->W, db->P, n_queries)};
    l.cur = query_codes;
    l.cur_n = (uint32_t)n_queries;
    l.qs = &db->scratch_q;
    ladder_index(l, n_queries);
    const bool laddered = ladder_runs(l.k_mode, db->knobs, db->two_phase, n_queries);
    if (first_step_probed(laddered, db->ladder_probe, n_queries, l.limit, l.bounds[0], l.index_step == 0)) RC_TRY(probe_first_step(l));
    bool go_on = laddered;
    for (size_t step = 0; go_on && step < l.bounds.n && l.cur_n >= kLadderMinQueries; step++) RC_TRY(run_ladder_step(l, step, &go_on));
    if (l.cur_n > 0) {  // whoever is left: the loose path
        std::vector<smafa_hit> far;
        RC_TRY(collect_range(db, l.qs, 0, l.cur_n, max_div, max_num_hits, far));
        if (!l.ids.empty())
            for (smafa_hit &h : far) h.query = l.ids[h.query];
        merge_done(l, far);
    }
    out.swap(l.done);
    if (max_num_hits != SMAFA_NONE && max_num_hits >= 1) cut_at_kth(out, max_num_hits);
    trim({&db->scratch});
    trim_together(db->keys_a, {&db->keys_b, &db->sort_tmp});
    return SMAFA_OK;
}

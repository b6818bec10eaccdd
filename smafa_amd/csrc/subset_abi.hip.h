// subset_abi.hip.h — the two calls that take rows out of a resident store, and their four entry points: a subset of the store as
// a NEW store (subset_store; smafa_db_subset_launch, smafa_db_subset) and its sequences back as code bytes (store_rows;
// smafa_db_rows_launch, smafa_db_rows).  Kernels: subset.hip.h.  Neither is a consumer of the join and neither enters its call
// frame: the source's join state, index, retry rows and captured graph stay as they are (the rows call may bring pos_of[] up to
// date, as any join would).  Both time themselves with the handle's two events and report like a self-store call
// (smafa_last_call_kernels, smafa_last_call_stats, smafa_last_scan_ms).
// Included once by engine.hip, inside extern "C", behind classify_abi.hip.h.
#pragma once

extern "C++" {

// what a call of this file starts and ends with on the source handle
static int subset_call_begin(smafa_db *db) {
    RC_TRY(use_device(db));
    db->call_kernels.clear();
    db->call_ms = 0.f;
    db->call_launches = db->call_scans = db->last_launches = 0;
    db->timed = false;
    db->call_timed = true;
    HIP_TRY(hipEventRecord(db->ev0, db->stream));
    return SMAFA_OK;
}
static int subset_call_end(smafa_db *db) {
    HIP_TRY(hipEventRecord(db->ev1, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, db->ev0, db->ev1));
    db->call_ms = ms;
    db->life_ms += ms;
    db->life_launches += db->call_launches;
    return SMAFA_OK;
}

// The subset.  d_keep: n uint32 on the device (nullptr for an empty source); d_old_of_new: n uint32 or nullptr; room: the entries
// the caller's old_of_new holds (the host form's cap; the launch form: no limit) — checked once k is known, before anything is
// allocated for the result.  *out and *n_kept were set to NULL and 0 by the entry point.
static int subset_steps(smafa_db *db, const char *who, const uint32_t *d_keep, int invert, smafa_db *sub, uint32_t *d_old_of_new,
                        uint64_t room, uint64_t *n_kept) {
    const uint32_t n = (uint32_t)db->n;
    // ---- the layout, the plane count: the source's, copied
    sub->P = db->P;
    if (db->layout_set) {
        sub->perm = db->perm;
        sub->tab = db->tab;
        RC_TRY(sub->d_perm.ensure(sub->perm.size() * sizeof(uint32_t)));
        RC_TRY(sub->d_tab.ensure(sub->tab.size()));
        HIP_TRY(hipMemcpyAsync(sub->d_perm.p, sub->perm.data(), sub->perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
        HIP_TRY(hipMemcpyAsync(sub->d_tab.p, sub->tab.data(), sub->tab.size(), hipMemcpyHostToDevice, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        sub->layout_set = true;
    }
    RC_TRY(subset_call_begin(db));
    if (n == 0) return subset_call_end(db);
    // ---- flags and their two exclusive sums; the scratch is the RESULT's (the source's buffers are not touched)
    const size_t words = (size_t)n + 1u;
    for (DevBuf *b : {&sub->keys_a, &sub->keys_b, &sub->idx_a, &sub->idx_b}) RC_TRY(b->ensure(words * sizeof(uint32_t)));
    uint32_t *const flag_s = sub->keys_a.as<uint32_t>(), *const flag_p = sub->keys_b.as<uint32_t>();
    uint32_t *const new_number = sub->idx_a.as<uint32_t>(), *const new_position = sub->idx_b.as<uint32_t>();
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, flag_s, new_number, (int)words, db->stream));
    RC_TRY(sub->sort_tmp.ensure(tmp_bytes));
    const dim3 block(256);
    hipLaunchKernelGGL(subset::keep_flags_kernel, row_grid(n + 1u), block, 0, db->stream, d_keep, db->d_order, n, invert ? 1u : 0u, flag_s, flag_p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sub->sort_tmp.p, tmp_bytes, flag_s, new_number, (int)words, db->stream));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sub->sort_tmp.p, tmp_bytes, flag_p, new_position, (int)words, db->stream));
    db->call_launches += 3u;  // (a sum's launches count as one)
    note_call_kernel(db, "subset::keep_flags_kernel");
    // ---- the kept rows of every run of the source
    const uint32_t n_runs = (uint32_t)db->runs.size();
    std::vector<uint32_t> ends(n_runs), kept_before(n_runs, 0);
    {
        uint64_t at = 0;
        for (uint32_t r = 0; r < n_runs; r++) ends[r] = (uint32_t)(at += db->runs[r].rows);  // (the last one is n)
    }
    RC_TRY(sub->upload.ensure(std::max<size_t>(2u * n_runs, 1u) * sizeof(uint32_t)));
    uint32_t *const d_ends = sub->upload.as<uint32_t>(), *const d_kept_before = d_ends + n_runs;
    if (n_runs) {
        HIP_TRY(hipMemcpyAsync(d_ends, ends.data(), n_runs * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
        hipLaunchKernelGGL(subset::run_ends_kernel, row_grid(n_runs), block, 0, db->stream, new_position, d_ends, n_runs, d_kept_before);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(kept_before.data(), d_kept_before, n_runs * sizeof(uint32_t), hipMemcpyDeviceToHost, db->stream));
        db->call_launches++;
        note_call_kernel(db, "subset::run_ends_kernel");
    }
    uint32_t k = 0;
    HIP_TRY(hipMemcpyAsync(&k, new_number + n, sizeof k, hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));  // (the launch form needs k on the host anyway)
    *n_kept = k;
    if (d_old_of_new && k > room)
        return set_error(SMAFA_ERR_CAPACITY, "%s: old_of_new too small: %u rows kept, capacity %llu", who, k, (unsigned long long)room);
    if (k) {
        // ---- the result's block: allocated here, by hand, so that a failure leaves nothing behind
        const uint64_t need = ((uint64_t)k + kWaveTile - 1) / kWaveTile;
        const uint64_t cap_tiles = (std::max<uint64_t>(need, 64) + kWgWaves - 1) / kWgWaves * kWgWaves;
        const size_t bytes = cap_tiles * sub->tile_words() * sizeof(uint32_t), order_bytes = cap_tiles * kWaveTile * sizeof(uint32_t);
        if (hipMalloc(&sub->d_planes, bytes) != hipSuccess || hipMalloc(&sub->d_order, order_bytes) != hipSuccess ||
            hipMalloc(&sub->d_zone, cap_tiles * sizeof(uint4)) != hipSuccess)  // (what was allocated goes with the handle)
            return set_error(SMAFA_ERR_NOMEM, "%s: no device memory for a store of %u rows (%zu bytes of planes)", who, k, bytes);
        sub->cap_tiles = cap_tiles;
        // zero-fill, as reserve_tiles leaves a fresh block: the padding of the last tile reads as all-zero planes
        HIP_TRY(hipMemsetAsync(sub->d_planes, 0, bytes, db->stream));
        HIP_TRY(hipMemsetAsync(sub->d_order, 0, order_bytes, db->stream));
        HIP_TRY(hipMemsetAsync(sub->d_zone, 0, cap_tiles * sizeof(uint4), db->stream));
        hipLaunchKernelGGL(subset::move_rows_kernel, row_grid(n), block, 0, db->stream, db->d_planes, sub->d_planes, db->d_order, sub->d_order,
                           new_number, new_position, n, db->P * db->W, d_old_of_new);
        HIP_TRY(hipGetLastError());
        // the zone words are the subset's own: a new tile usually straddles two old ones
        const uint32_t n_tiles = (uint32_t)need;
        hipLaunchKernelGGL(zone_kernel, dim3((n_tiles + kWgWaves - 1) / kWgWaves), block, 0, db->stream, reinterpret_cast<const uint4 *>(sub->d_planes),
                           sub->P, sub->W, sub->L, 0u, n_tiles, k, sub->d_zone);
        HIP_TRY(hipGetLastError());
        db->call_launches += 2u;
        note_call_kernel(db, "subset::move_rows_kernel");
        note_call_kernel(db, "smafa::zone_kernel");
        std::vector<uint4> z(n_tiles);
        HIP_TRY(hipMemcpyAsync(z.data(), sub->d_zone, z.size() * sizeof(uint4), hipMemcpyDeviceToHost, db->stream));
        RC_TRY(subset_call_end(db));
        note_zone_words(sub, 0, z.data(), z.size());
    } else {
        RC_TRY(subset_call_end(db));
    }
    // ---- what the result inherits: every run its kept rows and its `sorted`; the quarter rule's count as the source's was made
    for (uint32_t r = 0; r < n_runs; r++) {
        const uint32_t kept = kept_before[r] - (r ? kept_before[r - 1] : 0u);
        if (kept) sub->runs.push_back({kept, db->runs[r].sorted});
    }
    sub->rows_since_sort = n_runs && db->runs[0].sorted ? k - kept_before[0] : k;
    sub->n = k;
    sub->generation++;
    if (n > (1u << 20))
        for (DevBuf *b : {&sub->keys_a, &sub->keys_b, &sub->idx_a, &sub->idx_b, &sub->sort_tmp}) b->release();
    log_line(2, "subset of %u rows: %u kept in %zu runs, moved on the device in %.3f ms; %.2f shared filter bits per tile (the source: %.2f)", n, k,
             sub->runs.size(), db->call_ms, zone_bits_mean(sub), zone_bits_mean(db));
    return SMAFA_OK;
}

static int subset_store(smafa_db *db, const char *who, const uint32_t *d_keep, int invert, smafa_db **out, uint32_t *d_old_of_new, uint64_t room,
                        uint64_t *n_kept) {
    smafa_db *sub = nullptr;
    RC_TRY(smafa_db_create(&sub, db->device, db->alphabet, db->L));
    const int rc = subset_steps(db, who, d_keep, invert, sub, d_old_of_new, room, n_kept);
    if (rc) {
        (void)hipStreamSynchronize(db->stream);  // nothing enqueued may still write the result's block
        smafa_db_destroy(sub);
        (void)hipGetLastError();  // a failed hipMalloc stays the thread's last error until it is read: the source's next launch would take it for its own
        return rc;
    }
    *out = sub;
    return SMAFA_OK;
}

// handle, out (then *out = NULL), n_kept (then *n_kept = 0), keep unless the store is empty, the store's size
static int subset_args(const char *who, const smafa_db *db, smafa_db **out, uint64_t *n_kept, const void *keep) {
    if (!db) return missing(who, "handle");
    if (!out) return missing(who, "out");
    *out = nullptr;
    if (!n_kept) return missing(who, "n_kept");
    *n_kept = 0;
    if (!keep && db->n) return missing(who, "keep");
    if (db->n >= (1ull << 31))  // (the device scan counts its items in an int)
        return set_error(SMAFA_ERR_INVALID, "%s: a subset takes stores of fewer than 2^31 rows (this one: %llu)", who, (unsigned long long)db->n);
    return SMAFA_OK;
}

// ---- rows
// inv[source column][stored code] -> source code, the inverse of tab[]: built once per layout, on the host
static int inverse_table(smafa_db *db) {
    if (db->d_inv.p) return SMAFA_OK;
    const uint32_t lim = db->alphabet == SMAFA_ALPHABET_AA ? 28u : 5u;
    std::vector<uint8_t> inv((size_t)db->L * 32u, 0xff);
    for (uint32_t c = 0; c < db->L; c++)
        for (uint32_t code = 0; code < lim; code++) inv[(size_t)c * 32u + (db->tab[(size_t)c * 32u + code] & 31u)] = (uint8_t)code;
    RC_TRY(db->d_inv.ensure(inv.size()));
    const hipError_t e = hipMemcpy(db->d_inv.p, inv.data(), inv.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        db->d_inv.release();
        return set_error(SMAFA_ERR_DEVICE, "uploading the inverse code table failed: %s", hipGetErrorString(e));
    }
    return SMAFA_OK;
}

// d_subjects: m uint32 on the device, or nullptr: first .. first + m - 1 (checked by the caller); d_codes: m x L bytes.  m > 0.
static int store_rows(smafa_db *db, const char *who, const uint32_t *d_subjects, uint64_t first, uint64_t m, uint8_t *d_codes) {
    if (db->n >= (1ull << 32) || m > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "%s: too many rows in one call", who);
    if (db->L > subset::kUnpackMaxColumns)
        return set_error(SMAFA_ERR_INVALID, "%s: rows of up to %u columns (this store: %u)", who, subset::kUnpackMaxColumns, db->L);
    RC_TRY(subset_call_begin(db));
    if (db->n == 0) {  // (the launch form's list may name anything: every row is absent)
        HIP_TRY(hipMemsetAsync(d_codes, 0xff, m * db->L, db->stream));
        return subset_call_end(db);
    }
    RC_TRY(inverse_table(db));
    JoinCall c{db};
    RC_TRY(join_positions(c));  // pos_of[], valid for the store as it is now, as the join keeps it
    if (c.inverted) note_call_kernel(db, "smafa_join::inverse_order_kernel");
    const uint32_t lds_rows = std::min<uint32_t>(64u, std::max<uint32_t>(1u, subset::kUnpackLdsPerWave / db->L));
    const size_t lds_bytes = subset::kUnpackWaves * (((size_t)lds_rows * db->L + 15u) & ~(size_t)15u);
    const dim3 grid((uint32_t)(((m + 63u) / 64u + subset::kUnpackWaves - 1u) / subset::kUnpackWaves)), block(subset::kUnpackWaves * 64u);
    const auto by_planes = [&](auto planes_c) {
        constexpr int PS = decltype(planes_c)::value;
        hipLaunchKernelGGL(subset::unpack_rows_kernel<PS>, grid, block, lds_bytes, db->stream, db->d_planes, db->join.pos_of.as<uint32_t>(), d_subjects,
                           first, m, (uint32_t)db->n, db->L, db->W, db->d_perm.as<uint32_t>(), db->d_inv.as<uint8_t>(), lds_rows, d_codes);
        char name[64];
        snprintf(name, sizeof name, "subset::unpack_rows_kernel<%d>", PS);
        note_call_kernel(db, name);
    };
    if (db->P == 5) by_planes(ic<5>{});
    else if (db->P == 3) by_planes(ic<3>{});
    else by_planes(ic<2>{});
    HIP_TRY(hipGetLastError());
    db->call_launches++;
    RC_TRY(subset_call_end(db));
    log_line(2, "%llu rows of %u columns unpacked on the device in %.3f ms", (unsigned long long)m, db->L, db->call_ms);
    return SMAFA_OK;
}

// handle, codes unless m is 0, the range where no list is given
static int rows_args(const char *who, const smafa_db *db, bool listed, uint64_t first, uint64_t m, const void *codes) {
    if (!db) return missing(who, "handle");
    if (m == 0) return SMAFA_OK;
    if (!codes) return missing(who, "codes");
    if (!listed && (first > db->n || m > db->n - first))
        return set_error(SMAFA_ERR_INVALID, "%s: rows %llu .. %llu, the store has %llu subjects", who, (unsigned long long)first,
                         (unsigned long long)(first + m - 1), (unsigned long long)db->n);
    return SMAFA_OK;
}

}  // extern "C++"

int smafa_db_subset_launch(smafa_db *db, const void *d_keep, int invert, smafa_db **out, void *d_old_of_new, uint64_t *n_kept) try {
    const char *const who = "smafa_db_subset_launch";
    RC_TRY(subset_args(who, db, out, n_kept, d_keep));
    return subset_store(db, who, (const uint32_t *)d_keep, invert, out, (uint32_t *)d_old_of_new, ~0ull, n_kept);
} catch (...) {
    return smafa::exception_code("smafa_db_subset_launch");
}

int smafa_db_subset(smafa_db *db, const uint32_t *keep, int invert, smafa_db **out, uint32_t *old_of_new, uint64_t cap, uint64_t *n_kept) try {
    const char *const who = "smafa_db_subset";
    RC_TRY(subset_args(who, db, out, n_kept, keep));
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t n = db->n;
    // keep[] on its way in, old_of_new[] behind it on its way out
    RC_TRY(h.stage(std::max<uint64_t>(2u * n * sizeof(uint32_t), 1), 0));
    uint32_t *const d_keep = J.out.as<uint32_t>(), *const d_old = d_keep + n;
    if (n) HIP_TRY(hipMemcpyAsync(d_keep, keep, n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    smafa_db *sub = nullptr;
    RC_TRY(subset_store(db, who, n ? d_keep : nullptr, invert, &sub, old_of_new ? d_old : nullptr, cap, n_kept));
    int rc = h.fetch(old_of_new, d_old, *n_kept * sizeof(uint32_t));
    if (!rc) rc = h.wait();
    if (rc) {
        smafa_db_destroy(sub);
        return rc;
    }
    trim({&J.out});
    *out = sub;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_subset");
}

int smafa_db_rows_launch(smafa_db *db, const void *d_subjects, uint64_t first, uint64_t m, void *d_codes) try {
    const char *const who = "smafa_db_rows_launch";
    RC_TRY(rows_args(who, db, d_subjects, first, m, d_codes));
    if (m == 0) return SMAFA_OK;
    return store_rows(db, who, (const uint32_t *)d_subjects, first, m, (uint8_t *)d_codes);
} catch (...) {
    return smafa::exception_code("smafa_db_rows_launch");
}

int smafa_db_rows(smafa_db *db, const uint32_t *subjects, uint64_t first, uint64_t m, uint8_t *codes) try {
    const char *const who = "smafa_db_rows";
    RC_TRY(rows_args(who, db, subjects, first, m, codes));
    if (m == 0) return SMAFA_OK;
    if (subjects)
        for (uint64_t j = 0; j < m; j++)
            if (subjects[j] >= db->n)
                return set_error(SMAFA_ERR_INVALID, "%s: subjects[%llu] is %u, the store has %llu subjects", who, (unsigned long long)j, subjects[j],
                                 (unsigned long long)db->n);
    const HostForm h{db};
    auto &J = db->join;
    const uint64_t list_bytes = subjects ? (m * sizeof(uint32_t) + 15u) / 16u * 16u : 0u;
    RC_TRY(h.stage(list_bytes + m * db->L, 0));
    uint32_t *const d_subjects = J.out.as<uint32_t>();
    uint8_t *const d_codes = J.out.as<uint8_t>() + list_bytes;
    if (subjects) HIP_TRY(hipMemcpyAsync(d_subjects, subjects, m * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    RC_TRY(store_rows(db, who, subjects ? d_subjects : nullptr, first, m, d_codes));
    RC_TRY(h.fetch(codes, d_codes, m * db->L));
    RC_TRY(h.wait());
    trim({&J.out});
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_rows");
}

// cluster.cpp — cluster (the reference's src/cluster.rs:13-94): the batched, exact restatement of the reference's greedy
// loop, on one device (smafa_cluster), one rank of several processes (smafa_cluster_sharded) or several devices of one
// process (smafa_cluster_multi).  Prints "{raw record}\t{centroid string}\n" (src/cluster.rs:79-84).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "cluster_batch.h"
#include "drivers.h"

using namespace smafa;

namespace {

// First occurrences of every distinct row, in input order — the HashSet<Vec<u64>> test of src/cluster.rs:24,46-48.
// Rows are hashed by all threads, then thread t owns the rows whose hash falls in partition t and runs them, in input
// order, through its own open-addressing table; "first" is decided inside one partition, so the result does not
// depend on the number of threads.
inline uint64_t row_hash(const uint8_t *p, uint32_t L) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    uint32_t i = 0;
    for (; i + 8 <= L; i += 8) {
        uint64_t v;
        memcpy(&v, p + i, 8);
        h = (h ^ v) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    for (; i < L; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h ^ (h >> 29);
}

void first_occurrences(const uint8_t *rows, uint64_t n, uint32_t L, std::vector<uint32_t> &uniq) {
    const unsigned T = n >= (1u << 18) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    std::vector<uint64_t> hash(n);
    std::vector<uint8_t> first(n, 0);
    auto run = [&](auto &&fn) {
        if (T == 1) return fn(0u);
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < T; t++) pool.emplace_back(fn, t);
        for (auto &th : pool) th.join();
    };
    run([&](unsigned t) {
        for (uint64_t i = n * t / T, e = n * (t + 1) / T; i < e; i++) hash[i] = row_hash(rows + i * L, L);
    });
    run([&](unsigned t) {
        auto mine = [&](uint64_t h) { return (unsigned)((h >> 40) % T) == t; };  // slot bits come from the low end
        size_t count = 0;
        for (uint64_t i = 0; i < n; i++) count += mine(hash[i]);
        size_t cap = 16;
        while (cap < count * 2) cap *= 2;
        std::vector<uint32_t> slots(cap, UINT32_MAX);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t h = hash[i];
            if (!mine(h)) continue;
            size_t s = h & (cap - 1);
            bool seen = false;
            while (slots[s] != UINT32_MAX) {
                const uint32_t j = slots[s];
                if (hash[j] == h && memcmp(rows + (size_t)j * L, rows + i * L, L) == 0) {
                    seen = true;
                    break;
                }
                s = (s + 1) & (cap - 1);
            }
            if (!seen) {
                slots[s] = (uint32_t)i;
                first[i] = 1;
            }
        }
    });
    uniq.clear();
    for (uint64_t i = 0; i < n; i++)
        if (first[i]) uniq.push_back((uint32_t)i);
}

// ------------------------------------------------------------------------------------ cluster
//
// The reference handles one record at a time: skip exact duplicates, scan the record against the
// centroids found so far, join the nearest one if it is within max_divergence (ties: lowest centroid
// index), else become a new centroid (src/cluster.rs:35-85).  The same assignment is computed here in
// batches of B unseen records:
//   1. one GPU scan of the batch against the centroids known BEFORE the batch (bound: max_divergence,
//      tightened to each record's minimum) -> per record its nearest old centroid, lowest index on ties;
//   2. records with no old centroid in range are the only ones that can become centroids in this batch
//      ("candidates"); one GPU scan of the batch against the candidates gives every in-range
//      (record, candidate) pair;
//   3. a sequential pass in input order decides, for each record, between its old centroid and the
//      candidates EARLIER in the batch that did become centroids — old centroids have smaller indices
//      than new ones, and new ones are numbered in input order, so "smallest distance, then lowest
//      centroid index" is evaluated exactly as the reference's first-minimum scan (src/cluster.rs:62-68).
// Nothing is approximated: the result is the reference's, record for record.
//
// Sharded over `world` processes (one GPU each, smafa_cluster_sharded): steps 1 and 2 scan only this rank's
// contiguous slice of the batch, the slices' results are exchanged through the caller's allgather, and step 3
// runs identically on every rank, so the replicas of the centroid store stay equal without a broadcast.
// Step 3, the slice rule and the batch-size rule are pure functions in host/cluster_batch.h.

// the input of a clustering run, parsed and de-duplicated ONCE (every rank of a sharded run works from the same records)
struct ClusterInput {
    BulkRecords recs;
    std::vector<uint32_t> uniq;  // first occurrences, input order (src/cluster.rs:46-48)
    int pending = SMAFA_OK;      // the record that stopped the load fails AFTER the lines of the records before it are written
    std::string pending_msg;
    double t_start = 0;
};

int cluster_load(const char *input_fasta, int alphabet, int device, ClusterInput &in) {
    if (!input_fasta) return set_error(SMAFA_ERR_INVALID, "smafa_cluster: NULL path");
    if (alphabet != SMAFA_ALPHABET_NT && alphabet != SMAFA_ALPHABET_AA)
        return set_error(SMAFA_ERR_INVALID, "unknown alphabet %d", alphabet);
    in.t_start = now_seconds();
    log_line(1, "Clustering ..");  // src/cluster.rs:33
    // device bring-up overlaps the parse; it is waited for after the duplicates have been found too (they need no device)
    WarmDevices warm(device);
    BulkRecords &recs = in.recs;
    int rc = load_records_bulk(input_fasta, alphabet, true, recs);  // src/cluster.rs:28,35-43 for every record
    if (rc) return expect_fastx(rc, "valid path/file of input fasta");  // src/cluster.rs:28
    if (recs.n >= 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "too many records");
    in.pending = pending_panic(recs, "input", recs.L, in.pending_msg);  // src/cluster.rs:39 for a record that does not parse
    const double t_loaded = now_seconds();
    if (recs.n > 0) {
        in.uniq.reserve(recs.n);
        first_occurrences(recs.codes.data(), recs.n, (uint32_t)recs.L, in.uniq);  // src/cluster.rs:46-48
        log_line(2, "parsed %llu records in %.2f s, %zu distinct found in %.2f s", (unsigned long long)recs.n,
                 t_loaded - in.t_start, in.uniq.size(), now_seconds() - t_loaded);
    }
    const double t_wait = now_seconds();
    warm.join();
    log_line(2, "device bring-up: waited %.2f s for it after the load (%.2f s since the start)", now_seconds() - t_wait,
             now_seconds() - in.t_start);
    return SMAFA_OK;
}

// ---- output stage, overlapped with the scans (src/cluster.rs:79-84).  A record's line is final as soon as the batch
// that holds it is resolved (records are resolved in input order; duplicates print nothing), so rank 0 formats and
// writes the lines of finished batches on a writer thread while the next batches scan.  Every line is
// "raw record \t centroid string \n" = 2L + 2 bytes; blocks of lines are formatted by all threads and written in order.
class ClusterWriter {
  public:
    // centroid_of, centroid_rec: the run's two maps, read here while cluster_run fills them (see the reserve there)
    ClusterWriter(const ClusterInput &in, int alphabet, int out_fd, const std::vector<uint32_t> &centroid_of,
                  const std::vector<uint32_t> &centroid_rec)
        : recs(in.recs), L(in.recs.L), out_fd(out_fd), centroid_of(centroid_of), centroid_rec(centroid_rec) {
        for (int c = 0; c < 32; c++) letters[c] = letter_of(alphabet, (uint8_t)c);
    }
    void start() {  // (rank 0 only: without a thread publish() and finish() have nobody to tell)
        writer = std::thread([this]() noexcept { run(); });
    }
    void publish(uint64_t upto) {
        {
            std::lock_guard<std::mutex> lock(m);
            final_upto = upto;
        }
        cv.notify_all();
    }
    // the writer finishes the lines of the last batches: -> the write status, its text in smafa_last_error()
    int finish() {
        if (!writer.joinable()) return SMAFA_OK;
        const double t_out = now_seconds();
        publish(recs.n);
        writer.join();
        if (write_rc) return set_error(write_rc, "%s", write_msg.c_str());
        log_line(2, "%zu lines written in %.2f s (%.2f s of formatting + writing overlapped with the scans, %.2f s after the last batch)",
                 lines_written, t_write_busy, t_write_busy - std::min(t_write_busy, now_seconds() - t_out), now_seconds() - t_out);
        return SMAFA_OK;
    }
    ~ClusterWriter() {  // whatever way the run is left: the writer is told to stop and joined
        if (!writer.joinable()) return;
        {
            std::lock_guard<std::mutex> lock(m);
            stop = true;
        }
        cv.notify_all();
        writer.join();
    }

  private:
    const BulkRecords &recs;
    const size_t L;
    const int out_fd;
    const std::vector<uint32_t> &centroid_of, &centroid_rec;
    char letters[32];
    std::mutex m;
    std::condition_variable cv;
    uint64_t final_upto = 0;  // records [0, final_upto) have their final centroid_of / centroid_rec entries
    bool stop = false;        // the main loop failed: write nothing more
    std::thread writer;
    int write_rc = SMAFA_OK;
    std::string write_msg;
    size_t lines_written = 0;
    double t_write_busy = 0.0;
    std::vector<char> text;
    std::vector<uint32_t> lines;

    void run() noexcept {
        try {
            const uint64_t n = recs.n, block_records = 1u << 20;
            uint64_t done = 0;
            while (done < n) {
                uint64_t upto;
                {
                    std::unique_lock<std::mutex> lock(m);
                    cv.wait(lock, [&] { return stop || final_upto > done; });
                    if (stop) return;
                    upto = std::min<uint64_t>(final_upto, done + block_records);
                }
                const double t0 = now_seconds();
                write_rc = write_block(done, upto);
                if (write_rc) {
                    write_msg = smafa_last_error();
                    return;
                }
                done = upto;
                t_write_busy += now_seconds() - t0;
            }
        } catch (...) {
            write_rc = smafa::exception_code("the cluster output thread");
            try {
                write_msg = smafa_last_error();
            } catch (...) {
            }
        }
    }
    // the lines of records [done, upto), formatted and written
    int write_block(uint64_t done, uint64_t upto) {
        const size_t line_bytes = 2 * L + 2;
        const unsigned T = recs.n >= (1u << 16) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
        lines.clear();
        for (uint64_t i = done; i < upto; i++)
            if (centroid_of[i] != UINT32_MAX) lines.push_back((uint32_t)i);
        const size_t nk = lines.size();
        if (text.size() < nk * line_bytes) text.resize(nk * line_bytes);
        auto fill = [&](unsigned t, unsigned of) {
            for (size_t k = nk * t / of, e = nk * (t + 1) / of; k < e; k++) {
                const uint32_t i = lines[k];
                char *o = &text[k * line_bytes];
                memcpy(o, &recs.raw[(size_t)i * L], L);
                o[L] = '\t';
                const uint8_t *c = &recs.codes[(size_t)centroid_rec[centroid_of[i]] * L];
                for (size_t j = 0; j < L; j++) o[L + 1 + j] = letters[c[j] & 31];
                o[2 * L + 1] = '\n';
            }
        };
        const unsigned use = nk >= (1u << 14) ? T : 1u;
        if (use == 1) {
            fill(0, 1);
        } else {
            std::vector<std::thread> pool;
            pool.reserve(use);
            for (unsigned t = 0; t < use; t++) pool.emplace_back(fill, t, use);
            for (auto &th : pool) th.join();
        }
        lines_written += nk;
        return nk ? write_all(out_fd, text.data(), nk * line_bytes) : (int)SMAFA_OK;
    }
};

// what one rank of a run works with: its device, the run's parameters and its way to the other ranks
struct ClusterRank {
    int device, alphabet;
    uint32_t max_divergence;
    size_t L;
    uint32_t rank, world;
    smafa_allgather_fn allgather;
    void *ctx;
};

// one batch of unseen records through its two scans; the vectors keep their memory from batch to batch
struct ClusterBatch {
    size_t nb = 0, s_lo = 0, ns = 0;  // records; this rank's slice of them, [s_lo, s_lo + ns)
    std::vector<uint8_t> codes, cand_codes;
    std::vector<smafa_hit> old_hits, cand_hits;
    std::vector<uint32_t> old_d, old_c;  // record -> its nearest old centroid (UINT32_MAX: none in range)
    std::vector<uint32_t> cand_pos;      // candidate ordinal -> position in the batch
};

struct StageTimes {
    size_t batches = 0;
    double old = 0, cand = 0, seq = 0, append = 0;
};

// One allgather of a sharded run: `bytes` at `send` from this rank, every rank's bytes in rank order back at *all.  They must
// add up to `expect` bytes — or, with kWholeRows, to whole rows.
constexpr uint64_t kWholeRows = UINT64_MAX;
int exchange(const ClusterRank &r, const void *send, uint64_t bytes, const char *what, uint64_t expect, const void **all,
             uint64_t *all_bytes) {
    if (r.allgather(r.ctx, send, bytes, all, all_bytes) != 0) return set_error(SMAFA_ERR_IO, "allgather failed (%s)", what);
    if (expect == kWholeRows) {
        if (*all_bytes % sizeof(smafa_hit) || (*all_bytes && !*all))
            return set_error(SMAFA_ERR_INVALID, "allgather returned %llu bytes, not whole rows", (unsigned long long)*all_bytes);
    } else if (*all_bytes != expect || (expect && !*all)) {
        return set_error(SMAFA_ERR_INVALID, "allgather returned %llu bytes, expected %zu", (unsigned long long)*all_bytes,
                         (size_t)expect);
    }
    return SMAFA_OK;
}

// 1. nearest old centroid per record: rows ordered (record, distance, centroid), minimum only
int scan_old(const ClusterRank &r, smafa_db *centroids, bool any_centroids, ClusterBatch &bt) {
    const size_t nb = bt.nb, s_lo = bt.s_lo, ns = bt.ns;
    bt.old_hits.clear();
    if (any_centroids && ns) {
        const int rc = scan_to_host(centroids, bt.codes.data() + s_lo * r.L, ns, r.max_divergence, 1, bt.old_hits);
        if (rc) return rc;
    }
    bt.old_d.assign(nb, UINT32_MAX);
    bt.old_c.assign(nb, UINT32_MAX);
    for (size_t t = bt.old_hits.size(); t-- > 0;) {  // backwards: the first row of each record wins
        bt.old_d[s_lo + bt.old_hits[t].query] = bt.old_hits[t].dist;
        bt.old_c[s_lo + bt.old_hits[t].query] = bt.old_hits[t].subject;
    }
    if (r.world > 1) {  // exchange (distance, centroid) of every record: nb x 8 bytes
        std::vector<uint32_t> mine(2 * ns);
        for (size_t b = 0; b < ns; b++) {
            mine[2 * b] = bt.old_d[s_lo + b];
            mine[2 * b + 1] = bt.old_c[s_lo + b];
        }
        const void *all = nullptr;
        uint64_t all_bytes = 0;
        const int rc = exchange(r, mine.data(), mine.size() * 4, "nearest old centroids", nb * 8, &all, &all_bytes);
        if (rc) return rc;
        const uint32_t *w = (const uint32_t *)all;
        for (size_t b = 0; b < nb; b++) {
            bt.old_d[b] = w[2 * b];
            bt.old_c[b] = w[2 * b + 1];
        }
    }
    return SMAFA_OK;
}

// 2. candidates = records with no old centroid in range; every (record, candidate) pair in range, ordered (record, distance,
// candidate), the record as its position in the batch
int scan_candidates(const ClusterRank &r, DbGuard &cand, ClusterBatch &bt) {
    const size_t L = r.L;
    bt.cand_pos.clear();
    bt.cand_codes.clear();
    for (size_t b = 0; b < bt.nb; b++)
        if (bt.old_c[b] == UINT32_MAX) {
            bt.cand_pos.push_back((uint32_t)b);
            bt.cand_codes.insert(bt.cand_codes.end(), &bt.codes[b * L], &bt.codes[b * L] + L);
        }
    std::vector<smafa_hit> &cand_hits = bt.cand_hits;
    cand_hits.clear();
    if (bt.cand_pos.empty()) return SMAFA_OK;
    int rc = SMAFA_OK;
    if (!cand.db) rc = smafa_db_create(&cand.db, r.device, r.alphabet, (uint32_t)L);  // one handle for every batch: its device buffers are reused
    if (!rc) rc = db_clear(cand.db);
    if (!rc) rc = smafa_db_append(cand.db, bt.cand_codes.data(), bt.cand_pos.size());
    if (!rc && bt.ns) rc = scan_to_host(cand.db, bt.codes.data() + bt.s_lo * L, bt.ns, r.max_divergence, SMAFA_NONE, cand_hits);
    if (rc) return rc;
    for (smafa_hit &hrow : cand_hits) hrow.query += (uint32_t)bt.s_lo;  // position in the batch
    if (r.world > 1) {  // rows of slice r precede rows of slice r+1: the concatenation stays ordered
        const void *all = nullptr;
        uint64_t all_bytes = 0;
        rc = exchange(r, cand_hits.data(), cand_hits.size() * sizeof(smafa_hit), "candidate rows", kWholeRows, &all, &all_bytes);
        if (rc) return rc;
        const smafa_hit *rows = (const smafa_hit *)all;
        cand_hits.assign(rows, rows + all_bytes / sizeof(smafa_hit));
        for (const smafa_hit &hrow : cand_hits)
            if (hrow.query >= bt.nb || hrow.subject >= bt.cand_pos.size())
                return set_error(SMAFA_ERR_INVALID, "allgather returned a row outside the batch");
    }
    return SMAFA_OK;
}

// where the time of the batches went, and where this rank's launches did
void log_stages(const ClusterRank &r, const StageTimes &t, smafa_db *centroids, smafa_db *cand) {
    log_line(2, "%zu batches: scans vs old centroids %.2f s, candidate scans %.2f s, sequential pass %.2f s, "
                "centroid appends %.2f s", t.batches, t.old, t.cand, t.seq, t.append);
    double ms_a = 0, ms_b = 0;
    uint64_t la = 0, lb = 0;
    db_life_stats(centroids, &ms_a, &la);
    db_life_stats(cand, &ms_b, &lb);
    log_line(2, "scan kernels %.1f ms over %llu launches (vs old centroids %.1f ms, vs candidates %.1f ms)", ms_a + ms_b,
             (unsigned long long)(la + lb), ms_a, ms_b);
    // where this rank's launches really went (a multi-device run must not end up with every replica on device 0)
    int at = -1, at_c = -1;
    uint64_t off = 0, off_c = 0;
    smafa_launch_device(centroids, &at, &off);
    if (cand) smafa_launch_device(cand, &at_c, &off_c);
    log_line(2, "rank %u of %u: handle on device %d, scan launches issued with device %d current, %llu off the handle's device",
             r.rank, r.world, r.device, at, (unsigned long long)(off + off_c));
}

int cluster_run(const ClusterInput &in, uint32_t max_divergence, int out_fd, int device, int alphabet, uint32_t rank,
                uint32_t world, smafa_allgather_fn allgather, void *ctx) {
    if (world == 0 || rank >= world) return set_error(SMAFA_ERR_INVALID, "rank %u outside world of %u", rank, world);
    if (world > 1 && !allgather) return set_error(SMAFA_ERR_INVALID, "smafa_cluster_sharded: NULL allgather");
    const std::vector<uint8_t> &codes = in.recs.codes;
    const std::vector<uint32_t> &uniq = in.uniq;
    const uint64_t n = in.recs.n;
    const size_t L = in.recs.L;
    if (n > 0) {
        const ClusterRank r{device, alphabet, max_divergence, L, rank, world, allgather, ctx};
        std::vector<uint32_t> centroid_of(n, UINT32_MAX);  // record -> centroid ordinal
        std::vector<uint32_t> centroid_rec;                // centroid ordinal -> record
        // The writer reads both maps while the loop below fills them, and no lock covers their entries: centroid_rec is
        // reserved once, here, and never reallocated, and a batch is published only after its entries of both are written.
        centroid_rec.reserve(uniq.size());
        DbGuard centroids, cand;
        int rc = smafa_db_create(&centroids.db, device, alphabet, (uint32_t)L);
        if (rc) return rc;
        ClusterWriter writer(in, alphabet, out_fd, centroid_of, centroid_rec);
        if (rank == 0) writer.start();

        ClusterBatch bt;
        std::vector<uint32_t> centroid, became;  // resolve_batch's answer: batch position -> centroid, the new centroids
        std::vector<uint8_t> new_codes;
        StageTimes t;
        size_t pos = 0, B = 1024;
        // largest batch: a batch costs two scans + an append whatever its size (~2 ms of host round trips), the scans themselves
        // grow with it; SMAFA_CLUSTER_BATCH overrides (every rank reads the same environment)
        size_t batch_cap = 65536;
        if (const char *bc = getenv("SMAFA_CLUSTER_BATCH")) batch_cap = std::max<size_t>(256, strtoull(bc, nullptr, 10));
        while (pos < uniq.size()) {
            t.batches++;
            double t0 = now_seconds();
            const size_t nb = bt.nb = std::min(B, uniq.size() - pos);
            bt.codes.resize(nb * L);
            for (size_t b = 0; b < nb; b++) memcpy(&bt.codes[b * L], &codes[(size_t)uniq[pos + b] * L], L);
            bt.s_lo = slice_start(nb, rank, world);
            bt.ns = slice_start(nb, rank + 1, world) - bt.s_lo;
            rc = scan_old(r, centroids.db, !centroid_rec.empty(), bt);
            if (rc) return rc;
            t.old += now_seconds() - t0;
            t0 = now_seconds();
            rc = scan_candidates(r, cand, bt);
            if (rc) return rc;
            t.cand += now_seconds() - t0;
            t0 = now_seconds();
            // 3. sequential pass in input order (host/cluster_batch.h), and its answer applied
            resolve_batch(nb, bt.old_d.data(), bt.old_c.data(), bt.cand_pos, bt.cand_hits.data(), bt.cand_hits.size(),
                          max_divergence, (uint32_t)centroid_rec.size(), centroid, became);
            for (size_t b = 0; b < nb; b++) centroid_of[uniq[pos + b]] = centroid[b];
            new_codes.clear();
            for (const uint32_t b : became) {
                centroid_rec.push_back(uniq[pos + b]);
                new_codes.insert(new_codes.end(), &bt.codes[b * L], &bt.codes[b * L] + L);
            }
            t.seq += now_seconds() - t0;
            t0 = now_seconds();
            if (!became.empty()) {
                rc = smafa_db_append(centroids.db, new_codes.data(), became.size());
                if (rc) return rc;
            }
            t.append += now_seconds() - t0;
            pos += nb;
            // every record in front of the next unseen one is final now (the records between two first occurrences are duplicates)
            writer.publish(pos < uniq.size() ? uniq[pos] : n);
            B = next_batch_size(B, batch_cap, nb, bt.cand_pos.size(), bt.cand_hits.size());
        }
        log_stages(r, t, centroids.db, cand.db);
        rc = writer.finish();
        if (rc) return rc;
        log_line(2, "cluster: %.3f s from the start of the load to the last line", now_seconds() - in.t_start);
        log_line(1, "Clustering complete, took %llu seconds. Clustered %llu sequences into %zu clusters.",  // src/cluster.rs:87-92
                 (unsigned long long)(now_seconds() - in.t_start), (unsigned long long)n, centroid_rec.size());
    }
    if (in.pending != SMAFA_OK) return set_error(in.pending, "%s", in.pending_msg.c_str());
    return SMAFA_OK;
}

}  // namespace

extern "C" {

int smafa_cluster(const char *input_fasta, uint32_t max_divergence, int out_fd, int device, int alphabet) try {
    ClusterInput in;
    int rc = cluster_load(input_fasta, alphabet, device, in);
    if (rc) return rc;
    return cluster_run(in, max_divergence, out_fd, device, alphabet, 0, 1, nullptr, nullptr);
} catch (...) {
    return smafa::exception_code("smafa_cluster");
}

int smafa_cluster_sharded(const char *input_fasta, uint32_t max_divergence, int out_fd, int device, int alphabet,
                          uint32_t rank, uint32_t world, smafa_allgather_fn allgather, void *ctx) try {
    if (world == 0 || rank >= world) return set_error(SMAFA_ERR_INVALID, "rank %u outside world of %u", rank, world);
    if (world > 1 && !allgather) return set_error(SMAFA_ERR_INVALID, "smafa_cluster_sharded: NULL allgather");
    ClusterInput in;
    int rc = cluster_load(input_fasta, alphabet, device, in);
    if (rc) return rc;
    return cluster_run(in, max_divergence, out_fd, device, alphabet, rank, world, allgather, ctx);
} catch (...) {
    return smafa::exception_code("smafa_cluster_sharded");
}

// ---- the same clustering over several GPUs of one node by ONE process: one host thread per entry of `devices` plays a
// rank of smafa_cluster_sharded (its own replica of the centroid store on its own device, its slice of every batch), the
// input is parsed and de-duplicated once for all of them, and the two exchanges per batch go through memory.
namespace {
struct ThreadExchange {
    std::mutex m;
    std::condition_variable cv;
    uint32_t world = 0, arrived = 0;
    uint64_t round = 0;
    bool failed = false;
    std::vector<std::vector<uint8_t>> parts;
    std::vector<uint8_t> all[2];  // the result of round r lives in all[r & 1] until round r + 2 overwrites it
};
struct ThreadRank {
    ThreadExchange *ex;
    uint32_t rank;
};
int thread_allgather(void *ctx, const void *send, uint64_t send_bytes, const void **recv, uint64_t *recv_bytes) {
    ThreadRank *me = (ThreadRank *)ctx;
    ThreadExchange &ex = *me->ex;
    std::unique_lock<std::mutex> lock(ex.m);
    if (ex.failed) return 1;
    ex.parts[me->rank].assign((const uint8_t *)send, (const uint8_t *)send + send_bytes);
    const uint64_t my_round = ex.round;
    if (++ex.arrived == ex.world) {
        std::vector<uint8_t> &out = ex.all[my_round & 1];
        out.clear();
        for (const auto &p : ex.parts) out.insert(out.end(), p.begin(), p.end());
        ex.arrived = 0;
        ex.round++;
        ex.cv.notify_all();
    } else {
        ex.cv.wait(lock, [&] { return ex.round != my_round || ex.failed; });
        if (ex.round == my_round) return 1;  // somebody failed before the round completed
    }
    *recv = ex.all[my_round & 1].empty() ? nullptr : ex.all[my_round & 1].data();
    *recv_bytes = ex.all[my_round & 1].size();
    return 0;
}
}  // namespace

int smafa_cluster_multi(const char *input_fasta, uint32_t max_divergence, int out_fd, const int *devices, int ndev, int alphabet) try {
    if (!devices || ndev < 1 || ndev > 64) return set_error(SMAFA_ERR_INVALID, "smafa_cluster_multi: 1 to 64 devices expected");
    ClusterInput in;
    int rc = cluster_load(input_fasta, alphabet, devices[0], in);
    if (rc) return rc;
    if (ndev == 1) return cluster_run(in, max_divergence, out_fd, devices[0], alphabet, 0, 1, nullptr, nullptr);
    ThreadExchange ex;
    ex.world = (uint32_t)ndev;
    ex.parts.resize((size_t)ndev);
    std::vector<int> rcs((size_t)ndev, SMAFA_OK);
    std::vector<std::string> msgs((size_t)ndev);
    std::vector<ThreadRank> ranks((size_t)ndev);
    std::vector<std::thread> pool;
    auto leave = [&] {  // nobody waits for a rank that has left
        std::lock_guard<std::mutex> lock(ex.m);
        ex.failed = true;
        ex.cv.notify_all();
    };
    int start_rc = SMAFA_OK;
    try {
        pool.reserve((size_t)ndev);
        for (int r = 0; r < ndev; r++) {
            ranks[r] = {&ex, (uint32_t)r};
            pool.emplace_back([&, r]() noexcept {
                try {
                    rcs[r] = cluster_run(in, max_divergence, out_fd, devices[r], alphabet, (uint32_t)r, (uint32_t)ndev, thread_allgather, &ranks[r]);
                } catch (...) {  // no exception ends a rank's thread (std::terminate): it becomes the rank's error code
                    rcs[r] = smafa::exception_code("a cluster rank's thread");
                }
                if (rcs[r]) {
                    try {
                        msgs[r] = smafa_last_error();  // the text is per thread
                    } catch (...) {
                    }
                    leave();
                }
            });
        }
    } catch (...) {  // a thread could not be started: the ranks already running must not wait for it, and are joined
        start_rc = smafa::exception_code("starting a cluster rank's thread");
        leave();
    }
    for (auto &th : pool) th.join();
    if (start_rc) return start_rc;
    // every rank reports the same input-borne failure; a rank-local one (a device) is the first one's to tell
    for (int r = 0; r < ndev; r++)
        if (rcs[r] && msgs[r].find("allgather failed") == std::string::npos) return set_error(rcs[r], "%s", msgs[r].c_str());
    for (int r = 0; r < ndev; r++)
        if (rcs[r]) return set_error(rcs[r], "%s", msgs[r].c_str());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_cluster_multi");
}

}  // extern "C"

// drivers.cpp — the reference crate's public functions over the HIP scan engine:
//   makedb  (/root/reference/src/lib.rs:137-165)   host only
//   query   (/root/reference/src/lib.rs:198-325)   scan on the GPU, selection + TSV on the host
//   cluster (/root/reference/src/cluster.rs:13-94) batched, exact restatement of the greedy loop: host/cluster.cpp
//   count   (/root/reference/src/lib.rs:378-398)   host only
// and what they share with host/cluster.cpp and the store verbs of host/store_verbs.cpp (host/drivers.h).
// Output bytes are the reference's: `query` prints "{query}\t{subject}\t{distance}\t{subject string}\n"
// (src/lib.rs:292,310), `cluster` prints "{raw record}\t{centroid string}\n" (src/cluster.rs:79-84).
// Inputs the reference panics on fail with SMAFA_ERR_PANIC and the same message, after the rows the
// reference would already have printed.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "drivers.h"
#include "packed.h"

namespace smafa {

int write_all(int fd, const char *p, size_t n) {
    while (n) {
        const ssize_t w = ::write(fd, p, n);
        if (w < 0) {
            if (errno == EINTR) continue;
            return set_error(SMAFA_ERR_IO, "write failed: %s", strerror(errno));
        }
        p += w;
        n -= (size_t)w;
    }
    return SMAFA_OK;
}

void append_u32(std::string &s, uint32_t v) {
    char tmp[12];
    int n = 0;
    do {
        tmp[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) s.push_back(tmp[--n]);
}

bool db_file_is_packed(const char *db_path) {
    uint8_t head[8] = {0};
    FILE *f = fopen(db_path, "rb");
    if (!f) return false;
    const size_t got = fread(head, 1, sizeof head, f);
    fclose(f);
    return is_packed_file(head, got);
}

std::string length_panic_text(size_t len, size_t store_len) {
    char msg[160];
    snprintf(msg, sizeof msg, "Cannot compute distances between seq of length %zu and windows of lengths %zu", len, store_len);
    return msg;
}

int pending_panic(const BulkRecords &recs, const char *noun, size_t store_len, std::string &msg) {
    switch (recs.err_kind) {
        case 1: msg = recs.err_msg; break;  // src/lib.rs:38-41
        case 2: msg = length_panic_text(recs.err_len, store_len); break;
        case 3: msg = "Cannot add empty sequence to WindowSet"; break;
        case 4: msg = std::string("Failed to parse ") + noun + " sequence: " + recs.err_msg; break;  // record.expect(..)
        default: return SMAFA_OK;
    }
    return SMAFA_ERR_PANIC;
}

namespace {

// encode one record; on a byte outside the alphabet produce the panic text of src/lib.rs:38-41
int encode_record(int alphabet, const FastxRecord &rec, std::vector<uint8_t> &codes) {
    const size_t base = codes.size();
    codes.resize(base + rec.seq_len);
    for (size_t i = 0; i < rec.seq_len; i++) {
        const uint8_t c = code_of(alphabet, rec.seq[i]);
        if (c == 255) {
            codes.resize(base);
            return set_error(SMAFA_ERR_PANIC, "Byte %u cannot be interpreted as %s, in sequence \"%.*s\" at position %zu",
                             rec.seq[i], alphabet_noun(alphabet), (int)rec.id_len, (const char *)rec.id, i);
        }
        codes[base + i] = c;
    }
    return SMAFA_OK;
}

void append_decoded(std::string &s, int alphabet, const uint8_t *codes, uint32_t L) {
    const size_t base = s.size();
    s.resize(base + L);
    for (uint32_t i = 0; i < L; i++) s[base + i] = letter_of(alphabet, codes[i]);
}

}  // namespace

// "{query}\t{subject}\t{distance}\t{subject string}\n" per row (src/lib.rs:292,310), written to fd in order.  Big row
// lists are formatted by several threads, each into its own buffer over a contiguous slice of the rows.
int write_rows_text(const smafa_hit *rows, size_t n, const SubjectRows &subjects, int alphabet, uint32_t q_base, int fd) {
    const uint32_t L = subjects.L;
    // (a subject that cannot be read back — a damaged packed store — fails the query; the error text is per thread, so the
    // first failing slice's code and message are carried to the caller)
    auto format = [&](size_t lo, size_t hi, std::string &text, int &frc, std::string &fmsg) {
        frc = SMAFA_OK;
        text.clear();
        text.reserve((hi - lo) * ((size_t)L + 24));
        std::vector<uint8_t> row(L);
        for (size_t i = lo; i < hi; i++) {
            const smafa_hit &h = rows[i];
            append_u32(text, q_base + h.query);
            text.push_back('\t');
            append_u32(text, h.subject);
            text.push_back('\t');
            append_u32(text, h.dist);
            text.push_back('\t');
            frc = subjects.get(h.subject, row.data());
            if (frc) {
                fmsg = smafa_last_error();
                return;
            }
            append_decoded(text, alphabet, row.data(), L);
            text.push_back('\n');
        }
    };
    const size_t block = 1u << 18;  // rows per write
    const unsigned T = n >= (1u << 16) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    std::vector<std::string> parts(T), msgs(T);
    std::vector<int> rcs(T, SMAFA_OK);
    for (size_t b0 = 0; b0 < n; b0 += block * T) {
        const size_t b1 = std::min(n, b0 + block * T), span = b1 - b0;
        if (T == 1) {
            format(b0, b1, parts[0], rcs[0], msgs[0]);
        } else {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < T; t++)
                pool.emplace_back([&, t] { format(b0 + span * t / T, b0 + span * (t + 1) / T, parts[t], rcs[t], msgs[t]); });
            for (auto &th : pool) th.join();
        }
        for (unsigned t = 0; t < T; t++) {
            // the rows in front of the damaged one are written, as a sequential writer would have
            int rc = write_all(fd, parts[t].data(), parts[t].size());
            if (rc) return rc;
            if (rcs[t]) return set_error(rcs[t], "%s", msgs[t].c_str());
        }
    }
    return SMAFA_OK;
}

// The reference `.expect()`s its FASTX inputs: parse_fastx_file(..).expect(what) on the path and record.expect(what) on
// every record (src/lib.rs:144,149,221,234; src/cluster.rs:28,39), so an unreadable, empty, non-FASTX or truncated input
// is a panic — exit 101 — not an Err.  (The DB file is opened with `?`: src/lib.rs:208-210,218 stay SMAFA_ERR_IO /
// SMAFA_ERR_FORMAT, exit 1; so does everything in `count`, src/lib.rs:381,385.)
int expect_fastx(int rc, const char *what) {
    if (rc != SMAFA_ERR_IO && rc != SMAFA_ERR_FORMAT) return rc;
    const std::string msg = smafa_last_error();
    return set_error(SMAFA_ERR_PANIC, "%s: %s", what, msg.c_str());
}

}  // namespace smafa

using namespace smafa;

extern "C" {

// ---------------------------------------------------------------------------------- fastx_load
// The records BEFORE the first offending one, and what is wrong with that one (*pending = 0 or the error code, its text in
// smafa_last_error()): what a driver needs to print the rows the reference prints before it panics (src/lib.rs:232-318).
int smafa_fastx_load_partial(const char *path, int alphabet, uint8_t **codes_out, uint64_t *n_out, uint32_t *seq_len,
                             int *pending) try {
    if (!path || !codes_out || !n_out || !seq_len || !pending)
        return set_error(SMAFA_ERR_INVALID, "smafa_fastx_load_partial: NULL argument");
    if (alphabet != SMAFA_ALPHABET_NT && alphabet != SMAFA_ALPHABET_AA)
        return set_error(SMAFA_ERR_INVALID, "unknown alphabet %d", alphabet);
    *codes_out = nullptr;
    *n_out = 0;
    *seq_len = 0;
    *pending = SMAFA_OK;
    BulkRecords recs;
    int rc = load_records_bulk(path, alphabet, false, recs);
    if (rc) return rc;
    uint8_t *out = (uint8_t *)malloc(recs.codes.empty() ? 1 : recs.codes.size());
    if (!out) return set_error(SMAFA_ERR_NOMEM, "out of host memory");
    if (!recs.codes.empty()) memcpy(out, recs.codes.data(), recs.codes.size());
    *codes_out = out;
    *n_out = recs.n;
    *seq_len = (uint32_t)recs.L;
    if (recs.err_kind == 1) *pending = set_error(SMAFA_ERR_PANIC, "%s", recs.err_msg.c_str());
    else if (recs.err_kind == 2)
        *pending = set_error(SMAFA_ERR_PANIC, "Cannot compute distances between seq of length %zu and windows of lengths %zu",
                             recs.err_len, recs.L);
    else if (recs.err_kind == 3) *pending = set_error(SMAFA_ERR_PANIC, "Cannot add empty sequence to WindowSet");
    else if (recs.err_kind == 4) *pending = set_error(SMAFA_ERR_FORMAT, "%s", recs.err_msg.c_str());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_fastx_load_partial");
}

int smafa_fastx_load(const char *path, int alphabet, uint8_t **codes_out, uint64_t *n_out, uint32_t *seq_len) try {
    if (!path || !codes_out || !n_out || !seq_len) return set_error(SMAFA_ERR_INVALID, "smafa_fastx_load: NULL argument");
    if (alphabet != SMAFA_ALPHABET_NT && alphabet != SMAFA_ALPHABET_AA)
        return set_error(SMAFA_ERR_INVALID, "unknown alphabet %d", alphabet);
    *codes_out = nullptr;
    *n_out = 0;
    *seq_len = 0;
    BulkRecords recs;
    int rc = load_records_bulk(path, alphabet, false, recs);
    if (rc) return rc;
    if (recs.err_kind == 1) return set_error(SMAFA_ERR_PANIC, "%s", recs.err_msg.c_str());
    if (recs.err_kind == 2)
        return set_error(SMAFA_ERR_PANIC, "Cannot compute distances between seq of length %zu and windows of lengths %zu",
                         recs.err_len, recs.L);
    if (recs.err_kind == 3) return set_error(SMAFA_ERR_PANIC, "Cannot add empty sequence to WindowSet");
    if (recs.err_kind == 4) return set_error(SMAFA_ERR_FORMAT, "%s", recs.err_msg.c_str());
    std::vector<uint8_t> &codes = recs.codes;
    const uint64_t n = recs.n;
    const size_t L = recs.L;
    uint8_t *out = (uint8_t *)malloc(codes.empty() ? 1 : codes.size());
    if (!out) return set_error(SMAFA_ERR_NOMEM, "out of host memory");
    if (!codes.empty()) memcpy(out, codes.data(), codes.size());
    *codes_out = out;
    *n_out = n;
    *seq_len = (uint32_t)L;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_fastx_load");
}

// ------------------------------------------------------------------------------------- makedb
int smafa_makedb(const char *subject_fasta, const char *db_path, int alphabet) try {
    if (!subject_fasta || !db_path) return set_error(SMAFA_ERR_INVALID, "smafa_makedb: NULL path");
    if (alphabet != SMAFA_ALPHABET_NT && alphabet != SMAFA_ALPHABET_AA)
        return set_error(SMAFA_ERR_INVALID, "unknown alphabet %d", alphabet);
    BulkRecords recs;
    const double t_start = now_seconds();
    int rc = load_records_bulk(subject_fasta, alphabet, false, recs);  // src/lib.rs:143-152
    if (rc) return expect_fastx(rc, "valid path/file of subject fasta");  // src/lib.rs:144
    const double t_parsed = now_seconds();
    if (recs.err_kind == 3) return set_error(SMAFA_ERR_PANIC, "Cannot add empty sequence to WindowSet");  // src/lib.rs:103-108
    if (recs.err_kind == 1) return set_error(SMAFA_ERR_PANIC, "%s", recs.err_msg.c_str());                  // src/lib.rs:38-41
    if (recs.err_kind == 2)  // src/lib.rs:92-101
        return set_error(SMAFA_ERR_PANIC, "WindowSet seq length is %zu, got a new sequence of length %zu", recs.L, recs.err_len);
    if (recs.err_kind == 4) return set_error(SMAFA_ERR_PANIC, "valid record: %s", recs.err_msg.c_str());  // src/lib.rs:149
    std::vector<uint8_t> &codes = recs.codes;
    const uint64_t n = recs.n;
    const size_t L = recs.L;
    if (L > 0xffffffffull) return set_error(SMAFA_ERR_INVALID, "sequence too long");
    log_line(1, "Encoding of %llu sequences complete, writing db file %s", (unsigned long long)n, db_path);  // src/lib.rs:154-158
    rc = smafa_dbfile_write(db_path, alphabet, codes.data(), n, (uint32_t)L);  // src/lib.rs:161-162
    if (rc == SMAFA_OK) log_line(1, "DB file written");
    log_line(2, "makedb: parse + encode %.2f s, serialise + write %.2f s", t_parsed - t_start, now_seconds() - t_parsed);
    return rc;
} catch (...) {
    return smafa::exception_code("smafa_makedb");
}

// makedb with the packed store file as output (host/packed.cpp): the same parse + encode, then the subjects are packed on
// the device exactly as `query` would pack them, and the resident store is saved.
int smafa_makedb_packed(const char *subject_fasta, const char *db_path, int alphabet, int device) try {
    if (!subject_fasta || !db_path) return set_error(SMAFA_ERR_INVALID, "smafa_makedb_packed: NULL path");
    if (alphabet != SMAFA_ALPHABET_NT && alphabet != SMAFA_ALPHABET_AA)
        return set_error(SMAFA_ERR_INVALID, "unknown alphabet %d", alphabet);
    WarmDevices warm(device < 0 ? 1 << 30 : device);  // (an out-of-range device: nothing to warm)
    BulkRecords recs;
    const double t_start = now_seconds();
    int rc = load_records_bulk(subject_fasta, alphabet, false, recs);  // src/lib.rs:143-152
    const double t_parsed = now_seconds();
    warm.join();
    if (rc) return expect_fastx(rc, "valid path/file of subject fasta");
    if (recs.err_kind == 3) return set_error(SMAFA_ERR_PANIC, "Cannot add empty sequence to WindowSet");
    if (recs.err_kind == 1) return set_error(SMAFA_ERR_PANIC, "%s", recs.err_msg.c_str());
    if (recs.err_kind == 2)
        return set_error(SMAFA_ERR_PANIC, "WindowSet seq length is %zu, got a new sequence of length %zu", recs.L, recs.err_len);
    if (recs.err_kind == 4) return set_error(SMAFA_ERR_PANIC, "valid record: %s", recs.err_msg.c_str());
    if (recs.n == 0) return set_error(SMAFA_ERR_INVALID, "a packed store needs at least one sequence (its length fixes the layout)");
    if (recs.L > 0xffffffffull) return set_error(SMAFA_ERR_INVALID, "sequence too long");
    if (device < 0 || smafa_device_count() == 0) {  // no GPU (or none wanted): the same file, packed by host threads
        log_line(1, "Encoding of %llu sequences complete, packing on the host and writing %s", (unsigned long long)recs.n, db_path);
        rc = pack_store_on_host(alphabet, (uint32_t)recs.L, recs.codes.data(), recs.n, db_path);
        if (rc == SMAFA_OK) log_line(1, "DB file written");
        log_line(2, "makedb --packed: parse + encode %.2f s, pack on the host + write %.2f s", t_parsed - t_start, now_seconds() - t_parsed);
        return rc;
    }
    log_line(1, "Encoding of %llu sequences complete, packing on device %d and writing %s", (unsigned long long)recs.n, device, db_path);
    DbGuard guard;
    const double t_ready = now_seconds();
    rc = smafa_db_create(&guard.db, device, alphabet, (uint32_t)recs.L);
    if (!rc) rc = smafa_db_append(guard.db, recs.codes.data(), recs.n);
    const double t_packed = now_seconds();
    if (!rc) rc = smafa_db_save(guard.db, db_path);
    if (rc == SMAFA_OK) log_line(1, "DB file written");
    log_line(2, "makedb --packed: parse + encode %.2f s (device ready %.2f s after start), pack on the device %.2f s, copy back + write %.2f s",
             t_parsed - t_start, t_ready - t_start, t_packed - t_ready, now_seconds() - t_packed);
    return rc;
} catch (...) {
    return smafa::exception_code("smafa_makedb_packed");
}

// -------------------------------------------------------------------------------------- query
// One process, one handle per entry of `devices` (entries may repeat: several handles on one GPU), the store replicated
// on each.  The query loop of the reference carries no state between records except the running query number
// (src/lib.rs:232-318), so every chunk of queries is cut into ndev contiguous blocks, block g is scanned and selected by
// host thread g on handle g, and the blocks' rows are printed in block order: the output does not depend on ndev.
int smafa_query_multi(const char *db_path, const char *query_fasta, uint32_t max_divergence, uint32_t max_num_hits,
                      uint32_t limit_per_sequence, int out_fd, const int *devices, int ndev) try {
    if (!db_path || !query_fasta) return set_error(SMAFA_ERR_INVALID, "smafa_query: NULL path");
    if (!devices || ndev < 1 || ndev > 64) return set_error(SMAFA_ERR_INVALID, "smafa_query_multi: 1 to 64 devices expected");
    int alphabet = 0;
    uint64_t n = 0;
    uint32_t L = 0;
    FreeGuard codes_guard;
    uint8_t *codes = nullptr;
    const double t_start = now_seconds();
    WarmDevices warm(devices, ndev);  // device bring-up overlaps the file read and decode
    log_line(1, "Decoding db file \"%s\"", db_path);  // src/lib.rs:206
    PackedStore pk;  // a packed store file is mapped, not decoded (host/packed.cpp)
    const bool packed = db_file_is_packed(db_path);
    int rc;
    if (packed) {
        rc = pk.open(db_path);
        if (rc) return rc;
        alphabet = (int)pk.h.alphabet;
        n = pk.h.n;
        L = pk.h.seq_len;
    } else {
        rc = smafa_dbfile_read(db_path, &alphabet, &codes, &n, &L);  // src/lib.rs:208-218
        if (rc) return rc;
        codes_guard.p = codes;
    }
    SubjectRows subjects;
    subjects.codes = codes;
    subjects.packed = packed ? &pk : nullptr;
    subjects.L = L;
    log_line(2, "db %s: %llu sequences of length %u in %.2f s", packed ? "mapped" : "decoded", (unsigned long long)n, L,
             now_seconds() - t_start);

    // Query files of 32 MB and more (after decompression) are parsed and encoded up front by all threads
    // (load_records_bulk: FASTA or FASTQ, plain or gzip); smaller ones are streamed record by record.
    const uint64_t q_bytes = fastx_expanded_size(query_fasta);
    const bool bulk_queries = n > 0 && q_bytes >= (32u << 20) && q_bytes <= (4ull << 30);
    FastxReader reader;
    if (!bulk_queries) {
        rc = reader.open(query_fasta);  // src/lib.rs:221
        if (rc) return expect_fastx(rc, "valid path/file of query fasta");
    }

    // the store on every entry of `devices`: a group (host/group.cpp; public: smafa_group_*)
    struct GroupGuard {
        smafa_group *g = nullptr;
        ~GroupGuard() { smafa_group_destroy(g); }
    } group;
    if (n > 0) {
        warm.join();
        const double t0 = now_seconds();
        if (packed) {
            rc = group_load_packed(&group.g, devices, ndev, pk);
        } else {
            rc = smafa_group_create(&group.g, devices, ndev, alphabet, L);
            if (!rc) rc = smafa_group_append(group.g, codes, n);
        }
        if (rc) return rc;
        // A query file is scanned chunk by chunk against the same resident store: let every replica decide by itself when its block
        // index has paid for itself (rent or buy, smafa_set_index 3 — a run of a few thousand queries never builds one; a million
        // queries against 50M subjects build it during the first chunk).  An explicit SMAFA_INDEX wins.
        if (!getenv("SMAFA_INDEX"))
            for (int g = 0; g < ndev; g++) (void)smafa_set_index(group_member(group.g, g), 3);
        log_line(2, "subject store packed into HBM on %d handle(s) in %.2f s", ndev, now_seconds() - t0);
    }
    // fn(g) for every block of a chunk on its own host thread (without a store: nothing to scan, one thread)
    auto on_every_handle = [&](const std::function<int(int)> &fn) -> int {
        if (group.g) return group_on_every_handle(group.g, fn);
        for (int g = 0; g < ndev; g++) {
            const int r = fn(g);
            if (r) return r;
        }
        return SMAFA_OK;
    };
    log_line(1, "Querying ..");  // src/lib.rs:230
    double t_scan = 0;

    const bool kmode = max_num_hits != SMAFA_NONE && max_num_hits != 1;  // src/lib.rs:224
    // the device bound: k-th smallest distance (k = 1: the minimum); no k bound when k exceeds the store
    const uint32_t dev_k = !kmode ? 1u : (max_num_hits == 0 || max_num_hits > (uint32_t)n) ? SMAFA_NONE : max_num_hits;
    // rows per query are bounded by the store size when nothing else bounds them
    const bool unbounded = max_divergence == SMAFA_NONE && dev_k == SMAFA_NONE;
    const uint64_t chunk_queries =
        (unbounded ? std::max<uint64_t>(1, (16ull << 20) / std::max<uint64_t>(n, 1)) : 65536) * (uint64_t)ndev;

    std::vector<uint8_t> qcodes;
    uint32_t query_number = 0;  // src/lib.rs:231
    uint64_t in_chunk = 0;
    int pending = SMAFA_OK;  // error to report after the rows already due have been printed
    std::string pending_msg;

    // scan + select + print `count` queries whose code rows start at qptr; query_number already counts them
    std::vector<std::vector<smafa_hit>> block_hits((size_t)ndev), block_rows((size_t)ndev);
    auto run_chunk = [&](const uint8_t *qptr, uint64_t count) -> int {
        if (count == 0) return SMAFA_OK;
        const double t0 = now_seconds();
        // block g = queries [count*g/ndev, count*(g+1)/ndev) of the chunk, on handle g
        int r = on_every_handle([&](int g) -> int {
            const uint64_t lo = count * (uint64_t)g / (uint64_t)ndev, hi = count * (uint64_t)(g + 1) / (uint64_t)ndev;
            block_hits[g].clear();
            block_rows[g].clear();
            if (hi == lo) return SMAFA_OK;
            if (n > 0) {
                int rr = scan_to_host(group_member(group.g, g), qptr + (size_t)lo * L, hi - lo, max_divergence, dev_k, block_hits[g]);
                if (rr) return rr;
            }
            return select_rows(block_hits[g].data(), block_hits[g].size(), hi - lo, n, subjects, max_divergence, max_num_hits,
                               limit_per_sequence, block_rows[g]);
        });
        t_scan += now_seconds() - t0;
        if (r) return r;
        for (int g = 0; g < ndev; g++) {
            const uint64_t lo = count * (uint64_t)g / (uint64_t)ndev;
            r = write_rows_text(block_rows[g].data(), block_rows[g].size(), subjects, alphabet,
                                query_number - (uint32_t)count + (uint32_t)lo, out_fd);
            if (r) return r;
        }
        return SMAFA_OK;
    };
    auto flush = [&]() -> int {
        int r = run_chunk(qcodes.data(), in_chunk);
        in_chunk = 0;
        qcodes.clear();
        return r;
    };
    auto length_panic = [&](size_t len) {  // src/lib.rs:72-79
        pending = SMAFA_ERR_PANIC;
        pending_msg = length_panic_text(len, L);
    };

    if (bulk_queries) {
        // big query files: every record parsed and encoded up front by several threads (the loader stops at the
        // first offending record in file order, like the loop below), then scanned chunk by chunk
        BulkRecords recs;
        rc = load_records_bulk(query_fasta, alphabet, false, recs);
        if (rc) return expect_fastx(rc, "valid path/file of query fasta");
        uint64_t usable = recs.n;
        if (recs.n > 0 && recs.L != L) {  // the first query already fails the length check: nothing is printed
            usable = 0;
            length_panic(recs.L);
        } else if (recs.err_kind == 3) {  // an empty query fails the length check too
            length_panic(0);
        } else {  // src/lib.rs:234 for a record that does not parse
            pending = pending_panic(recs, "query", L, pending_msg);
        }
        if (usable > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "too many queries");
        for (uint64_t off = 0; off < usable; off += chunk_queries) {
            const uint64_t count = std::min<uint64_t>(chunk_queries, usable - off);
            query_number += (uint32_t)count;
            int frc = run_chunk(recs.codes.data() + (size_t)off * L, count);
            if (frc) return frc;
        }
        rc = 0;
    } else {
        FastxRecord rec;
        while ((rc = reader.next(rec)) == 1) {
            int erc = encode_record(alphabet, rec, qcodes);  // src/lib.rs:235
            if (erc) {
                pending = erc;
                pending_msg = smafa_last_error();
                break;
            }
            if (n > 0 && rec.seq_len != L) {  // only checked when the store has a length
                qcodes.resize(qcodes.size() - rec.seq_len);
                length_panic(rec.seq_len);
                break;
            }
            if (n == 0) qcodes.resize(qcodes.size() - rec.seq_len);  // nothing to compare with; selection will panic
            in_chunk++;
            query_number++;
            if (in_chunk >= chunk_queries) {
                int frc = flush();
                if (frc) return frc;
            }
        }
    }
    if (rc < 0 && pending == SMAFA_OK) {  // record.expect("Failed to parse query sequence"), src/lib.rs:234
        pending = expect_fastx(rc, "Failed to parse query sequence");
        pending_msg = smafa_last_error();
    }
    int frc = flush();
    if (frc) return frc;
    if (pending != SMAFA_OK) return set_error(pending, "%s", pending_msg.c_str());
    log_line(2, "%u queries: scans + selection %.2f s on %d handle(s)", query_number, t_scan, ndev);
    log_line(1, "Querying complete, took %llu seconds", (unsigned long long)(now_seconds() - t_start));  // src/lib.rs:320-323
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_query_multi");
}

int smafa_query(const char *db_path, const char *query_fasta, uint32_t max_divergence, uint32_t max_num_hits,
                uint32_t limit_per_sequence, int out_fd, int device) try {
    return smafa_query_multi(db_path, query_fasta, max_divergence, max_num_hits, limit_per_sequence, out_fd, &device, 1);
} catch (...) {
    return smafa::exception_code("smafa_query");
}


// ---------------------------------------------------------------------------------- write_rows
int smafa_write_rows(const smafa_hit *rows, uint64_t n_rows, const uint8_t *subject_codes, uint64_t n_subjects,
                     uint32_t seq_len, int alphabet, uint32_t query_offset, int out_fd) try {
    if ((!rows && n_rows) || (!subject_codes && n_rows)) return set_error(SMAFA_ERR_INVALID, "smafa_write_rows: NULL argument");
    if (alphabet != SMAFA_ALPHABET_NT && alphabet != SMAFA_ALPHABET_AA)
        return set_error(SMAFA_ERR_INVALID, "unknown alphabet %d", alphabet);
    for (uint64_t i = 0; i < n_rows; i++)
        if (rows[i].subject >= n_subjects)
            return set_error(SMAFA_ERR_INVALID, "row %llu names subject %u of %llu", (unsigned long long)i, rows[i].subject,
                             (unsigned long long)n_subjects);
    SubjectRows subjects;
    subjects.codes = subject_codes;
    subjects.L = seq_len;
    return write_rows_text(rows, n_rows, subjects, alphabet, query_offset, out_fd);
} catch (...) {
    return smafa::exception_code("smafa_write_rows");
}

// -------------------------------------------------------------------------------------- count
int smafa_count(const char *const *paths, uint64_t n_paths, int out_fd) try {
    std::string text = "[";
    for (uint64_t i = 0; i < n_paths; i++) {
        FastxReader reader;
        int rc = reader.open(paths[i]);
        if (rc) return rc;
        uint64_t reads = 0, bases = 0;
        FastxRecord rec;
        while ((rc = reader.next(rec)) == 1) {
            reads++;
            bases += rec.seq_len;
        }
        if (rc < 0) return rc;
        if (i) text.push_back(',');
        text += "{\"path\":\"";
        for (const char *c = paths[i]; *c; c++) {
            if (*c == '"' || *c == '\\') text.push_back('\\');
            text.push_back(*c);
        }
        text += "\",\"num_reads\":" + std::to_string(reads) + ",\"num_bases\":" + std::to_string(bases) + "}";
    }
    text += "]\n";
    return write_all(out_fd, text.data(), text.size());
} catch (...) {
    return smafa::exception_code("smafa_count");
}

}  // extern "C"

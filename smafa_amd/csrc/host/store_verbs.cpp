// store_verbs.cpp — the verbs over the resident store of a DB file: the self-join verbs (smafa_pairs .. smafa_neighbours),
// consensus and subset, and the two verbs with a reads file (smafa_table, smafa_classify), with the parsers of their side files.
// Each verb loads the DB file on a device, makes one call of the public header and prints its answer as tab-separated rows.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "drivers.h"

using namespace smafa;

namespace {

// ---- what the store verbs print with (smafa_pairs .. smafa_neighbours)
// one row of text: the fields, tabs between them
void append_row(std::string &text, std::initializer_list<uint32_t> fields) {
    char sep = 0;
    for (uint32_t f : fields) {
        if (sep) text.push_back(sep);
        append_u32(text, f);
        sep = '\t';
    }
    text.push_back('\n');
}

// rows 0 .. count - 1 to fd, at most `block` of them per write: row(text, i) appends row i
template <class Row>
int write_rows(int fd, size_t count, size_t block, Row row) {
    std::string text;
    for (size_t b0 = 0; b0 < count; b0 += block) {
        text.clear();
        for (size_t i = b0, e = std::min(count, b0 + block); i < e; i++) row(text, i);
        const int rc = write_all(fd, text.data(), text.size());
        if (rc) return rc;
    }
    return SMAFA_OK;
}
constexpr size_t kRowsPerWrite = (size_t)1 << 18;

}  // namespace

extern "C" {

// ------------------------------------------------------------------- pairs and components: the store
// The DB file of smafa_pairs / smafa_components on `device`: packed store files load as they lie, version 2 / 3 files are
// decoded and appended.  *empty: the DB holds no row (no length to make a store of); store->db stays NULL.
static int load_db_store(const char *db_path, int device, DbGuard *store, bool *empty) {
    *empty = false;
    WarmDevices warm(device);  // device bring-up overlaps the file read
    log_line(1, "Decoding db file \"%s\"", db_path);
    if (db_file_is_packed(db_path)) {
        warm.join();
        return smafa_db_load(&store->db, device, db_path);
    }
    int alphabet = 0;
    uint64_t n = 0;
    uint32_t L = 0;
    FreeGuard codes;
    uint8_t *rows = nullptr;
    int rc = smafa_dbfile_read(db_path, &alphabet, &rows, &n, &L);
    if (rc) return rc;
    codes.p = rows;
    warm.join();
    if (n == 0) {
        *empty = true;
        return SMAFA_OK;
    }
    rc = smafa_db_create(&store->db, device, alphabet, L);
    if (!rc) rc = smafa_db_append(store->db, rows, n);
    return rc;
}

// A store verb between its checks and its print: the clock, the store of the DB file, its subject count.
struct StoreVerb {
    double t_start = 0.0;
    DbGuard store;
    bool empty = false;  // the DB holds no row: store.db is NULL, n is 0
    size_t n = 0;
    unsigned long long seconds() const { return (unsigned long long)(now_seconds() - t_start); }
};

// What every store verb starts with, in this order: the path and the bound checked (who: the verb, for the texts), then the
// verb's further checks, the clock started, the DB file loaded on `device` and its subjects counted (print_pairs has no use for
// the count: its buffer grows by the call's own answer).
static int begin_store_verb(const char *who, const char *db_path, uint32_t max_divergence, int device, StoreVerb &v,
                            const std::function<int()> &more_checks = nullptr) {
    if (!db_path) return set_error(SMAFA_ERR_INVALID, "%s: NULL path", who);
    if (max_divergence == SMAFA_NONE) return set_error(SMAFA_ERR_INVALID, "%s: a bound (max_divergence) is needed", who);
    if (more_checks) {
        const int rc = more_checks();
        if (rc) return rc;
    }
    v.t_start = now_seconds();
    int rc = load_db_store(db_path, device, &v.store, &v.empty);
    if (rc || v.empty) return rc;
    smafa_db_info_t info{};
    rc = smafa_db_info(v.store.db, &info);
    v.n = (size_t)info.n_subjects;
    return rc;
}

// -------------------------------------------------------------------------------------- pairs
// The self-join of a DB file's subjects (smafa_db_self_hits), printed "{i}\t{j}\t{distance}\n" per pair — or, since a row
// (smafa_db_self_hits_since), the pairs whose larger number is at least that row.
static int print_pairs(const char *who, const char *db_path, bool since, uint64_t first_row, uint32_t max_divergence, int out_fd, int device) {
    StoreVerb v;
    int rc = begin_store_verb(who, db_path, max_divergence, device, v);
    if (rc) return rc;
    if (v.empty)  // (an empty DB has no pairs)
        return since && first_row ? set_error(SMAFA_ERR_INVALID, "%s: first_row %llu, the store has 0 subjects", who, (unsigned long long)first_row)
                                  : SMAFA_OK;
    std::vector<smafa_hit> pairs((size_t)1 << 16);
    uint64_t count = 0;
    const auto join = [&] {
        return since ? smafa_db_self_hits_since(v.store.db, first_row, max_divergence, pairs.data(), pairs.size(), &count)
                     : smafa_db_self_hits(v.store.db, max_divergence, pairs.data(), pairs.size(), &count);
    };
    while ((rc = join()) == SMAFA_ERR_CAPACITY) pairs.resize(count);
    if (rc) return rc;
    rc = write_rows(out_fd, count, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_row(text, {pairs[i].query, pairs[i].subject, pairs[i].dist});
    });
    if (rc) return rc;
    log_line(1, "%llu pairs within %u, took %llu seconds", (unsigned long long)count, max_divergence, v.seconds());
    return SMAFA_OK;
}

int smafa_pairs(const char *db_path, uint32_t max_divergence, int out_fd, int device) try {
    return print_pairs("smafa_pairs", db_path, false, 0, max_divergence, out_fd, device);
} catch (...) {
    return smafa::exception_code("smafa_pairs");
}

int smafa_pairs_since(const char *db_path, uint64_t first_row, uint32_t max_divergence, int out_fd, int device) try {
    return print_pairs("smafa_pairs_since", db_path, true, first_row, max_divergence, out_fd, device);
} catch (...) {
    return smafa::exception_code("smafa_pairs_since");
}

// --------------------------------------------------------------------------------- components
// The label of every subject of a DB file (smafa_db_self_components), printed "{i}\t{label}\n" in subject order.
int smafa_components(const char *db_path, uint32_t max_divergence, int out_fd, int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_components", db_path, max_divergence, device, v);
    if (rc || v.empty) return rc;
    std::vector<uint32_t> labels(v.n);
    uint64_t count = 0;
    rc = smafa_db_self_components(v.store.db, max_divergence, labels.data(), labels.size(), &count);
    if (!rc) rc = write_rows(out_fd, v.n, kRowsPerWrite, [&](std::string &text, size_t i) { append_row(text, {(uint32_t)i, labels[i]}); });
    if (rc) return rc;
    log_line(1, "%llu components of %llu sequences within %u, took %llu seconds", (unsigned long long)count, (unsigned long long)v.n,
             max_divergence, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_components");
}

// The labels of every subject of a DB file at every bound 0 .. max_divergence (smafa_db_self_levels), printed
// "{i}\t{label_0}\t...\t{label_N}\n" in subject order.
int smafa_component_levels(const char *db_path, uint32_t max_divergence, int out_fd, int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_component_levels", db_path, max_divergence, device, v);
    if (rc || v.empty) return rc;
    const size_t n = v.n, T = (size_t)max_divergence + 1;
    std::vector<uint32_t> labels(n * T);
    std::vector<uint64_t> counts(T);
    rc = smafa_db_self_levels(v.store.db, max_divergence, labels.data(), labels.size(), counts.data());
    if (!rc) rc = write_rows(out_fd, n, std::max<size_t>(1, kRowsPerWrite / T), [&](std::string &text, size_t i) {
        append_u32(text, (uint32_t)i);
        for (size_t t = 0; t < T; t++) {
            text.push_back('\t');
            append_u32(text, labels[t * n + i]);
        }
        text.push_back('\n');
    });
    if (rc) return rc;
    log_line(1, "%llu components of %llu sequences within 0, %llu within %u, took %llu seconds", (unsigned long long)counts[0],
             (unsigned long long)n, (unsigned long long)counts[T - 1], max_divergence, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_component_levels");
}

// ------------------------------------------------------------------------------------ forest
// The minimum spanning forest of a DB file's subjects up to max_divergence (smafa_db_self_forest), printed
// "{a}\t{b}\t{distance}\n" per edge in the host form's order: by distance, then a, then b.
int smafa_forest(const char *db_path, uint32_t max_divergence, int out_fd, int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_forest", db_path, max_divergence, device, v);
    if (rc || v.empty) return rc;
    const size_t T = (size_t)max_divergence + 1;
    std::vector<smafa_hit> edges(std::max<size_t>(v.n, 2) - 1);  // (one row at least: the call takes no NULL buffer)
    std::vector<uint64_t> level_ends(T);
    rc = smafa_db_self_forest(v.store.db, max_divergence, edges.data(), edges.size(), level_ends.data());
    const size_t count = (size_t)level_ends[T - 1];
    if (!rc) rc = write_rows(out_fd, count, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_row(text, {edges[i].query, edges[i].subject, edges[i].dist});
    });
    if (rc) return rc;
    log_line(1, "%llu edges among %llu sequences within %u, took %llu seconds", (unsigned long long)count, (unsigned long long)v.n,
             max_divergence, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_forest");
}

// ------------------------------------------------------------------------------------ reach forest
// The mutual-reachability forest of a DB file's subjects up to max_divergence at min_pts (smafa_db_self_reach_forest), printed
// "{a}\t{b}\t{weight}\n" per edge in the host form's order: by weight, then a, then b — or, with `cores`, the core distance of
// every subject instead, "{i}\t{core}\n" in subject order, -1 for a row that is sparse at the bound.
int smafa_reach_forest(const char *db_path, uint32_t max_divergence, uint32_t min_pts, int cores, int out_fd, int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_reach_forest", db_path, max_divergence, device, v);
    if (rc || v.empty) return rc;
    const size_t T = (size_t)max_divergence + 1;
    std::vector<smafa_hit> edges(std::max<size_t>(v.n, 2) - 1);  // (one row at least: the call takes no NULL buffer)
    std::vector<uint64_t> level_ends(T);
    std::vector<uint32_t> core(v.n);
    rc = smafa_db_self_reach_forest(v.store.db, max_divergence, min_pts, edges.data(), edges.size(), level_ends.data(), core.data());
    const size_t count = (size_t)level_ends[T - 1];
    if (!rc && cores) rc = write_rows(out_fd, v.n, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_u32(text, (uint32_t)i);
        text.push_back('\t');
        if (core[i] == SMAFA_NONE) text += "-1";
        else append_u32(text, core[i]);
        text.push_back('\n');
    });
    else if (!rc) rc = write_rows(out_fd, count, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_row(text, {edges[i].query, edges[i].subject, edges[i].dist});
    });
    if (rc) return rc;
    log_line(1, "%llu edges among %llu sequences within %u at min_pts %u, took %llu seconds", (unsigned long long)count,
             (unsigned long long)v.n, max_divergence, min_pts, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_reach_forest");
}

// ------------------------------------------------------------------------------------ stable clusters
// The stable-cluster label of every subject of a DB file (smafa_db_self_stable), printed "{i}\t{label}\n" in subject order — with
// `joined` "{i}\t{label}\t{level}\n", the level at which the subject joined its cluster; noise rows have -1 in both columns.
int smafa_stable(const char *db_path, uint32_t max_divergence, uint32_t min_pts, uint32_t min_cluster_size, int joined, int out_fd,
                 int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_stable", db_path, max_divergence, device, v);
    if (rc || v.empty) return rc;
    std::vector<uint32_t> labels(v.n), since(joined ? v.n : 0);
    uint64_t count = 0;
    rc = smafa_db_self_stable(v.store.db, max_divergence, min_pts, min_cluster_size, labels.data(), joined ? since.data() : nullptr, nullptr,
                              labels.size(), &count);
    const auto append_or_none = [](std::string &text, uint32_t value) {
        if (value == SMAFA_NONE) text += "-1";
        else append_u32(text, value);
    };
    if (!rc) rc = write_rows(out_fd, v.n, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_u32(text, (uint32_t)i);
        text.push_back('\t');
        append_or_none(text, labels[i]);
        if (joined) {
            text.push_back('\t');
            append_or_none(text, since[i]);
        }
        text.push_back('\n');
    });
    if (rc) return rc;
    log_line(1, "%llu stable clusters among %llu sequences up to %u at min_pts %u, min_cluster_size %u, took %llu seconds",
             (unsigned long long)count, (unsigned long long)v.n, max_divergence, min_pts, min_cluster_size, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_stable");
}

// ------------------------------------------------------------------------------------ consensus
// A labels file as the label verbs print it: line j is "{j}\t{label}" and whatever columns follow, label -1 for SMAFA_NONE.  `text`
// is the whole file; -> labels[n], or SMAFA_ERR_INVALID naming the first line that is not what it should be.
// who: the verb, for the texts; may_end_early: the subjects behind the file's last line keep SMAFA_NONE (`smafa table`)
static int parse_labels(const char *who, const std::string &text, size_t n, bool may_end_early, std::vector<uint32_t> &labels) {
    labels.assign(n, SMAFA_NONE);
    size_t at = 0, line = 0;
    const auto bad = [&](const char *what) {
        return set_error(SMAFA_ERR_INVALID, "%s: labels line %llu: %s", who, (unsigned long long)line + 1, what);
    };
    // an unsigned decimal number of at most ten digits at text[at ..), -> false where there is none
    const auto number = [&](uint64_t *out) {
        size_t digits = 0;
        uint64_t v = 0;
        while (at < text.size() && text[at] >= '0' && text[at] <= '9' && digits < 11) v = v * 10 + (uint64_t)(text[at++] - '0'), digits++;
        *out = v;
        return digits > 0 && digits < 11;
    };
    for (; at < text.size(); line++) {
        if (line >= n) return bad("more lines than the database has sequences");
        uint64_t i = 0, label = SMAFA_NONE;
        if (!number(&i)) return bad("no sequence number");
        if (i != line) return bad("the sequence number is not the line's own (line j carries sequence j)");
        if (at >= text.size() || text[at] != '\t') return bad("no tab behind the sequence number");
        at++;
        if (text.compare(at, 2, "-1") == 0) at += 2;
        else if (!number(&label)) return bad("no label");
        else if (label >= n) return bad("the label is neither -1 nor the number of a sequence of the database");
        if (at < text.size() && text[at] != '\t' && text[at] != '\n' && text[at] != '\r') return bad("the label is not a number");
        labels[line] = (uint32_t)label;
        while (at < text.size() && text[at] != '\n') at++;  // further columns
        if (at < text.size()) at++;
    }
    if (line < n && !may_end_early) return bad("the file ends here, the database has more sequences");
    return SMAFA_OK;
}

// the whole of a verb's side file ("-": stdin); who: the verb, what: the file's kind, for the texts
static int read_whole(const char *who, const char *what, const char *path, std::string &text) {
    const bool std_in = !strcmp(path, "-");
    const int fd = std_in ? 0 : open(path, O_RDONLY);
    if (fd < 0) return set_error(SMAFA_ERR_IO, "%s: cannot open %s file \"%s\": %s", who, what, path, strerror(errno));
    char buf[1 << 16];
    ssize_t got = 0;
    while ((got = read(fd, buf, sizeof buf)) > 0 || (got < 0 && errno == EINTR))
        if (got > 0) text.append(buf, (size_t)got);
    const int err = errno;
    if (!std_in) close(fd);
    return got < 0 ? set_error(SMAFA_ERR_IO, "%s: reading %s file \"%s\": %s", who, what, path, strerror(err)) : SMAFA_OK;
}

// The consensus of every labelled cluster of a DB file (smafa_db_consensus), printed
// "{label}\t{size}\t{nearest}\t{max_div}\t{SEQUENCE}\n" per cluster in ascending label order.
int smafa_consensus(const char *db_path, const char *labels_path, int out_fd, int device) try {
    if (!labels_path) return set_error(SMAFA_ERR_INVALID, "smafa_consensus: NULL labels path");
    StoreVerb v;
    int rc = begin_store_verb("smafa_consensus", db_path, 0 /* no bound to check */, device, v);
    if (rc) return rc;
    std::string text;
    rc = read_whole("smafa_consensus", "labels", labels_path, text);
    std::vector<uint32_t> labels;
    if (!rc) rc = parse_labels("smafa_consensus", text, v.n, false, labels);
    if (rc || v.empty) return rc;
    std::string().swap(text);
    smafa_db_info_t info{};
    rc = smafa_db_info(v.store.db, &info);
    if (rc) return rc;
    const size_t L = info.seq_len;
    uint64_t K = 0;
    rc = smafa_db_consensus(v.store.db, labels.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, &K);
    if (rc && rc != SMAFA_ERR_CAPACITY) return rc;
    std::vector<uint32_t> ids(K), sizes(K), nearest(K), div(v.n), worst(K, 0);
    std::vector<uint8_t> codes(K * L);
    if (K) rc = smafa_db_consensus(v.store.db, labels.data(), ids.data(), sizes.data(), codes.data(), nearest.data(), div.data(), K, &K);
    if (rc) return rc;
    // max_div per cluster: ids[] ascends, so a label's cluster is found by bisection
    for (size_t i = 0; i < v.n; i++) {
        if (labels[i] == SMAFA_NONE) continue;
        const size_t k = (size_t)(std::lower_bound(ids.begin(), ids.end(), labels[i]) - ids.begin());
        worst[k] = std::max(worst[k], div[i]);
    }
    std::vector<char> letters(L);
    int decode_rc = SMAFA_OK;
    rc = write_rows(out_fd, K, std::max<size_t>(1, kRowsPerWrite / (L / 8 + 1)), [&](std::string &out, size_t k) {
        append_u32(out, ids[k]);
        for (uint32_t field : {sizes[k], nearest[k], worst[k]}) {
            out.push_back('\t');
            append_u32(out, field);
        }
        out.push_back('\t');
        const int drc = smafa_decode(info.alphabet, codes.data() + k * L, L, letters.data());
        if (drc) decode_rc = drc;
        out.append(letters.data(), L);
        out.push_back('\n');
    });
    if (!rc) rc = decode_rc;
    if (rc) return rc;
    log_line(1, "%llu consensus sequences of %llu sequences, took %llu seconds", (unsigned long long)K, (unsigned long long)v.n, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_consensus");
}

// --------------------------------------------------------------------------------------- subset
// A list of sequence numbers, one per line in the first column; whatever tab-separated columns follow are ignored, duplicates
// are allowed.  `text` is the whole file; -> listed[n] (1 where the number occurs), or SMAFA_ERR_INVALID naming the first line
// that is not of that form or names a sequence the database does not have.
static int parse_number_list(const char *who, const std::string &text, size_t n, std::vector<uint32_t> &listed) {
    listed.assign(n, 0u);
    size_t at = 0, line = 0;
    const auto bad = [&](const char *what) {
        return set_error(SMAFA_ERR_INVALID, "%s: list line %llu: %s", who, (unsigned long long)line + 1, what);
    };
    for (; at < text.size(); line++) {
        size_t digits = 0;
        uint64_t v = 0;
        while (at < text.size() && text[at] >= '0' && text[at] <= '9' && digits < 11) v = v * 10 + (uint64_t)(text[at++] - '0'), digits++;
        if (digits == 0 || digits >= 11) return bad("no sequence number");
        if (at < text.size() && text[at] != '\t' && text[at] != '\n' && text[at] != '\r') return bad("the sequence number is not a number");
        if (v >= n) return bad("the database has no sequence of that number");
        listed[(size_t)v] = 1u;
        while (at < text.size() && text[at] != '\n') at++;  // further columns
        if (at < text.size()) at++;
    }
    return SMAFA_OK;
}

// A subset of a DB file's sequences (smafa_db_subset) saved as a packed store, "{new}\t{old}\n" per kept sequence printed.
int smafa_subset(const char *db_path, const char *keep_path, const char *drop_path, const char *out_path, int out_fd, int device) try {
    const char *const who = "smafa_subset";
    StoreVerb v;
    int rc = begin_store_verb(who, db_path, 0 /* no bound to check */, device, v, [&] {
        if (!out_path) return set_error(SMAFA_ERR_INVALID, "%s: NULL output path", who);
        if (keep_path && drop_path) return set_error(SMAFA_ERR_INVALID, "%s: a keep list or a drop list, not both", who);
        if (!keep_path && !drop_path) return set_error(SMAFA_ERR_INVALID, "%s: a keep list or a drop list is needed", who);
        return (int)SMAFA_OK;
    });
    if (rc) return rc;
    if (v.empty) return set_error(SMAFA_ERR_INVALID, "%s: the database holds no sequence: there is no store to take a subset of", who);
    std::string text;
    rc = read_whole(who, "list", keep_path ? keep_path : drop_path, text);
    std::vector<uint32_t> listed;
    if (!rc) rc = parse_number_list(who, text, v.n, listed);
    if (rc) return rc;
    std::string().swap(text);
    DbGuard sub;
    std::vector<uint32_t> old_of_new(v.n);
    uint64_t k = 0;
    rc = smafa_db_subset(v.store.db, listed.data(), drop_path ? 1 : 0, &sub.db, old_of_new.data(), old_of_new.size(), &k);
    if (!rc) rc = smafa_db_save(sub.db, out_path);
    if (!rc) rc = write_rows(out_fd, (size_t)k, kRowsPerWrite, [&](std::string &out, size_t i) { append_row(out, {(uint32_t)i, old_of_new[i]}); });
    if (rc) return rc;
    log_line(1, "%llu of %llu sequences kept in \"%s\", took %llu seconds", (unsigned long long)k, (unsigned long long)v.n, out_path, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_subset");
}

// ------------------------------------------------------------------------------------ density
// The density-cluster label and the degree of every subject of a DB file (smafa_db_self_density), printed
// "{i}\t{label}\t{degree}\n" in subject order; noise rows have the label -1.
int smafa_density(const char *db_path, uint32_t max_divergence, uint32_t min_pts, int out_fd, int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_density", db_path, max_divergence, device, v);
    if (rc || v.empty) return rc;
    std::vector<uint32_t> labels(v.n), degrees(v.n);
    uint64_t counts[3] = {0, 0, 0};
    rc = smafa_db_self_density(v.store.db, max_divergence, min_pts, labels.data(), degrees.data(), labels.size(), counts);
    if (!rc) rc = write_rows(out_fd, v.n, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_u32(text, (uint32_t)i);
        text.push_back('\t');
        if (labels[i] == SMAFA_NONE) text += "-1";
        else append_u32(text, labels[i]);
        text.push_back('\t');
        append_u32(text, degrees[i]);
        text.push_back('\n');
    });
    if (rc) return rc;
    log_line(1, "%llu clusters, %llu core and %llu noise among %llu sequences within %u at min_pts %u, took %llu seconds",
             (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)v.n,
             max_divergence, min_pts, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_density");
}

// ------------------------------------------------------------------------------------ peaks
// The abundance-peak label, the parent and the weight of every subject of a DB file (smafa_db_self_peaks), printed
// "{i}\t{label}\t{parent}\t{weight}\n" in subject order.
int smafa_peaks(const char *db_path, uint32_t max_divergence, uint32_t radius, int out_fd, int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_peaks", db_path, max_divergence, device, v, [&] {
        if (radius == SMAFA_NONE || radius <= max_divergence) return (int)SMAFA_OK;
        return set_error(SMAFA_ERR_INVALID, "smafa_peaks: radius %u is larger than max_divergence %u", radius, max_divergence);
    });
    if (rc || v.empty) return rc;
    const size_t n = v.n;
    std::vector<uint32_t> labels(n), parents(n), weights(n);
    uint64_t n_peaks = 0;
    rc = smafa_db_self_peaks(v.store.db, max_divergence, radius, labels.data(), parents.data(), weights.data(), n, &n_peaks);
    if (!rc) rc = write_rows(out_fd, n, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_row(text, {(uint32_t)i, labels[i], parents[i], weights[i]});
    });
    if (rc) return rc;
    log_line(1, "%llu peaks among %llu sequences within %u, weighed within %u, took %llu seconds", (unsigned long long)n_peaks,
             (unsigned long long)n, max_divergence, radius == SMAFA_NONE ? max_divergence : radius, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_peaks");
}

// ------------------------------------------------------------------------------------ chimeras
// A weights file: "{i}\t{weight}" and whatever columns follow per line, in any order; a subject without a line has weight 0.
// `text` is the whole file; -> weights[n], or SMAFA_ERR_INVALID naming the first line that is not what it should be.
// who: the verb, what: the file's kind ("weights", "samples"), value: what its second column holds, absent: the value of a row
// without a line — `smafa table` reads its two per-read files with this too
static int parse_weights(const char *who, const char *what, const char *value, uint32_t absent, const std::string &text, size_t n,
                         std::vector<uint32_t> &weights) {
    weights.assign(n, absent);
    std::vector<bool> seen(n, false);
    size_t at = 0, line = 0;
    const auto bad = [&](const std::string &why) {
        return set_error(SMAFA_ERR_INVALID, "%s: %s line %llu: %s", who, what, (unsigned long long)line + 1, why.c_str());
    };
    // an unsigned decimal number of at most ten digits at text[at ..), -> false where there is none
    const auto number = [&](uint64_t *out) {
        size_t digits = 0;
        uint64_t v = 0;
        while (at < text.size() && text[at] >= '0' && text[at] <= '9' && digits < 11) v = v * 10 + (uint64_t)(text[at++] - '0'), digits++;
        *out = v;
        return digits > 0 && digits < 11;
    };
    for (; at < text.size(); line++) {
        uint64_t i = 0, weight = 0;
        if (!number(&i)) return bad("no sequence number");
        if (at >= text.size() || text[at] != '\t') return bad("no tab behind the sequence number");
        at++;
        if (i >= n) return bad("the sequence number is not one of the database's");
        if (seen[i]) return bad("a second line for this sequence");
        if (!number(&weight) || weight > 0xffffffffull) return bad(std::string("no ") + value + " (an unsigned 32-bit number)");
        if (at < text.size() && text[at] != '\t' && text[at] != '\n' && text[at] != '\r') return bad(std::string("the ") + value + " is not a number");
        seen[i] = true;
        weights[i] = (uint32_t)weight;
        while (at < text.size() && text[at] != '\n') at++;  // further columns
        if (at < text.size()) at++;
    }
    return SMAFA_OK;
}

// smafa_peaks with the weights of a file (smafa_db_self_peaks_weighted): the same lines
int smafa_peaks_weighted(const char *db_path, uint32_t max_divergence, uint32_t radius, const char *weights_path, int out_fd, int device) try {
    const char *const who = "smafa_peaks_weighted";
    StoreVerb v;
    int rc = begin_store_verb(who, db_path, max_divergence, device, v, [&] {
        if (!weights_path) return set_error(SMAFA_ERR_INVALID, "%s: NULL weights path", who);
        if (radius == SMAFA_NONE || radius <= max_divergence) return (int)SMAFA_OK;
        return set_error(SMAFA_ERR_INVALID, "%s: radius %u is larger than max_divergence %u", who, radius, max_divergence);
    });
    if (rc || v.empty) return rc;
    const size_t n = v.n;
    std::vector<uint32_t> given;
    {
        std::string text;
        rc = read_whole(who, "weights", weights_path, text);
        if (!rc) rc = parse_weights(who, "weights", "weight", 0, text, n, given);
        if (rc) return rc;
    }
    std::vector<uint32_t> labels(n), parents(n), weights(n);
    uint64_t n_peaks = 0;
    rc = smafa_db_self_peaks_weighted(v.store.db, max_divergence, radius, given.data(), labels.data(), parents.data(), weights.data(), n, &n_peaks);
    if (!rc) rc = write_rows(out_fd, n, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_row(text, {(uint32_t)i, labels[i], parents[i], weights[i]});
    });
    if (rc) return rc;
    log_line(1, "%llu peaks among %llu sequences within %u, given weights summed within %u, took %llu seconds", (unsigned long long)n_peaks,
             (unsigned long long)n, max_divergence, radius == SMAFA_NONE ? max_divergence : radius, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_peaks_weighted");
}

// The verdict of the chimera check for every subject of a DB file (smafa_db_self_chimeras), printed
// "{i}\t{flag}\t{left_parent}\t{left_len}\t{right_parent}\t{right_len}\t{weight}\n" in subject order, -1 for SMAFA_NONE.
int smafa_chimeras(const char *db_path, uint32_t max_divergence, uint32_t radius, uint32_t min_fold, const char *weights_path, int out_fd,
                   int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_chimeras", db_path, max_divergence, device, v, [&] {
        if (radius != SMAFA_NONE && radius > max_divergence)
            return set_error(SMAFA_ERR_INVALID, "smafa_chimeras: radius %u is larger than max_divergence %u", radius, max_divergence);
        if (min_fold == 0) return set_error(SMAFA_ERR_INVALID, "smafa_chimeras: min_fold is 0");
        return (int)SMAFA_OK;
    });
    if (rc || v.empty) return rc;
    const size_t n = v.n;
    std::vector<uint32_t> given;
    if (weights_path) {
        std::string text;
        rc = read_whole("smafa_chimeras", "weights", weights_path, text);
        if (!rc) rc = parse_weights("smafa_chimeras", "weights", "weight", 0, text, n, given);
        if (rc) return rc;
    }
    std::vector<uint32_t> flags(n), left(n), left_len(n), right(n), right_len(n), weights(n);
    uint64_t n_chimeras = 0;
    rc = smafa_db_self_chimeras(v.store.db, max_divergence, radius, min_fold, weights_path ? given.data() : nullptr, flags.data(), left.data(),
                                left_len.data(), right.data(), right_len.data(), weights.data(), n, &n_chimeras);
    if (!rc) rc = write_rows(out_fd, n, kRowsPerWrite, [&](std::string &text, size_t i) {
        const auto parent = [&](uint32_t p) {
            if (p == SMAFA_NONE) text += "-1";
            else append_u32(text, p);
        };
        append_u32(text, (uint32_t)i);
        text.push_back('\t');
        append_u32(text, flags[i]);
        text.push_back('\t');
        parent(left[i]);
        text.push_back('\t');
        append_u32(text, left_len[i]);
        text.push_back('\t');
        parent(right[i]);
        text.push_back('\t');
        append_u32(text, right_len[i]);
        text.push_back('\t');
        append_u32(text, weights[i]);
        text.push_back('\n');
    });
    if (rc) return rc;
    log_line(1, "%llu chimeras among %llu sequences within %u, weights %s, fold %u, took %llu seconds", (unsigned long long)n_chimeras,
             (unsigned long long)n, max_divergence, weights_path ? "given" : "counted", min_fold, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_chimeras");
}

// ------------------------------------------------------------------------ verbs with a reads file
// What `smafa table` and `smafa classify` share: a store verb with a reads file, per-read samples and weights files, an entry
// buffer that grows by the call's own answer and the same three columns per entry.
struct ReadsVerb {
    StoreVerb v;
    FreeGuard codes;  // the reads' code rows
    uint64_t m = 0;
    std::vector<uint32_t> samples, weights;  // where their files are given
    uint32_t n_samples = 1;
    const uint8_t *rows() const { return static_cast<const uint8_t *>(codes.p); }
};

// begin_store_verb for such a verb.  Checked in this order: the two paths and the bound, the verb's further checks, that at most
// one of its side files (own: the kind of the verb's own file, the first of `side_paths`) is stdin; then the store, and — unless
// the DB holds no row — the reads loaded in its alphabet and their length held against its rows'.
static int begin_reads_verb(const char *who, const char *db_path, const char *query_fasta, uint32_t max_divergence, int device, ReadsVerb &r,
                            const char *own, std::initializer_list<const char *> side_paths, const std::function<int()> &more_checks) {
    int rc = begin_store_verb(who, db_path, max_divergence, device, r.v, [&] {
        if (!query_fasta) return set_error(SMAFA_ERR_INVALID, "%s: NULL reads path", who);
        const int mrc = more_checks();
        if (mrc) return mrc;
        int from_stdin = 0;
        for (const char *path : side_paths) from_stdin += path && !strcmp(path, "-");
        if (from_stdin > 1) return set_error(SMAFA_ERR_INVALID, "%s: at most one of the %s, samples and weights files may be stdin", who, own);
        return (int)SMAFA_OK;
    });
    if (rc || r.v.empty) return rc;
    smafa_db_info_t info{};
    rc = smafa_db_info(r.v.store.db, &info);
    if (rc) return rc;
    uint8_t *rows = nullptr;
    uint32_t L = 0;
    log_line(1, "Reading reads file \"%s\"", query_fasta);
    rc = smafa_fastx_load(query_fasta, info.alphabet, &rows, &r.m, &L);
    if (rc) return rc;
    r.codes.p = rows;
    if (r.m && L != info.seq_len)  // src/lib.rs:72-79, as `smafa query` fails
        return set_error(SMAFA_ERR_PANIC, "Cannot compute distances between seq of length %u and windows of lengths %u", L, info.seq_len);
    return SMAFA_OK;
}

// a side file read whole and handed to parse(text)
static int side_file(const char *who, const char *path, const char *what, const std::function<int(const std::string &)> &parse) {
    std::string text;
    const int rc = read_whole(who, what, path, text);
    return rc ? rc : parse(text);
}

// the samples and weights files (nullptr: none), one line per read; n_samples: the largest sample number + 1
static int read_samples_weights(const char *who, const char *samples_path, const char *weights_path, ReadsVerb &r) {
    int rc = SMAFA_OK;
    if (samples_path)
        rc = side_file(who, samples_path, "samples", [&](const std::string &text) { return parse_weights(who, "samples", "sample", 0, text, r.m, r.samples); });
    if (!rc && weights_path)
        rc = side_file(who, weights_path, "weights", [&](const std::string &text) { return parse_weights(who, "weights", "weight", 1, text, r.m, r.weights); });
    if (rc) return rc;
    uint32_t top = 0;
    for (uint32_t s : r.samples) top = std::max(top, s);
    if (top == SMAFA_NONE) return set_error(SMAFA_ERR_INVALID, "%s: sample number %u is too large", who, top);
    r.n_samples = top + 1u;
    return SMAFA_OK;
}

// call() fills `entries` and totals[]; on SMAFA_ERR_CAPACITY totals[0] is the number it needs: once more with that many
static int call_with_entries(std::vector<smafa_table_entry> &entries, const uint64_t *totals, const std::function<int()> &call) {
    int rc = call();
    if (rc == SMAFA_ERR_CAPACITY) {
        entries.resize(totals[0]);
        rc = call();
    }
    return rc;
}

// a number, -1 for SMAFA_NONE
static void append_field(std::string &text, uint32_t f) {
    if (f == SMAFA_NONE) text += "-1";
    else append_u32(text, f);
}

// the first `count` entries, "{label}\t{sample}\t{count}\n" each: label(text, id) appends an entry's label
static int write_entries(int out_fd, const std::vector<smafa_table_entry> &entries, uint64_t count,
                         const std::function<void(std::string &, uint32_t)> &label) {
    return write_rows(out_fd, count, kRowsPerWrite, [&](std::string &text, size_t e) {
        label(text, entries[e].label);
        text.push_back('\t');
        append_u32(text, entries[e].sample);
        text.push_back('\t');
        text += std::to_string((unsigned long long)entries[e].count);
        text.push_back('\n');
    });
}

// ------------------------------------------------------------------------------------ table
// The abundance table of a reads file against a DB file (smafa_db_assign), printed "{label}\t{sample}\t{count}\n" per entry in
// table order — or "{read}\t{subject}\t{dist}\n" per read (per_read), or "{i}\t{count}\n" per subject (per_sequence); -1 for
// SMAFA_NONE.  An empty DB prints nothing.
int smafa_table(const char *db_path, const char *query_fasta, uint32_t max_divergence, const char *labels_path, const char *samples_path,
                const char *weights_path, int per_read, int per_sequence, int out_fd, int device) try {
    const char *const who = "smafa_table";
    ReadsVerb r;
    StoreVerb &v = r.v;
    int rc = begin_reads_verb(who, db_path, query_fasta, max_divergence, device, r, "labels", {labels_path, samples_path, weights_path}, [&] {
        if (per_read && per_sequence) return set_error(SMAFA_ERR_INVALID, "%s: per_read and per_sequence exclude each other", who);
        return (int)SMAFA_OK;
    });
    if (rc || v.empty) return rc;
    const uint64_t m = r.m;
    std::vector<uint32_t> labels;
    if (labels_path) rc = side_file(who, labels_path, "labels", [&](const std::string &text) { return parse_labels(who, text, v.n, true, labels); });
    if (!rc) rc = read_samples_weights(who, samples_path, weights_path, r);
    if (rc) return rc;
    const uint32_t n_samples = r.n_samples;
    std::vector<uint32_t> subject(per_read ? m : 0), dist(per_read ? m : 0);
    std::vector<uint64_t> subject_counts(per_sequence ? v.n : 0);
    std::vector<smafa_table_entry> entries((size_t)std::min<uint64_t>(m, (uint64_t)1 << 16));
    uint64_t totals[4] = {0, 0, 0, 0};
    rc = call_with_entries(entries, totals, [&] {
        return smafa_db_assign(v.store.db, r.rows(), m, max_divergence, labels_path ? labels.data() : nullptr, samples_path ? r.samples.data() : nullptr,
                               n_samples, weights_path ? r.weights.data() : nullptr, per_read ? subject.data() : nullptr,
                               per_read ? dist.data() : nullptr, per_sequence ? subject_counts.data() : nullptr,
                               entries.empty() ? nullptr : entries.data(), entries.size(), totals);
    });
    if (rc) return rc;
    if (per_read) rc = write_rows(out_fd, m, kRowsPerWrite, [&](std::string &text, size_t q) {
        append_u32(text, (uint32_t)q);
        text.push_back('\t');
        append_field(text, subject[q]);
        text.push_back('\t');
        append_field(text, dist[q]);
        text.push_back('\n');
    });
    else if (per_sequence) rc = write_rows(out_fd, v.n, kRowsPerWrite, [&](std::string &text, size_t i) {
        append_u32(text, (uint32_t)i);
        text.push_back('\t');
        text += std::to_string((unsigned long long)subject_counts[i]);
        text.push_back('\n');
    });
    else rc = write_entries(out_fd, entries, totals[0], append_field);
    if (rc) return rc;
    log_line(1, "%llu table entries of %llu reads in %u samples against %llu sequences within %u: weight %llu assigned, %llu unassigned, took %llu seconds",
             (unsigned long long)totals[0], (unsigned long long)m, n_samples, (unsigned long long)v.n, max_divergence,
             (unsigned long long)totals[1], (unsigned long long)totals[2], v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_table");
}

// ------------------------------------------------------------------------------------ classify
// The nodes of a taxonomy file, interned by (parent id, name) in order of first appearance: a node's id is its number here, so
// two nodes of one name under different parents never share an id.
struct TaxonNodes {
    std::vector<uint32_t> parent;  // SMAFA_NONE: a rank-0 node
    std::vector<std::string> name;
    std::map<std::pair<uint32_t, std::string>, uint32_t> id_of;
    uint32_t intern(uint32_t up, const std::string &text) {
        const auto at = id_of.find({up, text});
        if (at != id_of.end()) return at->second;
        const uint32_t id = (uint32_t)name.size();
        id_of.emplace(std::make_pair(up, text), id);
        parent.push_back(up);
        name.push_back(text);
        return id;
    }
    // the names joined by ';' down to the node; "root" and "unassigned" for the two special values
    void append_lineage(std::string &text, uint32_t id) const {
        if (id == SMAFA_NONE) return (void)(text += "unassigned");
        if (id == SMAFA_TAXON_ROOT || id >= name.size()) return (void)(text += "root");
        uint32_t path[16], depth = 0;
        for (uint32_t at = id; at != SMAFA_NONE && depth < 16; at = parent[at]) path[depth++] = at;
        while (depth) {
            text += name[path[--depth]];
            if (depth) text.push_back(';');
        }
    }
};

// A taxonomy file: "{i}\t{name};{name};..." and whatever columns follow per line, in any order, names trimmed of blanks; a
// subject without a line has no lineage.  `text` is the whole file; -> rows[n][16] of node ids (SMAFA_NONE behind a row's last
// name) and *ranks, the longest row (at least 1), or SMAFA_ERR_INVALID naming the first line that is not what it should be.
static int parse_taxonomy(const char *who, const std::string &text, size_t n, TaxonNodes &nodes, std::vector<uint32_t> &rows, uint32_t *ranks) {
    rows.assign(n * 16, SMAFA_NONE);
    *ranks = 1;
    std::vector<bool> seen(n, false);
    size_t at = 0, line = 0;
    const auto bad = [&](const char *why) {
        return set_error(SMAFA_ERR_INVALID, "%s: taxonomy line %llu: %s", who, (unsigned long long)line + 1, why);
    };
    for (; at < text.size(); line++) {
        size_t digits = 0;
        uint64_t i = 0;
        while (at < text.size() && text[at] >= '0' && text[at] <= '9' && digits < 11) i = i * 10 + (uint64_t)(text[at++] - '0'), digits++;
        if (digits == 0 || digits >= 11) return bad("no sequence number");
        if (at >= text.size() || text[at] != '\t') return bad("no tab behind the sequence number");
        at++;
        if (i >= n) return bad("the sequence number is not one of the database's");
        if (seen[i]) return bad("a second line for this sequence");
        seen[i] = true;
        size_t end = at;
        while (end < text.size() && text[end] != '\t' && text[end] != '\n') end++;
        uint32_t depth = 0, up = SMAFA_NONE;
        bool gap = false;  // an empty name: fine at the end of the column, not in front of another name
        for (size_t a = at; a <= end;) {
            size_t b = a;
            while (b < end && text[b] != ';') b++;
            size_t first = a, last = b;
            while (first < last && (text[first] == ' ' || text[first] == '\r')) first++;
            while (last > first && (text[last - 1] == ' ' || text[last - 1] == '\r')) last--;
            if (first == last) {
                gap = true;
            } else {
                if (gap) return bad("an empty name in front of another");
                if (depth == 16) return bad("more than 16 names");
                const std::string name = text.substr(first, last - first);
                if (depth == 0 && (name == "root" || name == "unassigned")) return bad("the first name is \"root\" or \"unassigned\", which the output keeps for itself");
                up = nodes.intern(up, name);
                rows[i * 16 + depth++] = up;
            }
            a = b + 1;
        }
        *ranks = std::max(*ranks, depth);
        at = end;
        while (at < text.size() && text[at] != '\n') at++;  // further columns
        if (at < text.size()) at++;
    }
    return SMAFA_OK;
}

// The classification of a reads file against a DB file (smafa_db_classify), printed "{lineage}\t{sample}\t{count}\n" per entry in
// table order — or "{read}\t{subject}\t{dist}\t{ties}\t{depth}\t{lineage}\n" per read (per_read).  An empty DB prints nothing.
int smafa_classify(const char *db_path, const char *query_fasta, uint32_t max_divergence, uint32_t slack, const char *taxonomy_path,
                   const char *samples_path, const char *weights_path, int per_read, int out_fd, int device) try {
    const char *const who = "smafa_classify";
    ReadsVerb r;
    StoreVerb &v = r.v;
    int rc = begin_reads_verb(who, db_path, query_fasta, max_divergence, device, r, "taxonomy", {taxonomy_path, samples_path, weights_path}, [&] {
        if (!taxonomy_path) return set_error(SMAFA_ERR_INVALID, "%s: NULL taxonomy path", who);
        return (int)SMAFA_OK;
    });
    if (rc || v.empty) return rc;
    const uint64_t m = r.m;
    TaxonNodes nodes;
    std::vector<uint32_t> wide;
    uint32_t ranks = 1;
    rc = side_file(who, taxonomy_path, "taxonomy", [&](const std::string &text) { return parse_taxonomy(who, text, v.n, nodes, wide, &ranks); });
    if (!rc) rc = read_samples_weights(who, samples_path, weights_path, r);
    if (rc) return rc;
    std::vector<uint32_t> lineage(v.n * ranks);  // the rows cut to the longest
    for (size_t i = 0; i < v.n; i++) std::copy(wide.begin() + i * 16, wide.begin() + i * 16 + ranks, lineage.begin() + i * ranks);
    std::vector<uint32_t>().swap(wide);
    const uint32_t n_samples = r.n_samples;
    const size_t per = per_read ? m : 0;
    std::vector<uint32_t> subject(per), dist(per), taxon(per), depth(per), ties(per);
    std::vector<smafa_table_entry> entries((size_t)std::min<uint64_t>(m, (uint64_t)1 << 16));
    uint64_t totals[6] = {0, 0, 0, 0, 0, 0};
    rc = call_with_entries(entries, totals, [&] {
        return smafa_db_classify(v.store.db, r.rows(), m, max_divergence, slack, lineage.data(), ranks, samples_path ? r.samples.data() : nullptr,
                                 n_samples, weights_path ? r.weights.data() : nullptr, per_read ? subject.data() : nullptr,
                                 per_read ? dist.data() : nullptr, per_read ? taxon.data() : nullptr, per_read ? depth.data() : nullptr,
                                 per_read ? ties.data() : nullptr, entries.empty() ? nullptr : entries.data(), entries.size(), totals);
    });
    if (rc) return rc;
    const auto lineage_of = [&](std::string &text, uint32_t id) { nodes.append_lineage(text, id); };
    if (per_read) rc = write_rows(out_fd, m, kRowsPerWrite, [&](std::string &text, size_t q) {
        append_u32(text, (uint32_t)q);
        text.push_back('\t');
        append_field(text, subject[q]);
        text.push_back('\t');
        append_field(text, dist[q]);
        text.push_back('\t');
        append_u32(text, ties[q]);
        text.push_back('\t');
        append_field(text, depth[q]);
        text.push_back('\t');
        lineage_of(text, taxon[q]);
        text.push_back('\n');
    });
    else rc = write_entries(out_fd, entries, totals[0], lineage_of);
    if (rc) return rc;
    log_line(1, "%llu taxon entries of %llu reads in %u samples against %llu sequences within %u, slack %u, %u ranks: weight %llu assigned (%llu on the "
             "root), %llu unassigned, %llu reads with ties, took %llu seconds",
             (unsigned long long)totals[0], (unsigned long long)m, n_samples, (unsigned long long)v.n, max_divergence, slack, ranks,
             (unsigned long long)totals[1], (unsigned long long)totals[4], (unsigned long long)totals[2], (unsigned long long)totals[5], v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_classify");
}

// ------------------------------------------------------------------------------------ neighbours
// The neighbours of every subject of a DB file within the bound, nearest first, at most max_num_hits of them
// (smafa_db_self_neighbours), printed "{i}\t{j}\t{dist}\n" ordered by (i, dist, j): both directions of every pair.
int smafa_neighbours(const char *db_path, uint32_t max_divergence, uint32_t max_num_hits, int out_fd, int device) try {
    StoreVerb v;
    int rc = begin_store_verb("smafa_neighbours", db_path, max_divergence, device, v, [&] {
        return max_num_hits ? (int)SMAFA_OK : set_error(SMAFA_ERR_INVALID, "smafa_neighbours: max_num_hits is 0");
    });
    if (rc || v.empty) return rc;
    const size_t n = v.n;
    std::vector<uint64_t> offsets(n + 1);
    std::vector<uint32_t> neighbours, dists;
    uint64_t total = 0;
    // the capacity protocol: the degrees alone first, then the call sized by them
    rc = smafa_db_self_neighbours(v.store.db, max_divergence, max_num_hits, offsets.data(), nullptr, nullptr, 0, &total);
    if (rc == SMAFA_ERR_CAPACITY) {
        neighbours.resize((size_t)total);
        dists.resize((size_t)total);
        rc = smafa_db_self_neighbours(v.store.db, max_divergence, max_num_hits, offsets.data(), neighbours.data(), dists.data(), total, &total);
    }
    if (rc) return rc;
    // (not write_rows: a write ends with the row whose list crosses a multiple of kRowsPerWrite entries, never inside a list)
    std::string text;
    for (size_t i = 0; i < n; i++) {
        for (uint64_t e = offsets[i]; e < offsets[i + 1]; e++) append_row(text, {(uint32_t)i, neighbours[e], dists[e]});
        if (i + 1 == n || offsets[i + 1] / kRowsPerWrite != offsets[i] / kRowsPerWrite) {
            rc = write_all(out_fd, text.data(), text.size());
            if (rc) return rc;
            text.clear();
        }
    }
    log_line(1, "%llu neighbours of %llu sequences within %u, took %llu seconds", (unsigned long long)total, (unsigned long long)n,
             max_divergence, v.seconds());
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_neighbours");
}

}  // extern "C"

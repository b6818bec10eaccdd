// engine.h — internal interfaces shared by the device half (engine.hip) and the host half (host/*.cpp)
// of libsmafa_amd.so.  No HIP types here: host files are compiled with g++.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/smafa_amd.h"

namespace smafa {

// records the message for smafa_last_error() and returns `code`
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// Inside `catch (...)` of an exported function (every int-returning entry point is a function-try-block: no C++ exception
// leaves the C ABI): std::bad_alloc / std::length_error / std::system_error -> SMAFA_ERR_NOMEM, anything else ->
// SMAFA_ERR_INVALID, the message recorded.  (Worker threads do not catch: running out of memory there ends the process,
// as an allocation failure does in the reference — Rust aborts.)
int exception_code(const char *where) noexcept;

// Scan `n_queries` code rows against the store; rows ordered by (query, dist, subject); rows above the
// k-th smallest distance of their query already removed.  max_num_hits: SMAFA_NONE = no k bound.
int scan_to_host(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div, uint32_t max_num_hits,
                 std::vector<smafa_hit> &out);

// Queries per workgroup pass of a scan launch over n_wg_tiles four-wave shares of the store: `override` (smafa_set_query_block)
// as it is, else nq split into as many blocks as give the grid about 16 workgroups per slot, each of at least 256 queries.  The
// slot count, n_cu x 6, is the first scan kernel's (6 four-wave workgroups per CU); today's zone kernel runs 14 two-wave workgroups
// per CU.  The constants are kept because the block count they give still sits on the flat part of the sweep (aa 10M x 10 000:
// 2-4 blocks 0.415-0.426 ms, 6 — the automatic one — 0.424-0.432, 8 0.44, 12 0.46; nt 10M x 100 000: 8 blocks, the automatic
// count, 1.97 ms, 4 2.03, 2 2.16: profiles/r12_query_block.txt), not because they describe the kernel that runs now.
// chunk > 1: the kernel walks a block in chunks of that many queries, and the automatic size is rounded up to whole chunks — a
// block of 1667 ends in a chunk of 3 live queries that costs a whole one.
inline uint32_t query_block_size(uint32_t override, uint32_t n_cu, uint32_t n_wg_tiles, uint32_t nq, uint32_t chunk) {
    if (override) return override < (nq ? nq : 1u) ? override : (nq ? nq : 1u);
    const uint32_t want_items = n_cu * 6u * 16u;
    uint32_t nqb = (want_items + n_wg_tiles - 1) / n_wg_tiles;
    const uint32_t max_nqb = nq / 256u > 1u ? nq / 256u : 1u;
    nqb = nqb < max_nqb ? nqb : max_nqb;
    if (nqb < 1u) nqb = 1u;
    uint32_t qb = (nq + nqb - 1) / nqb;
    if (chunk > 1u) qb = (qb + chunk - 1) / chunk * chunk;
    return qb ? qb : 1u;
}

// The self-join's piece-size rule (self_join.hip.h: join_pass): what follows a scan of `rows` store rows that found `count` rows
// for a scratch list of `capacity` rows which may grow to `ceiling` rows (SMAFA_JOIN_SCRATCH_MAX).  A count the list held is
// taken, and a piece size reduced earlier doubles back towards `block` (SMAFA_JOIN_BLOCK) once a count falls under a quarter of
// the ceiling.  A count the list did not hold is exact all the same: under the ceiling the list grows to it and the same rows are
// scanned again; above it the piece is cut in half, to whole 64-record chunks; 64 rows or fewer cannot be cut and the call fails.
enum PieceVerdict { kPieceTake, kPieceGrow, kPieceHalve, kPieceFail };
struct PieceRule {
    PieceVerdict verdict;
    uint64_t piece;  // rows per scan from here on
};
inline PieceRule join_piece_rule(uint64_t count, uint64_t capacity, uint64_t ceiling, uint64_t rows, uint64_t piece, uint64_t block) {
    if (count <= capacity) {
        const uint64_t twice = piece * 2 < block ? piece * 2 : block;
        return {kPieceTake, piece < block && count * 4 < ceiling ? twice : piece};
    }
    if (count <= ceiling) return {kPieceGrow, piece};
    if (rows <= 64) return {kPieceFail, piece};
    const uint64_t half = (rows / 2 + 63) / 64 * 64;
    return {kPieceHalve, half > 64 ? half : 64};
}

// The read-table calls' span rule (read_table.hip.h: read_table_spans, for the abundance table and the classification).  A span of reads is scanned in the tightening mode (each read's
// bound follows its smallest distance) into `room` rows of the handle's row list; in that mode a count above the room only says
// "did not fit".  The first room holds 64 rows per read of the span, at least 4096, at most the ceiling (SMAFA_ASSIGN_ROWS_MAX).
// A span that did not fit: the room doubles, up to the ceiling, and the same reads are scanned again; at the ceiling the span is
// cut to max(64, ((reads / 2 + 63) / 64) * 64) reads, and a span of 64 reads or fewer fails.  The reduced span is kept.
inline uint64_t assign_first_room(uint64_t span, uint64_t ceiling) {
    const uint64_t want = span * 64 > 4096 ? span * 64 : 4096;
    return want < ceiling ? want : ceiling;
}
inline PieceRule assign_span_rule(uint64_t count, uint64_t room, uint64_t ceiling, uint64_t reads) {
    if (count <= room) return {kPieceTake, reads};
    if (room < ceiling) return {kPieceGrow, reads};
    if (reads <= 64) return {kPieceFail, reads};
    const uint64_t half = (reads / 2 + 63) / 64 * 64;
    return {kPieceHalve, half > 64 ? half : 64};
}

// How the neighbours call (self_join.hip.h: join_neighbours) orders its entries (row, dist, neighbour): a pure function of the
// store's rows, the bound and the sequence length.  dist_bits holds the largest distance the join can report,
// min(max_div, seq_len); row_bits holds n - 1.  Where both fit 32 bits an entry is ONE 64-bit key, row << (32 + dist_bits) |
// dist << 32 | neighbour, and one radix sort over its 32 + dist_bits + row_bits bits orders the list (sorts = 1); otherwise two
// stable sorts do, by dist << 32 | neighbour and then by the row (sorts = 2).
struct NeighbourKey {
    uint32_t dist_bits, row_bits, sorts;
};
inline NeighbourKey neighbour_key_rule(uint64_t n, uint32_t max_div, uint32_t seq_len) {
    const uint64_t bound = max_div < seq_len ? max_div : seq_len, last = n ? n - 1 : 0;
    uint32_t dist_bits = 1, row_bits = 1;
    while (dist_bits < 32 && (1ull << dist_bits) <= bound) dist_bits++;
    while (row_bits < 32 && (1ull << row_bits) <= last) row_bits++;
    return {dist_bits, row_bits, row_bits + dist_bits <= 32 ? 1u : 2u};
}

// Bring the HIP runtime and the device context up (a few hundred ms the first time in a process).  The drivers call it
// on a helper thread while they read and decode their input; failures are ignored here — the first real call reports.
void warm_device(int device);
// device time of the scan kernels of every host-buffer scan on this handle so far, and their launches
void db_life_stats(const smafa_db *db, double *kernel_ms, uint64_t *launches);
// Forget the subjects but keep the handle's device memory, stream and scratch (cluster's per-batch candidate store).
int db_clear(smafa_db *db);
class PackedStore;
// Where the drivers read a subject's symbols from: code rows in host memory (a decoded version-2 file) or the mapped
// bit-plane tiles of a packed store file (host/packed.cpp), decoded row by row — only hit rows are ever read.
struct SubjectRows {
    const uint8_t *codes = nullptr;
    const PackedStore *packed = nullptr;
    uint32_t L = 0;
    int get(uint64_t j, uint8_t *out) const;  // L code bytes of subject j; fails on a damaged packed store
};
// selection rules of src/lib.rs:241-315 (see smafa_select_rows in the public header)
int select_rows(const smafa_hit *hits, uint64_t n_hits, uint64_t n_queries, uint64_t n_subjects,
                const SubjectRows &subjects, uint32_t max_div, uint32_t max_num_hits, uint32_t limit_per_sequence,
                std::vector<smafa_hit> &rows);
// "{q_base + query}\t{subject}\t{distance}\t{subject string}\n" per row (src/lib.rs:292,310) to fd (host/drivers.cpp)
int write_rows_text(const smafa_hit *rows, size_t n, const SubjectRows &subjects, int alphabet, uint32_t q_base, int fd);
// IO / format failures of the FASTX layer become the reference's .expect(what) panic (host/drivers.cpp)
int expect_fastx(int rc, const char *what);
// a store handle whose HBM image comes straight from a mapped packed store file
int db_load_packed(smafa_db **out, int device, const PackedStore &pk);

// ---- a store replicated over several devices behind one handle (host/group.cpp; public: smafa_group_*)
// fn(g) for every member on its own host thread; first failure in member order
int group_on_every_handle(smafa_group *grp, const std::function<int(int)> &fn);
int group_load_packed(smafa_group **out, const int *devices, int ndev, const PackedStore &pk);
smafa_db *group_member(smafa_group *grp, int g);
int group_size(const smafa_group *grp);

// stderr logging of the drivers (host/common.cpp): level 1 = info, 2 = debug
int verbosity();
void log_line(int level, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
double now_seconds();

// alphabet tables (host/alphabet.cpp)
uint8_t code_of(int alphabet, uint8_t byte);  // 255 = outside the alphabet
const uint8_t *code_table(int alphabet);      // the same as a 256-entry table (for loops over many bytes)
char letter_of(int alphabet, uint8_t code);
const char *alphabet_noun(int alphabet);  // "nucleotide" / "amino acid" for the panic text

}  // namespace smafa

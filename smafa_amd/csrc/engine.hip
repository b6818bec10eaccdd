// engine.hip — device half of the C ABI (include/smafa_amd.h): HBM-resident subject store, packed
// query sets, scan launches, row collection and ordering.  Host-only entry points (FASTX, DB file,
// selection, drivers) live in host/*.cpp.  No CPU fallback anywhere: without a HIP device every call
// here fails.
#include <hipcub/hipcub.hpp>
#include <cmath>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "scan_plan.h"
#include "kth_plan.h"
#include "host/packed.h"
#include "kernels.hip.h"
#include "index.hip.h"
#include "join.hip.h"
#include "components.hip.h"
#include "levels.hip.h"
#include "density.hip.h"
#include "peaks.hip.h"
#include "neighbours.hip.h"
#include "delta.hip.h"
#include "forest.hip.h"
#include "reach.hip.h"
#include "stable.hip.h"
#include "consensus.hip.h"
#include "chimera.hip.h"
#include "assign.hip.h"
#include "classify.hip.h"
#include "subset.hip.h"

namespace smafa {

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return set_error(SMAFA_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// planes per query record: 3 code bits for ACGTN, 5 for the amino-acid codes 0..27
static int query_planes_for(int alphabet) { return alphabet == SMAFA_ALPHABET_AA ? 5 : 3; }

// row counter (u64) at byte 0, ticket counters of finish_rows from byte 256 on
constexpr size_t kCtrBytes = 256 + (size_t)(1 + kTicketGroups) * kTicketStride * sizeof(uint32_t);

// grow-only device buffer (scratch that is reused across calls: hipMalloc/hipFree cost far more than a scan)
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return SMAFA_OK;
        if (p) HIP_TRY(hipFree(p));
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes, 4096);
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return SMAFA_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// Scratch of an unusually large answer is not worth keeping (the buffers regrow on demand): behind a call, each of `bufs` that has
// grown past kTrimBytes is released (trim) — or all of `rest` with `lead`, where `lead` has (trim_together: the sort's buffers).
// Which buffers a call names decides what the next call allocates.
constexpr size_t kTrimBytes = 512ull << 20;
static void trim(std::initializer_list<DevBuf *> bufs) {
    for (DevBuf *b : bufs)
        if (b->cap > kTrimBytes) b->release();
}
static void trim_together(DevBuf &lead, std::initializer_list<DevBuf *> rest) {
    if (lead.cap <= kTrimBytes) return;
    lead.release();
    for (DevBuf *b : rest) b->release();
}

}  // namespace smafa

using namespace smafa;

static std::atomic<uint64_t> g_qset_serial{1};

struct smafa_qset {
    smafa_db *db = nullptr;
    uint64_t nq = 0;
    uint64_t serial = 0;  // unique per fill of the set: a recreated set at a recycled address is a different set
    DevBuf qrec, thr, cnt;  // packed records, per-query bounds, per-query distance histograms (k >= 2 only)
};

struct smafa_db {
    int device = 0;
    int alphabet = 0;
    uint32_t L = 0, W = 0, QS = 0;
    uint32_t P = 0;   // planes stored per SUBJECT: 5 (aa), 3 (nt), or 2 while no nucleotide subject holds an N
    uint32_t PQ = 0;  // planes per QUERY record: 5 (aa) or 3 (nt)
    uint64_t n = 0;          // subjects stored
    uint64_t cap_tiles = 0;  // allocated wave tiles
    uint32_t *d_planes = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    uint32_t last_launches = 0;
    // totals over the scans of the most recent host-buffer call (smafa_scan_hits: the near-hit ladder and the tightening
    // path are several scans): smafa_last_call_stats
    float call_ms = 0.f;
    uint32_t call_launches = 0, call_scans = 0;
    // Where the scan launches of this handle really went: the HIP device current on the launching thread at each launch
    // (smafa_launch_device).  A member of a multi-device group whose worker thread forgot hipSetDevice would show here.
    int launch_device = -1;
    uint64_t launches_off_device = 0;
    double life_ms = 0.0;        // ... and over the handle's life (the cluster driver's debug line)
    uint64_t life_launches = 0;
    // smafa_scan_each: the K one-query launches captured once as a HIP graph and replayed
    hipGraphExec_t each_graph = nullptr;
    // (the captured kernel nodes bake in the set's device record buffer: the key names the set by its serial and that pointer,
    // not by its host address alone — a destroyed set's address is handed out again by the next `new`)
    struct EachKey { const void *qs, *qrec, *hits, *counts; uint64_t qs_serial, cap, nq, generation; uint32_t max_div, qb; int zone; bool filter; } each_key{};
    std::vector<std::string> each_kernels;  // ... and the instantiations its capture launched (a replay names them again)
    uint32_t qb_override = 0;
    ScanKnobs knobs;  // the switches the kernel choice of a scan launch reads (scan_plan.h)
    // what the last launch used (smafa_last_scan_plan)
    uint32_t plan_lazy = 0, plan_tiles = 1, plan_qblocks = 1;
    char plan_kernel[96] = "";  // the instantiation of the last launch, as rocprofv3 names it (smafa_last_scan_kernel)
    // every distinct instantiation the current call launched, in first-launch order (smafa_last_call_kernels); reset by
    // smafa_scan_hits, smafa_scan_launch, smafa_scan_each and smafa_distances
    std::vector<std::string> call_kernels;
    int n_cu = 256;
    // scratch of the host-buffer API, kept across calls
    DevBuf upload;            // staging for code rows on their way to the pack kernel
    DevBuf hits, count;       // rows and their counter
    DevBuf scratch;           // row list of the tightening modes (everything appended while bounds were still running)
    DevBuf ctrs;              // [0]: the scan kernels' row counter (u64), [256]: finished-workgroup tickets (u32); both zero between scans
    DevBuf keys_a, keys_b, sort_tmp;
    DevBuf idx_a, idx_b;      // sort payload of an append: source row per sorted position
    // ---- layout of the packed store (fixed when the first rows arrive)
    bool layout_set = false;
    std::vector<uint32_t> perm;  // packed column j holds source column perm[j]
    std::vector<uint8_t> tab;    // [source column][code] -> stored code
    DevBuf d_perm, d_tab;
    DevBuf d_inv;                // [source column][stored code] -> code, the inverse of tab: built by the first smafa_db_rows call (subset_abi.hip.h)
    uint32_t *d_order = nullptr;  // position -> subject index (cap_tiles * 256 entries)
    uint4 *d_zone = nullptr;      // per wave tile: shared filter bits (cap_tiles entries)
    struct Run { uint64_t rows; bool sorted; };
    std::vector<Run> runs;        // the appends the store consists of (each sorted within itself or not); kept in the packed file
    // What the zone level can prune with, MEASURED: shared filter bits per wave tile (both words), read back after every
    // append; hist[b] = tiles sharing b bits.  Sorting gives ~log2(rows / 256) on unrelated sequences, related ones share
    // more, many small appends share few — zone_pays() works from this, not from assumptions about the data.
    std::vector<uint8_t> tile_bits;
    uint64_t zone_hist[65] = {0};
    uint64_t rows_since_sort = 0;  // rows appended since the whole store was last in one sorted run
    uint32_t resorts = 0;          // full re-sorts so far (resort_store)
    bool resort = true;            // SMAFA_RESORT=0: never
    uint64_t resort_min = 32768;   // stores below this many rows are left alone (SMAFA_RESORT_MIN)
    bool sort_rows = true;        // sort big appends by their filter words (SMAFA_SORT=0: keep the append order)
    smafa_qset scratch_q;     // query set of smafa_scan_hits / smafa_distances
    smafa_qset scratch_q2;    // the compacted batch of queries the near-hit probe did not finish
    smafa_qset scratch_q3;    // the sample of open queries the later steps of the ladder are planned from
    smafa_qset join_q;        // the self-join's block of store rows as query records (store_records_kernel)
    bool two_phase = true;    // near-hit probe before the tightening path (SMAFA_TWO_PHASE=0 disables)
    bool stream_nt = true;    // one-query-block launches of scan_lazy_kernel load their filter words non-temporally (SMAFA_STREAM_NT=0)
    uint32_t count_first_k = 3;  // smallest k whose loose-bound scans count first and append second (SMAFA_COUNT_FIRST_K)
    bool ladder_probe = true;    // the ladder's first step is asked of a 256-query sample before the whole batch pays for it (SMAFA_LADDER_PROBE=0)
    int zone_key_gate = -1;      // ScanArgs::key_gate (SMAFA_ZONE_KEY_GATE; 65: no key test); -1: by alphabet (kernels.hip.h)
    bool kth_hist_seed = true;   // k >= 2: the seed bound from an LDS histogram over the first tiles (SMAFA_KTH_HIST_SEED=0: a counting launch)
    uint32_t kth_sample_min_tiles = 4096;  // stores below this many wave tiles (1M subjects) count everything first (SMAFA_KTH_SAMPLE_MIN_TILES)
    uint32_t kth_sample_div = 32;  // ... counting only the first 1/32 of the tiles, the rest counted and appended in one pass (SMAFA_KTH_SAMPLE=0: count everything first)
    uint32_t kth_groups = 0;  // test switch: at most this many tile groups per query chunk when kth_seed_kernel counts a sample (SMAFA_KTH_GROUPS; 0: automatic)
    // rows of a smafa_scan_hits call that ended in SMAFA_ERR_CAPACITY, kept for the caller's "grow and retry":
    // the retry with the same arguments against the same store is answered without scanning again
    std::vector<smafa_hit> retry_rows;
    std::vector<uint8_t> retry_codes;  // the query bytes of that call (compared exactly; the key only screens)
    uint64_t retry_key = 0, retry_nq = 0, generation = 0;  // generation: bumped whenever the subjects change
    uint32_t retry_div = 0, retry_k = 0;
    bool retry_valid = false;
    // ---- block index of the resident store (index.hip.h): built on request (smafa_db_build_index) or on demand (mode 2), tied to
    // the store's state — any append, re-sort or re-plane leaves it stale and the scan kernels run until it is built again
    struct BlockIndex {
        bool valid = false;
        uint64_t generation = 0, n = 0;
        uint32_t resorts = 0, P = 0;
        uint32_t B = 0, dir_bits = 0;
        uint16_t col_begin[kIndexMaxBlocks + 1] = {0};
        uint64_t max_run[kIndexMaxBlocks] = {0};  // longest run of equal keys of block b
        double mean_run[kIndexMaxBlocks] = {0};   // sum(run^2) / n: candidates a query drawn like the store's rows meets there
        double build_ms = 0.0;
        DevBuf kp, dir, stats, rows;
    } index;
    int index_mode = 1;             // 0: never probed; 1: probed where a built index pays; 2: also built by the first scan that could
                                    // use one; 3: ... built once such scans have cost what the build would (SMAFA_INDEX)
    double index_debt_ms = 0.0;     // mode 3: estimated kernel time of the eligible scans since the store last changed
    uint64_t index_debt_generation = 0;
    uint64_t index_failed_generation = 0;  // generation + 1 of the store whose automatic build failed (0: none)
    uint64_t index_max_run = 4096;  // a block whose longest run exceeds this is never probed (SMAFA_INDEX_MAX_RUN)
    double index_cand_per_subject = -1.0;  // candidates per query the probes may expect, per stored subject (SMAFA_INDEX_CAND;
                                           // < 0: by the bound's class — index_cand_limit)
    uint64_t index_min_rows = 65536;  // mode 2 builds an index for stores of at least this many subjects (SMAFA_INDEX_MIN_ROWS)
    uint32_t index_fail_builds = 0;   // tests: the next builds of this handle fail at their sort scratch (SMAFA_INDEX_FAIL_BUILDS)
    uint32_t index_probes = 0;      // launches answered by the index over the handle's life (smafa_index_info)
    // ---- self-join (smafa_db_self_launch, join.hip.h)
    struct JoinState {
        DevBuf pos_of;  // subject number -> position, the inverse of d_order; tied to the store's state like the index
        bool valid = false;
        uint64_t generation = 0, n = 0;
        uint32_t resorts = 0;
        DevBuf out, cnt;  // rows of the host form (smafa_db_self_hits) on their way to the caller, and their counter
        DevBuf parent;    // components (components.hip.h): the union-find's parent[], 4 B per subject, live for one call;
                          // levels (levels.hip.h): one per scanned level, level-major
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // block begin, records done, scan done, filter / link done
        double rec_ms = 0, scan_ms = 0, filter_ms = 0;            // per stage, over the blocks of the last join
        double link_ms = 0, flatten_ms = 0;                       // components: init + link passes, the flatten launch
        uint32_t blocks = 0, rescans = 0;
        // density (density.hip.h): parent holds parent[], degree[] and attach[], 4 B x 3 per subject, live for one call
        DevBuf kept;   // the kept pair list: the rows count_keep_kernel kept, for the one link launch of a one-join call
        DevBuf ctl;    // two uint64: the kept total, and "some row is core"; peaks: four — the kept total, unused, the crown, and
                       // (its low word) the jump rounds' "changed"
        double count_ms = 0;  // density: init + count/keep passes
        uint32_t joins = 0;   // density: how often the store was joined by the last call (0: no scan, 1 or 2)
        bool kept_stuck = false;  // density: growing the kept list failed in this call; it is not tried again
        // peaks (peaks.hip.h): parent holds best[] (8 B per subject) and weight[] (4 B) behind it, live for one call; kept, ctl,
        // count_ms (init + weigh/keep passes), link_ms (the climb), flatten_ms (settle + jump rounds) and joins as for density
        uint32_t jump_rounds = 0;
        // neighbours (neighbours.hip.h): the entry list, 8 B per entry and 4 B more behind them where the sort needs the row apart;
        // its capacity is kept across calls, its contents are not.  ctl[0] is the entry total; parent holds lower[] and the cut
        // degrees, 8 B x 2 per subject, live for one call; filter_ms (pack), count_ms (sort), link_ms (bounds, cut and sum) and
        // flatten_ms (emit)
        DevBuf entries;
        uint64_t entries_cap = 0;  // entries the list has room for
        uint32_t growths = 0;      // how often the last call grew it
        // delta join (delta.hip.h): the subject numbers of the new rows, 4 B each — the order[] of its pieces; ctl[0] counts the
        // labels seed_parents_kernel refused
        DevBuf rows;
        // forest (forest.hip.h): parent holds one union-find, 4 B per subject, live for one call; kept as for density; ctl[0] is the
        // kept total, ctl[1] the running edge total; count_ms (keep passes), link_ms (init + span launches), flatten_ms (the star
        // launch) and joins (1, or 1 + the scanned classes on the slow path)
        // reach forest (reach.hip.h): parent holds the union-find and core[] behind it, 4 B x 2 per subject, live for one call; hist
        // the tallies, 4 B x E per subject, zeroed at the start of every call; kept as for density; ctl[0] is the kept total,
        // ctl[1] the rows that are not sparse, ctl[2] the running edge total; count_ms (tally/keep passes), filter_ms (the cores
        // launch), link_ms (init + span launches), flatten_ms (the star launch) and joins as for the forest
        DevBuf hist;
        // stable clusters (stable.hip.h): the reach forest's state as above, and `stable`, live for one call: the forest's edges
        // and level ends, the root and flag planes (4 B x 2 per subject and plane), kids[], two halves of size[], run[] and sum[]
        // and the chosen total (stable_layout, self_join.hip.h); select_ms: everything behind the reach forest's last pass
        DevBuf stable;
        double select_ms = 0;
        // consensus (consensus.hip.h): `cons`, live for one call: the bad-row word, mark[] and dense[] (4 B x 2 per subject),
        // seg_begin[] and the slots (12 B per group), the records (4 x P x W B per group) and one table of 32 x 32W counters per
        // window of consensus_chunk sorted entries; the sort's double buffers are keys_a / keys_b / idx_a / idx_b (16 B per position).
        // count_ms (groups), filter_ms (keys, sort and bounds), link_ms (tally and vote), flatten_ms (measure and finish)
        DevBuf cons;
        // read-table calls (read_table.hip.h: ReadTable): parent holds best[] (8 B per read), the call's own words, mark[] and its
        // sums (4 B x 2 per read), live for one call; the sort's double buffers are keys_a / keys_b (8 B per read) and idx_a /
        // idx_b (4 B per read).  count_ms (init), link_ms (the best passes), flatten_ms (keys, sort, heads, sums and fold)
        // abundance table (assign.hip.h): no words of its own
        // LCA classification (classify.hip.h): depth[] and ties[] (4 B x 2 per read) between best[] and mark[]; filter_ms (the
        // agree passes)
    } join;
    uint64_t join_block = 65536;    // rows per block of the self-join (SMAFA_JOIN_BLOCK)
    uint64_t join_stride = 16;      // blocks a span of the self-join is dealt into (SMAFA_JOIN_STRIDE; 1: consecutive positions)
    uint64_t join_scratch_max = 1ull << 27;  // rows the block's scratch list may grow to (1.5 GB) before the block is halved (SMAFA_JOIN_SCRATCH_MAX)
    uint64_t density_keep_max = 1ull << 27;  // rows the kept pair list (density and peaks calls) may grow to; 0: never kept, the store is joined
                                             // twice (SMAFA_DENSITY_KEEP_MAX; default: the value of join_scratch_max)
    uint64_t consensus_chunk = 4096;  // sorted entries per wave of consensus::tally_vote_kernel (SMAFA_CONSENSUS_CHUNK)
    uint64_t assign_span = 65536;     // reads per scan of the abundance table (SMAFA_ASSIGN_SPAN)
    uint64_t assign_rows_max = 1ull << 27;  // rows the row list may grow to for one span before the span is halved (SMAFA_ASSIGN_ROWS_MAX;
                                            // default: the value of join_scratch_max)
    bool neighbour_two_sorts = false;  // neighbours: the two-sort order also where one key would hold an entry (SMAFA_NEIGHBOUR_SORT=2, tests)
    bool call_timed = false;        // the last call was a self-join: smafa_last_scan_ms reports the totals over its blocks
    size_t tile_words() const { return (size_t)P * W * kWaveTile; }
    ScanShape shape() const { return {P, PQ, W, L}; }
    uint64_t hits_cap() const { return hits.cap / sizeof(smafa_hit); }
};

namespace smafa {

static int use_device(const smafa_db *db) {
    HIP_TRY(hipSetDevice(db->device));
    return SMAFA_OK;
}

// ---- layout of a store: which source column sits in which packed column, and how each column's codes are re-coded.
// Both leave every distance unchanged (a distance counts columns whose codes differ; neither the order of the columns
// nor a per-column injective renaming of the codes changes that), so they are free parameters of the HBM layout, chosen
// for the prefilter: plane 0 is the plane its lower bounds look at, packed columns 0..31 its first level.
//   * per column, the letters are split into two sets of nearly equal total frequency (greedy, by descending count);
//     the first set gets even codes, the second odd ones: bit 0 of the stored code then flips for a mismatch as often
//     as this column's letter distribution allows.  Nucleotides: A C G T are permuted among 0..3 and N stays 4 (the
//     2-plane form of an N-free store holds bits 0 and 1); of the three A/C/G/T pairings, {A,C}|{G,T} is preferred
//     while it is within 5 % of the best — it is the one that sees transitions, the commonest real substitutions.
//   * columns are ordered by that flip probability, 2p(1-p), best first: conserved columns end up in the last words.
// Decided once per handle, from a sample of the first rows it receives (compute_layout, host/layout.cpp).
static int choose_layout(smafa_db *db, const uint8_t *codes, uint64_t n) {
    compute_layout(db->alphabet, db->L, codes, n, db->perm, db->tab);  // host/layout.cpp
    int rc = db->d_perm.ensure(db->perm.size() * sizeof(uint32_t));
    if (!rc) rc = db->d_tab.ensure(db->tab.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(db->d_perm.p, db->perm.data(), db->perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipMemcpyAsync(db->d_tab.p, db->tab.data(), db->tab.size(), hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));  // the vectors may be reallocated later; the copy is done now
    db->layout_set = true;
    return SMAFA_OK;
}

template <int P>
static void launch_pack(smafa_db *db, const uint8_t *d_codes, const uint32_t *d_src, uint64_t first, uint64_t n,
                        uint32_t *d_out, int mode, uint32_t *d_order) {
    const uint64_t groups = (first + n + 63) / 64 - first / 64;
    const uint32_t blocks = (uint32_t)((groups + kWgWaves - 1) / kWgWaves);
    hipLaunchKernelGGL(pack_rows_kernel<P>, dim3(blocks), dim3(256), 0, db->stream, d_codes, d_src, first, n, db->L, db->W,
                       d_out, mode, db->QS, db->d_perm.as<uint32_t>(), db->d_tab.as<uint8_t>(), d_order);
}

// fold the zone words of tiles [t0, t0 + count) into the store's shared-bit statistics (a re-computed tile replaces its
// earlier entry)
static void note_zone_words(smafa_db *db, uint32_t t0, const uint4 *z, size_t count) {
    if (db->tile_bits.size() < (size_t)t0 + count) db->tile_bits.resize((size_t)t0 + count, 255);
    for (size_t i = 0; i < count; i++) {
        uint8_t &slot = db->tile_bits[t0 + i];
        if (slot != 255) db->zone_hist[slot]--;
        slot = (uint8_t)(__builtin_popcount(z[i].y) + __builtin_popcount(z[i].w));
        db->zone_hist[slot]++;
    }
}

// mean of the shared filter bits over the store's tiles (the probes read it from the level-2 lines)
static double zone_bits_mean(const smafa_db *db) {
    uint64_t tiles = 0, bits = 0;
    for (uint32_t b = 0; b <= 64; b++) tiles += db->zone_hist[b], bits += b * db->zone_hist[b];
    return tiles ? (double)bits / (double)tiles : 0.0;
}

constexpr uint64_t kSortMin = 4096;  // appends of fewer rows keep their order (their tiles share few bits anyway)

// Upload code rows and pack them with the ballot kernel.  mode 0: subjects, at positions first.. of the store — big
// appends are first sorted by their filter words (row_keys_kernel + a device radix sort), so that the subjects of a
// wave tile share their leading filter bits (the zone level of the scan), and the zone words of the touched tiles are
// recomputed; mode 1: query records, in the caller's order.
static int pack_rows(smafa_db *db, const uint8_t *codes, uint64_t first, uint64_t n, uint32_t *d_out, int mode) {
    if (n == 0) return SMAFA_OK;
    if (n > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "too many rows in one call");
    if (!db->layout_set) {
        int lrc = choose_layout(db, codes, mode == 0 ? n : 0);  // a query batch says nothing about the subjects
        if (lrc) return lrc;
    }
    const size_t bytes = (size_t)n * db->L;
    int rc = db->upload.ensure(bytes);
    if (rc) return rc;
    uint8_t *d_codes = db->upload.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(d_codes, codes, bytes, hipMemcpyHostToDevice, db->stream));
    const uint32_t *d_src = nullptr;
    // (the device radix sort counts its items in an int: appends of 2^31 rows and more keep their order)
    const bool sorted = mode == 0 && db->sort_rows && n >= kSortMin && n < (1ull << 31);
    if (sorted) {
        rc = db->keys_a.ensure(n * sizeof(unsigned long long));
        if (!rc) rc = db->keys_b.ensure(n * sizeof(unsigned long long));
        if (!rc) rc = db->idx_a.ensure(n * sizeof(uint32_t));
        if (!rc) rc = db->idx_b.ensure(n * sizeof(uint32_t));
        if (rc) return rc;
        unsigned long long *ka = db->keys_a.as<unsigned long long>(), *kb = db->keys_b.as<unsigned long long>();
        uint32_t *ia = db->idx_a.as<uint32_t>(), *ib = db->idx_b.as<uint32_t>();
        hipLaunchKernelGGL(row_keys_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, db->stream, d_codes, n, db->L,
                           db->d_perm.as<uint32_t>(), db->d_tab.as<uint8_t>(), ka, ia);
        size_t tmp_bytes = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, ka, kb, ia, ib, (int)n, 0, 64, db->stream));
        rc = db->sort_tmp.ensure(tmp_bytes);
        if (rc) return rc;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, tmp_bytes, ka, kb, ia, ib, (int)n, 0, 64, db->stream));
        d_src = ib;
    }
    const uint32_t planes = mode == 0 ? db->P : db->PQ;  // subjects may be stored with fewer planes than queries
    uint32_t *d_order = mode == 0 ? db->d_order : nullptr;
    if (planes == 5) launch_pack<5>(db, d_codes, d_src, first, n, d_out, mode, d_order);
    else if (planes == 3) launch_pack<3>(db, d_codes, d_src, first, n, d_out, mode, d_order);
    else launch_pack<2>(db, d_codes, d_src, first, n, d_out, mode, d_order);
    HIP_TRY(hipGetLastError());
    if (mode == 0) {
        const uint32_t t0 = (uint32_t)(first / kWaveTile), t1 = (uint32_t)((first + n + kWaveTile - 1) / kWaveTile);
        hipLaunchKernelGGL(zone_kernel, dim3((t1 - t0 + kWgWaves - 1) / kWgWaves), dim3(256), 0, db->stream,
                           reinterpret_cast<const uint4 *>(db->d_planes), db->P, db->W, db->L, t0, t1, (uint32_t)(first + n), db->d_zone);
        HIP_TRY(hipGetLastError());
        db->runs.push_back({n, sorted});
        std::vector<uint4> z(t1 - t0);
        HIP_TRY(hipMemcpyAsync(z.data(), db->d_zone + t0, z.size() * sizeof(uint4), hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        note_zone_words(db, t0, z.data(), z.size());
    }
    // the caller's host buffer is borrowed for the call only, and `upload` is reused by the next call
    HIP_TRY(hipStreamSynchronize(db->stream));
    return SMAFA_OK;
}

// A store that grew by many appends — a DB loaded in pieces, cluster's centroid set — is a patchwork of runs that were
// sorted one by one (or not at all, below kSortMin rows): its tiles share far fewer filter bits than a store of that size
// can.  Before a scan, once the rows appended since the last full sort make up a quarter of the store, the whole store is
// sorted again ON THE DEVICE: keys read back from the filter plane, one radix sort, every row moved to its new position
// (planes and order[]), zone words recomputed.  Each re-sort is paid for by the growth since the last one (geometric:
// <= 4 row moves per row over the store's life); subject indices (order[]) do not change, only positions do.
// No room for a second copy of the planes: the store stays as it is.
static int resort_store(smafa_db *db) {
    const uint64_t n = db->n;
    const double t_begin = now_seconds();
    db->rows_since_sort = 0;  // whatever happens below: not again before the store has grown
    int rc = db->keys_a.ensure(n * sizeof(unsigned long long));
    if (!rc) rc = db->keys_b.ensure(n * sizeof(unsigned long long));
    if (!rc) rc = db->idx_a.ensure(n * sizeof(uint32_t));
    if (!rc) rc = db->idx_b.ensure(n * sizeof(uint32_t));
    if (rc) return rc;
    uint32_t *d_new = nullptr, *d_order = nullptr;
    uint4 *d_zone = nullptr;  // the new zone words go to their own buffer: the live ones stay valid until the swap below
    const size_t bytes = db->cap_tiles * db->tile_words() * sizeof(uint32_t);
    const size_t order_bytes = db->cap_tiles * kWaveTile * sizeof(uint32_t);
    const size_t zone_bytes = db->cap_tiles * sizeof(uint4);
    if (hipMalloc(&d_new, bytes) != hipSuccess || hipMalloc(&d_order, order_bytes) != hipSuccess ||
        hipMalloc(&d_zone, zone_bytes) != hipSuccess) {
        (void)hipGetLastError();
        if (d_new) (void)hipFree(d_new);
        if (d_order) (void)hipFree(d_order);
        return SMAFA_OK;
    }
    auto fail = [&](int code) {
        (void)hipFree(d_new);
        (void)hipFree(d_order);
        (void)hipFree(d_zone);
        return code;
    };
    unsigned long long *ka = db->keys_a.as<unsigned long long>(), *kb = db->keys_b.as<unsigned long long>();
    uint32_t *ia = db->idx_a.as<uint32_t>(), *ib = db->idx_b.as<uint32_t>();
    const uint32_t blocks = (uint32_t)((n + 255) / 256);
    hipError_t e = hipMemsetAsync(d_new, 0, bytes, db->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_order, 0, order_bytes, db->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_zone, 0, zone_bytes, db->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(position_keys_kernel, dim3(blocks), dim3(256), 0, db->stream, db->d_planes, db->P, db->W, n, ka, ia);
        e = hipGetLastError();
    }
    size_t tmp_bytes = 0;
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, ka, kb, ia, ib, (int)n, 0, 64, db->stream);
    if (e == hipSuccess && (rc = db->sort_tmp.ensure(tmp_bytes)) != 0) return fail(rc);
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, tmp_bytes, ka, kb, ia, ib, (int)n, 0, 64, db->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(permute_rows_kernel, dim3(blocks), dim3(256), 0, db->stream, db->d_planes, d_new, ib, db->d_order,
                           d_order, n, db->P * db->W);
        e = hipGetLastError();
    }
    const uint32_t n_tiles = (uint32_t)((n + kWaveTile - 1) / kWaveTile);
    std::vector<uint4> z(n_tiles);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(zone_kernel, dim3((n_tiles + kWgWaves - 1) / kWgWaves), dim3(256), 0, db->stream,
                           reinterpret_cast<const uint4 *>(d_new), db->P, db->W, db->L, 0u, n_tiles, (uint32_t)n, d_zone);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(z.data(), d_zone, z.size() * sizeof(uint4), hipMemcpyDeviceToHost, db->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) return fail(set_error(SMAFA_ERR_DEVICE, "re-sorting the store failed: %s", hipGetErrorString(e)));
    // planes, order and zone words change hands together: a failure above leaves the handle exactly as it was
    (void)hipFree(db->d_planes);
    (void)hipFree(db->d_order);
    (void)hipFree(db->d_zone);
    db->d_planes = d_new;
    db->d_order = d_order;
    db->d_zone = d_zone;
    db->tile_bits.clear();
    for (uint64_t &h : db->zone_hist) h = 0;
    note_zone_words(db, 0, z.data(), z.size());
    db->runs.assign(1, {n, true});
    db->resorts++;
    log_line(2, "store of %llu rows sorted again on the device in %.2f ms (re-sort %u)", (unsigned long long)n,
             (now_seconds() - t_begin) * 1e3, db->resorts);
    if (n > (1u << 20))
        for (DevBuf *b : {&db->keys_a, &db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp}) b->release();
    return SMAFA_OK;
}

static int maybe_resort(smafa_db *db) {
    if (!db->sort_rows || !db->resort || db->runs.size() < 2 || db->n < db->resort_min || db->n >= (1ull << 31)) return SMAFA_OK;
    if (db->rows_since_sort * 4 < db->n) return SMAFA_OK;
    return resort_store(db);
}

static int validate_codes(const smafa_db *db, const uint8_t *codes, uint64_t n, uint8_t *max_code = nullptr) {
    const uint8_t lim = db->alphabet == SMAFA_ALPHABET_AA ? 28 : 5;
    const size_t total = (size_t)n * db->L;
    uint8_t worst = 0;
    for (size_t i = 0; i < total; i++) worst = codes[i] > worst ? codes[i] : worst;
    if (worst >= lim) return set_error(SMAFA_ERR_INVALID, "code byte %u outside the alphabet (max %u)", worst, lim - 1);
    if (max_code) *max_code = worst;
    return SMAFA_OK;
}

// 2-plane (N-free) nucleotide store -> 3 planes, in place of the old block
static int upgrade_planes(smafa_db *db, uint32_t p_new) {
    if (db->P >= p_new) return SMAFA_OK;
    if (db->cap_tiles) {
        uint32_t *d_new = nullptr;
        const size_t words = db->cap_tiles * (size_t)p_new * db->W * kWaveTile;
        HIP_TRY(hipMalloc(&d_new, words * sizeof(uint32_t)));
        hipLaunchKernelGGL(replane_kernel, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, db->stream, db->d_planes,
                           d_new, db->cap_tiles, db->P, p_new, db->W);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(db->stream));
        HIP_TRY(hipFree(db->d_planes));
        db->d_planes = d_new;
    }
    db->P = p_new;
    return SMAFA_OK;
}

static int reserve_tiles(smafa_db *db, uint64_t need_tiles) {
    if (need_tiles <= db->cap_tiles) return SMAFA_OK;
    uint64_t ncap = db->cap_tiles ? db->cap_tiles * 2 : 64;
    if (ncap < need_tiles) ncap = need_tiles;
    ncap = (ncap + kWgWaves - 1) / kWgWaves * kWgWaves;
    uint32_t *d_new = nullptr, *d_order = nullptr;
    uint4 *d_zone = nullptr;
    const size_t bytes = ncap * db->tile_words() * sizeof(uint32_t);
    HIP_TRY(hipMalloc(&d_new, bytes));
    HIP_TRY(hipMalloc(&d_order, ncap * kWaveTile * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_zone, ncap * sizeof(uint4)));
    // zero-fill: padding subjects of the last tile read as all-zero planes and are masked by position; a zero zone
    // entry shares no bits (prunes nothing)
    HIP_TRY(hipMemsetAsync(d_new, 0, bytes, db->stream));
    HIP_TRY(hipMemsetAsync(d_order, 0, ncap * kWaveTile * sizeof(uint32_t), db->stream));
    HIP_TRY(hipMemsetAsync(d_zone, 0, ncap * sizeof(uint4), db->stream));
    if (db->d_planes) {
        HIP_TRY(hipMemcpyAsync(d_new, db->d_planes, db->cap_tiles * db->tile_words() * sizeof(uint32_t),
                               hipMemcpyDeviceToDevice, db->stream));
        HIP_TRY(hipMemcpyAsync(d_order, db->d_order, db->cap_tiles * kWaveTile * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                               db->stream));
        HIP_TRY(hipMemcpyAsync(d_zone, db->d_zone, db->cap_tiles * sizeof(uint4), hipMemcpyDeviceToDevice, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        HIP_TRY(hipFree(db->d_planes));
        HIP_TRY(hipFree(db->d_order));
        HIP_TRY(hipFree(db->d_zone));
    }
    db->d_planes = d_new;
    db->d_order = d_order;
    db->d_zone = d_zone;
    db->cap_tiles = ncap;
    return SMAFA_OK;
}

// fill a query set (its buffers grow as needed) from host code rows
static int qset_fill(smafa_qset *qs, smafa_db *db, const uint8_t *query_codes, uint64_t n_queries) {
    qs->db = db;
    qs->nq = n_queries;
    qs->serial = g_qset_serial.fetch_add(1);
    // whole 64-query chunks plus one: a chunk staged by scan_zone_kernel's LDS-DMA is always 64 records from wherever its
    // query block starts (kernels.hip.h, dma()), so up to 63 records past the last query are read (zeros, never used)
    const uint64_t padded = std::max<uint64_t>((n_queries + 63) / 64 * 64, 64) + 64;
    int rc = qs->qrec.ensure(padded * db->QS * sizeof(uint32_t));
    if (!rc) rc = qs->thr.ensure(padded * sizeof(uint32_t));
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(qs->qrec.p, 0, padded * db->QS * sizeof(uint32_t), db->stream));
    return pack_rows(db, query_codes, 0, n_queries, qs->qrec.as<uint32_t>(), 1);
}

// remember which instantiation ran, spelled the way rocprofv3 lists it, and add it to the call's list (first launch only)
static void note_call_kernel(const smafa_db *db, const char *name) {
    auto &names = const_cast<smafa_db *>(db)->call_kernels;
    if (std::find(names.begin(), names.end(), name) == names.end()) names.emplace_back(name);
}
static void note_kernel(const smafa_db *db, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void note_kernel(const smafa_db *db, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(const_cast<smafa_db *>(db)->plan_kernel, sizeof db->plan_kernel, fmt, ap);
    va_end(ap);
    note_call_kernel(db, db->plan_kernel);
}

template <int N>
using ic = std::integral_constant<int, N>;

// The twelve (PS, PQ, W) shapes the per-shape kernels are instantiated for: fn(ic<PS>, ic<PQ>, ic<W>) for the store's shape, and
// what it returns; false without a call where the store has no such shape (more than four words per plane).
template <class F>
static bool for_shape(const ScanShape &s, F &&fn) {
    auto by_words = [&](auto ps, auto pq) {
        return s.W == 1 ? fn(ps, pq, ic<1>{}) : s.W == 2 ? fn(ps, pq, ic<2>{}) : s.W == 3 ? fn(ps, pq, ic<3>{}) : s.W == 4 && fn(ps, pq, ic<4>{});
    };
    if (s.P == 2 && s.PQ == 3) return by_words(ic<2>{}, ic<3>{});
    if (s.P == 3 && s.PQ == 3) return by_words(ic<3>{}, ic<3>{});
    return s.P == 5 && s.PQ == 5 && by_words(ic<5>{}, ic<5>{});
}

// Launch the plan's instantiation.  Every choice was made by plan_scan (scan_plan.h); the branches below only spell the
// instantiations the binary holds — tests/test_kernel_census.py counts them, so a guard that is too wide fails there.
// false: the plan names an instantiation that does not exist.
static bool launch_scan(const smafa_db *db, const uint32_t *d_qrec, const ScanArgs &a, uint32_t grid, const ScanPlan &plan) {
    const uint4 *planes = reinterpret_cast<const uint4 *>(db->d_planes);
    auto go = [&](auto kernel, int block, auto... more) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, db->stream, planes, d_qrec, a, more...);
        return true;
    };
    const bool seed = plan.seed;
    if (plan.family == ScanFamily::generic) return go(scan_generic_kernel, 256, db->P, db->PQ, db->W, db->QS);
    if (plan.family == ScanFamily::wide) {  // above 128 columns, or up to 32 (SMAFA_WIDE_FROM=3: from 65); one instantiation per plane pair
        auto wide = [&](auto ps, auto pq, auto fw, auto wc) {
            constexpr int PS = decltype(ps)::value, PQ = decltype(pq)::value, FW = decltype(fw)::value, WC = decltype(wc)::value;
            return plan.fw == (uint32_t)FW && plan.wc == (uint32_t)WC &&
                   (seed ? go(scan_wide_kernel<PS, PQ, true, FW, WC>, 256, db->W) : go(scan_wide_kernel<PS, PQ, false, FW, WC>, 256, db->W));
        };
        auto planes_of = [&](auto ps, auto pq) {
            return wide(ps, pq, ic<1>{}, ic<0>{}) || wide(ps, pq, ic<3>{}, ic<0>{}) || wide(ps, pq, ic<3>{}, ic<3>{}) || wide(ps, pq, ic<3>{}, ic<4>{});
        };
        return db->P == 2 ? planes_of(ic<2>{}, ic<3>{}) : db->P == 3 ? planes_of(ic<3>{}, ic<3>{}) : planes_of(ic<5>{}, ic<5>{});
    }
    return for_shape(db->shape(), [&](auto ps, auto pq, auto w) {
        constexpr int PS = decltype(ps)::value, PQ = decltype(pq)::value, W = decltype(w)::value;
        switch (plan.family) {
        case ScanFamily::zone_few:
            return go(scan_zone_few_kernel<PS, PQ, W>, 256);
        case ScanFamily::zone:
            return plan.direct  ? go(scan_zone_kernel<PS, PQ, W, true, true>, kZoneWgWaves * 64)
                   : plan.fixed ? go(scan_zone_kernel<PS, PQ, W, true, false>, kZoneWgWaves * 64)
                                : go(scan_zone_kernel<PS, PQ, W, false, false>, kZoneWgWaves * 64);
        case ScanFamily::lazy: {
            constexpr int T = W <= 2 ? 4 : 2;  // the only tile count of this shape
            if (plan.T != (uint32_t)T) return false;
            if (seed) return go(scan_lazy_kernel<PS, PQ, W, T, true, false>, 256);
            if constexpr (W == 2) {  // SUMFOLD exists for two words per plane
                if (plan.sumfold) return go(scan_lazy_kernel<PS, PQ, W, T, false, true>, 256);
            }
            return go(scan_lazy_kernel<PS, PQ, W, T, false, false>, 256);
        }
        case ScanFamily::scan: {
            auto tiles = [&](auto t) {  // FOLD 1 to 3 exist for two words per plane, 2 from three planes on, 3 from four
                constexpr int T = decltype(t)::value;
                if (seed) return go(scan_kernel<PS, PQ, W, T, true, 0>, 256);
                if constexpr (W == 2) {
                    if (plan.fold == 1) return go(scan_kernel<PS, PQ, W, T, false, 1>, 256);
                    if constexpr (PS >= 3) {
                        if (plan.fold == 2) return go(scan_kernel<PS, PQ, W, T, false, 2>, 256);
                    }
                    if constexpr (PS >= 4) {
                        if (plan.fold == 3) return go(scan_kernel<PS, PQ, W, T, false, 3>, 256);
                    }
                }
                return plan.fold == 0 && go(scan_kernel<PS, PQ, W, T, false, 0>, 256);
            };
            if (plan.T == 1) return tiles(ic<1>{});  // one tile per wave everywhere, two up to two words, four for two planes of those
            if constexpr (W <= 2) {
                if (plan.T == 2) return tiles(ic<2>{});
                if constexpr (PS == 2) {
                    if (plan.T == 4) return tiles(ic<4>{});
                }
            }
            return false;
        }
        default:
            return false;
        }
    });
}

// ---------------------------------------------------------------------------------------------
// The block index (index.hip.h).
static bool index_current(const smafa_db *db) {
    const auto &ix = db->index;
    return ix.valid && ix.generation == db->generation && ix.n == db->n && ix.resorts == db->resorts && ix.P == db->P;
}

static void index_drop(smafa_db *db) {
    db->index.valid = false;
    for (DevBuf *b : {&db->index.kp, &db->index.dir, &db->index.stats, &db->index.rows}) b->release();
}

static int index_build_steps(smafa_db *db, uint32_t blocks) {
    auto &ix = db->index;
    ix.valid = false;
    if (db->W > (uint32_t)kIndexMaxWords)
        return set_error(SMAFA_ERR_INVALID, "the block index takes rows of up to %d columns (this store: %u)", kIndexMaxWords * 32, db->L);
    if (blocks < 1 || blocks > (uint32_t)kIndexMaxBlocks || blocks > db->L)
        return set_error(SMAFA_ERR_INVALID, "the block index takes 1..%u blocks for this store (asked: %u)",
                         std::min<uint32_t>(kIndexMaxBlocks, db->L), blocks);
    if (db->n == 0 || db->n >= (1ull << 31)) return set_error(SMAFA_ERR_INVALID, "the block index takes 1..2^31-1 subjects");
    int rc = use_device(db);
    if (rc) return rc;
    rc = maybe_resort(db);  // (positions are final afterwards: an index built before a due re-sort would be stale at once)
    if (rc) return rc;
    const double t_begin = now_seconds();
    const uint32_t n = (uint32_t)db->n;
    uint32_t dir_bits = 8;
    while (dir_bits < 22 && (1ull << (dir_bits + 2)) < n) dir_bits++;
    const size_t dir_entries = ((size_t)1 << dir_bits) + 1;
    const size_t row_bytes = (size_t)index_row_vectors((int)db->P, (int)db->W) * sizeof(uint4);
    rc = ix.kp.ensure((size_t)blocks * n * sizeof(uint2));
    if (!rc) rc = ix.rows.ensure((size_t)n * row_bytes);
    if (!rc) rc = ix.dir.ensure((size_t)blocks * dir_entries * sizeof(uint32_t));
    if (!rc) rc = ix.stats.ensure((size_t)kIndexMaxBlocks * 2 * sizeof(unsigned long long));
    // (SMAFA_INDEX_FAIL_BUILDS, tests: a size no device has — hipMalloc says out of memory at once, as where HBM has run out)
    const bool fail = db->index_fail_builds > 0;
    if (fail) db->index_fail_builds--;
    if (!rc) rc = db->keys_a.ensure(fail ? (size_t)1 << 60 : (size_t)n * sizeof(uint32_t));
    if (!rc) rc = db->keys_b.ensure((size_t)n * sizeof(uint32_t));
    if (!rc) rc = db->idx_a.ensure((size_t)n * sizeof(uint32_t));
    if (!rc) rc = db->idx_b.ensure((size_t)n * sizeof(uint32_t));
    if (rc) return rc;
    uint32_t *ka = db->keys_a.as<uint32_t>(), *ia = db->idx_a.as<uint32_t>();
    uint32_t *kb = db->keys_b.as<uint32_t>(), *ib = db->idx_b.as<uint32_t>();
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, ka, kb, ia, ib, (int)n, 0, 32, db->stream));
    rc = db->sort_tmp.ensure(tmp_bytes);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ix.stats.p, 0, (size_t)kIndexMaxBlocks * 2 * sizeof(unsigned long long), db->stream));
    const uint32_t grid = (n + 255u) / 256u;
    for (uint32_t b = 0; b <= blocks; b++) ix.col_begin[b] = (uint16_t)((uint64_t)b * db->L / blocks);
    hipLaunchKernelGGL(index_rows_kernel, dim3(grid), dim3(256), 0, db->stream, db->d_planes, db->P, db->W, n, ix.rows.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    for (uint32_t b = 0; b < blocks; b++) {
        hipLaunchKernelGGL(index_keys_kernel, dim3(grid), dim3(256), 0, db->stream, db->d_planes, db->P, db->W, n,
                           (uint32_t)ix.col_begin[b], (uint32_t)ix.col_begin[b + 1], ka, ia);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(db->sort_tmp.p, tmp_bytes, ka, kb, ia, ib, (int)n, 0, 32, db->stream));
        hipLaunchKernelGGL(index_dir_kernel, dim3((uint32_t)((dir_entries + 255) / 256)), dim3(256), 0, db->stream, kb, n, dir_bits,
                           ix.dir.as<uint32_t>() + (size_t)b * dir_entries);
        hipLaunchKernelGGL(index_stats_kernel, dim3(std::min<uint32_t>(grid, 2048u)), dim3(256), 0, db->stream, kb, n,
                           ix.stats.as<unsigned long long>() + (size_t)b * 2);
        hipLaunchKernelGGL(index_interleave_kernel, dim3(grid), dim3(256), 0, db->stream, kb, ib, n, ix.kp.as<uint2>() + (size_t)b * n);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long st[kIndexMaxBlocks * 2] = {0};
    HIP_TRY(hipMemcpyAsync(st, ix.stats.p, (size_t)blocks * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    for (uint32_t b = 0; b < blocks; b++) {
        ix.max_run[b] = st[2 * b];
        ix.mean_run[b] = (double)st[2 * b + 1] / (double)n;
    }
    ix.B = blocks;
    ix.dir_bits = dir_bits;
    ix.generation = db->generation;
    ix.n = db->n;
    ix.resorts = db->resorts;
    ix.P = db->P;
    ix.build_ms = (now_seconds() - t_begin) * 1e3;
    ix.valid = true;
    if (n > (1u << 20))
        for (DevBuf *b : {&db->keys_a, &db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp}) b->release();
    log_line(2, "block index of %u rows: %u blocks, %.1f MB, built on the device in %.2f ms", n, blocks,
             (double)(ix.kp.cap + ix.dir.cap + ix.rows.cap) / 1e6, ix.build_ms);
    return SMAFA_OK;
}

// Build (or rebuild) the index with `blocks` blocks: serves every fixed bound up to blocks - 1.
// A build that fails leaves nothing behind: the runtime keeps a failed hipMalloc as the thread's last error until somebody
// reads it — the next launch's HIP_TRY(hipGetLastError()) would take it for its own, and the scan that was to fall back to the
// scan kernels would fail with the build's error — and the sort scratch, 16 bytes per subject and more, is given back.
static int index_build(smafa_db *db, uint32_t blocks) {
    const int rc = index_build_steps(db, blocks);
    if (rc) {
        (void)hipGetLastError();
        for (DevBuf *b : {&db->keys_a, &db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp}) b->release();
    }
    return rc;
}

// Candidates per query the probes of a scan with this bound may expect before the scan kernels are the better choice.
// Measured on 10M-subject stores (profiles/r04_index.txt): a candidate costs ~0.025 ns (its row of the index's row-major copy,
// one or two cache lines; gathered from the bit-planes it was 0.18 ns for 60 amino-acid columns).  A scanned subject costs the
// batched kernels, per query: the zone kernel ~8e-14 s x the share of (query, tile) pairs that pass the zone level (level 1
// over the tile for each of them: aa bound 5, share 0.2: 1.7e-14 s; bound 3: 3.7e-15; nt bound 3, share 0.025: 2.9e-15; bound 7:
// 5.3e-14), the filter-plane-resident kernel at the bounds its folds reject 8e-14 s (aa 8..12, nt 9), the all-planes forms
// 1.2e-13 s and more.  The candidates allowed are 0.45 of break-even — queries are not spread like the store's own rows — and an
// underestimate of the scan only leaves a scan where the index would have been faster.
static double index_cand_limit(const smafa_db *db, uint32_t thr0) {
    double per_subject = db->index_cand_per_subject;
    if (per_subject < 0.0) {
        const ScanShape shape = db->shape();
        const bool prunes = prefilter_prunes(shape, db->knobs, thr0);
        // (two-word amino-acid stores: the zone kernel's key test cuts its time per pass-share to ~0.3 of that, 2.4e-14 —
        // 10M x 10k bound 5: 1.69 -> 0.56 ms, profiles/r05_zone_keys.txt, -> 0.50 ms with the key work hoisted per chunk,
        // profiles/r06_zone_hoist.txt; nucleotides at bound 3: 2.69 -> 2.54 ms, kept at 8e-14)
        const double zone_s = db->W == 2 && db->alphabet == SMAFA_ALPHABET_AA ? 2.4e-14 : 8e-14;
        // (up to 128 columns: scan_zone_kernel; longer stores have the zone level inside scan_wide_kernel, not counted here)
        const bool zone = db->W <= 4 && zone_pays(shape, db->knobs, thr0, prunes, {db->zone_hist});
        const double scan_s = zone ? zone_s * std::min(1.0, std::max(0.02, zone_pass_share(db->zone_hist, thr0)))
                              : fold_rejects(shape, db->knobs, thr0) || prunes ? 8e-14
                                                                               : 1.2e-13;
        per_subject = 0.45 * scan_s / 0.025e-9;
    }
    return std::max(16.0, per_subject * (double)db->n);
}

// Which blocks a fixed-bound scan would probe, and whether that beats the scan kernels: bound + 1 blocks out of the usable
// ones (longest run within index_max_run), the ones with the fewest expected candidates.
static bool index_plan(const smafa_db *db, uint32_t thr0, uint32_t nq, uint8_t *probe_block) {
    const auto &ix = db->index;
    if (!db->index_mode || !db->knobs.use_filter || !index_current(db) || nq <= 64u || thr0 + 1u > ix.B) return false;
    uint8_t usable[kIndexMaxBlocks];
    uint32_t nu = 0;
    for (uint32_t b = 0; b < ix.B; b++)
        if (ix.max_run[b] <= db->index_max_run) usable[nu++] = (uint8_t)b;
    if (nu < thr0 + 1u) return false;
    std::sort(usable, usable + nu, [&](uint8_t x, uint8_t y) { return ix.mean_run[x] < ix.mean_run[y] || (ix.mean_run[x] == ix.mean_run[y] && x < y); });
    double expected = 0.0;
    for (uint32_t j = 0; j <= thr0; j++) expected += ix.mean_run[usable[j]];
    if (expected > index_cand_limit(db, thr0)) return false;
    for (uint32_t j = 0; j <= thr0; j++) probe_block[j] = usable[j];
    return true;
}

static int index_probe(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t thr0, const uint8_t *probe_block,
                       smafa_hit *d_rows, uint64_t rows_cap, unsigned long long *d_count) {
    const auto &ix = db->index;
    IndexArgs x;
    x.kp = ix.kp.as<uint2>();
    x.rows = ix.rows.as<uint4>();
    x.dir = ix.dir.as<uint32_t>();
    x.n = (uint32_t)ix.n;
    x.dir_bits = ix.dir_bits;
    x.n_probes = thr0 + 1u;
    x.bound = thr0;
    x.L = db->L;
    x.QS = db->QS;
    for (uint32_t j = 0; j < (uint32_t)kIndexMaxBlocks; j++) {
        x.probe_block[j] = j <= thr0 ? probe_block[j] : 0;
        x.probe_cols[j] = (uint32_t)ix.col_begin[x.probe_block[j]] | ((uint32_t)ix.col_begin[x.probe_block[j] + 1] << 16);
    }
    ScanArgs a{};
    a.n_subjects = (uint32_t)db->n;
    a.hits = d_rows;
    a.cap = rows_cap;
    a.count = d_count;  // zeroed by the caller; rows are reserved straight from it and it IS the result
    a.order = db->d_order;
    int cur_dev = -1;
    if (hipGetDevice(&cur_dev) == hipSuccess) {
        db->launch_device = cur_dev;
        if (cur_dev != db->device) db->launches_off_device++;
    }
    const uint32_t *qrec = qs->qrec.as<uint32_t>();
    // One dispatch holds fewer than 2^32 work-items (its grid size is 32 bits: a launch of 2^32 + 2^23 of them probed only the
    // first queries, with no error), and the kernel numbers its (query, probe) groups from a 32-bit thread index: a batch of
    // more than 2^31 / kIndexGroup groups is probed in query ranges that each stay below that (rows go to one list).
    const uint32_t per_launch = (uint32_t)((1ull << 31) / kIndexGroup / x.n_probes);
    for (uint32_t qb = q_begin; qb < q_end;) {
        const uint32_t qe = q_end - qb > per_launch ? qb + per_launch : q_end;
        x.q_begin = qb;
        x.q_end = qe;
        const uint64_t groups = (uint64_t)(qe - qb) * x.n_probes;
        const uint64_t grid = (groups * kIndexGroup + kIndexWg - 1u) / kIndexWg;
        const bool launched = for_shape(db->shape(), [&](auto ps, auto pq, auto w) {
            constexpr int PS = decltype(ps)::value, PQ = decltype(pq)::value, W = decltype(w)::value;
            hipLaunchKernelGGL((index_probe_kernel<PS, PQ, W>), dim3((uint32_t)grid), dim3(kIndexWg), 0, db->stream, db->d_planes, qrec, x, a);
            note_kernel(db, "smafa::index_probe_kernel<%d, %d, %d>", PS, PQ, W);
            return true;
        });
        if (!launched) return set_error(SMAFA_ERR_INVALID, "no index probe for %u/%u planes x %u words", db->P, db->PQ, db->W);
        HIP_TRY(hipGetLastError());
        db->last_launches++;
        qb = qe;
    }
    db->plan_lazy = 0;
    db->plan_tiles = 0;
    db->plan_qblocks = 1;
    db->index_probes++;
    return SMAFA_OK;
}

// one kernel launch: queries [q_begin, q_end) x wave tiles [tile_begin, tile_end).  Rows go to `d_rows` (room for
// `rows_cap`) through the handle's counter; publish != NULL: the launch is the whole scan — its last workgroup writes the
// row total to *publish and leaves the counters at zero.
static int launch_tiles(smafa_db *db, smafa_qset *qs, uint32_t q_begin, uint32_t q_end, uint32_t tile_begin,
                        uint32_t tile_end, uint32_t k_tight, uint32_t thr0, smafa_hit *d_rows, uint64_t rows_cap,
                        unsigned long long *publish, bool per_query_bounds = false, unsigned long long *own_counter = nullptr) {
    ScanArgs a;
    const uint32_t nq = q_end - q_begin, n_tiles = tile_end - tile_begin;
    const bool per_query = k_tight || per_query_bounds;
    // which kernel, how many tiles per wave and waves per workgroup: decided once, in scan_plan.h
    const ScanPlan plan = plan_scan(db->shape(), db->knobs, {thr0, nq, d_rows == nullptr && k_tight == 1, d_rows != nullptr, per_query, {db->zone_hist}});
    const uint32_t T = plan.T;
    a.tile_begin = tile_begin;
    a.tile_end = tile_end;
    a.n_wg_tiles = (n_tiles + plan.wg_waves * T - 1) / (plan.wg_waves * T);
    a.n_subjects = (uint32_t)db->n;
    a.q_begin = q_begin;
    a.q_end = q_end;
    // queries per workgroup pass (query_block_size, engine.h).  (The block size is chosen per 4-wave share of the store whatever
    // the workgroup size, so that it does not change with kZoneWgWaves: profiles/r02_zone_variants.txt)
    a.qb_size = query_block_size(db->qb_override, (uint32_t)db->n_cu, (n_tiles + kWgWaves * T - 1) / (kWgWaves * T), nq,
                                 plan.whole_chunks ? (uint32_t)kChunk : 1u);
    // fixed common bound: no per-query array, no fill launch; per_query_bounds: fixed bounds read from thr
    a.thr = per_query ? qs->thr.as<uint32_t>() : nullptr;
    a.thr0 = thr0;
    a.cnt = qs->cnt.as<uint32_t>();
    a.cnt_stride = db->L + 1;
    a.k_tight = k_tight;
    a.use_filter = db->knobs.use_filter ? 1u : 0u;
    a.hits = d_rows;
    a.cap = rows_cap;
    a.count = db->ctrs.as<unsigned long long>();
    a.done = publish ? reinterpret_cast<uint32_t *>(db->ctrs.as<uint8_t>() + 256) : nullptr;
    a.publish = publish;
    if (own_counter) {  // the caller zeroed a counter of its own for this launch: rows are reserved from it and it IS the result —
        a.count = own_counter;  // nobody takes a ticket (smafa_scan_each: a workgroup's returning ticket atomic at the end of
        a.done = nullptr;       // a one-query pass cost the streaming form 13 % — profiles/r03_stream_nt.txt)
        a.publish = nullptr;
    }
    a.order = db->d_order;
    a.zone = db->d_zone;
    a.zone_on = plan.zone_on ? 1u : 0u;
    // the key sets of scan_zone_kernel<.., DIRECT> (two-word stores): X and Z split filter word 1's L - 32 columns, KB each where
    // they fit (60 columns, KB = 12: X = columns 32..43, Z = 44..55); Y, word 0's last KB columns, is fixed
    {
        const uint32_t n1 = db->L > 32u ? std::min(db->L - 32u, 32u) : 0u, kb = (uint32_t)SMAFA_ZONE_KEY_BITS;
        const uint32_t xw = n1 >= 2u * kb ? kb : n1 / 2u;
        a.key_xmask = xw ? (uint32_t)((1ull << xw) - 1ull) : 0u;
        a.key_zlo = xw;
        a.key_gate = db->zone_key_gate >= 0                  ? (uint32_t)db->zone_key_gate
                     : db->alphabet == SMAFA_ALPHABET_AA ? (uint32_t)SMAFA_ZONE_KEY_GATE
                                                         : (uint32_t)SMAFA_ZONE_KEY_GATE_NT;
    }
    const uint64_t n_qblocks = (q_end - q_begin + a.qb_size - 1) / a.qb_size;
    // non-temporal loads (scan_lazy_kernel's filter words, scan_kernel's tiles): where a cached copy is never read again — one
    // query block, or more bytes per query block than the 256 MiB Infinity Cache holds until the next one comes round
    // (bytes one query block reads: the filter plane's words for the filter-plane-resident kernels, whole tiles for scan_kernel)
    const uint64_t range_bytes = (uint64_t)n_tiles * (plan.reported_lazy ? db->W : db->P * db->W) * 1024u;
    a.stream_once = (db->stream_nt && (n_qblocks == 1 || range_bytes >= (256ull << 20))) ? 1u : 0u;
    const uint64_t grid = n_qblocks * a.n_wg_tiles;
    if (grid > 0x7fffffffull)
        return set_error(SMAFA_ERR_INVALID, "scan grid too large (%llu workgroups)", (unsigned long long)grid);
    int cur_dev = -1;
    if (hipGetDevice(&cur_dev) == hipSuccess) {
        db->launch_device = cur_dev;
        if (cur_dev != db->device) db->launches_off_device++;
    }
    const std::string id = scan_kernel_name(plan, db->shape());
    note_kernel(db, "%s", id.c_str());
    // (the call's list names scan_wide_kernel's zone-level form as a marker of its own, after the template-id)
    if (plan.zone_on) note_kernel(db, "%s (zone level on)", id.c_str());
    if (!launch_scan(db, qs->qrec.as<uint32_t>(), a, (uint32_t)grid, plan)) return set_error(SMAFA_ERR_INVALID, "no kernel %s", id.c_str());
    db->plan_lazy = plan.reported_lazy ? 1u : 0u;
    db->plan_tiles = T;
    db->plan_qblocks = (uint32_t)n_qblocks;
    HIP_TRY(hipGetLastError());
    db->last_launches++;
    return SMAFA_OK;
}

// ---------------------------------------------------------------------------------------------
#include "scan_host.hip.h"  // one scan of a resident set (scan_range), rows to the host, the host-buffer call (scan_to_host)
#include "self_join.hip.h"  // the self-join: its two drivers and the calls that consume their pieces

void db_life_stats(const smafa_db *db, double *kernel_ms, uint64_t *launches) {
    *kernel_ms = db ? db->life_ms : 0.0;
    *launches = db ? db->life_launches : 0;
}

void warm_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return;
    if (hipSetDevice(device) != hipSuccess) return;
    (void)hipFree(nullptr);  // forces the context
}

// Rows past n in the last tile keep their old bits; every kernel tests subject < n_subjects before it reports or
// tightens a bound, exactly as it does for the zero padding of a fresh store.
int db_clear(smafa_db *db) {
    if (!db) return set_error(SMAFA_ERR_INVALID, "db_clear: NULL handle");
    db->n = 0;
    db->runs.clear();
    db->rows_since_sort = 0;
    db->tile_bits.clear();
    for (uint64_t &h : db->zone_hist) h = 0;
    db->generation++;
    return SMAFA_OK;
}

// A handle whose HBM image is a mapped packed store file: no decode, no pack kernel — three copies.
int db_load_packed(smafa_db **out, int device, const PackedStore &pk) {
    if (!out) return set_error(SMAFA_ERR_INVALID, "db_load_packed: out is NULL");
    int rc = smafa_db_create(out, device, (int)pk.h.alphabet, pk.h.seq_len);
    if (rc) return rc;
    smafa_db *db = *out;
    auto fail = [&](int code) {
        smafa_db_destroy(db);
        *out = nullptr;
        return code;
    };
    db->P = pk.h.planes;
    db->perm.assign(pk.perm, pk.perm + (size_t)db->W * 32);
    db->tab.assign(pk.tab, pk.tab + (size_t)db->L * 32);
    rc = db->d_perm.ensure(db->perm.size() * sizeof(uint32_t));
    if (!rc) rc = db->d_tab.ensure(db->tab.size());
    if (rc) return fail(rc);
    hipError_t e = hipMemcpyAsync(db->d_perm.p, db->perm.data(), db->perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db->d_tab.p, db->tab.data(), db->tab.size(), hipMemcpyHostToDevice, db->stream);
    db->layout_set = true;
    if (e == hipSuccess && pk.h.n > 0) {
        rc = reserve_tiles(db, pk.h.n_tiles);
        if (rc) return fail(rc);
        e = hipMemcpyAsync(db->d_planes, pk.planes, pk.h.n_tiles * db->tile_words() * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(db->d_order, pk.order, pk.h.n_tiles * kWaveTile * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream);
        // The zone words are recomputed from the planes, not taken from the file: a scan skips tiles on their say-so, and
        // a damaged copy would lose rows silently (the file's copy serves host-side readers).  One pass over the filter
        // plane: 20 us at 10M rows.
        std::vector<uint4> z(pk.h.n_tiles);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(zone_kernel, dim3((uint32_t)((pk.h.n_tiles + kWgWaves - 1) / kWgWaves)), dim3(256), 0, db->stream,
                               reinterpret_cast<const uint4 *>(db->d_planes), db->P, db->W, db->L, 0u, (uint32_t)pk.h.n_tiles,
                               (uint32_t)pk.h.n, db->d_zone);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(z.data(), db->d_zone, z.size() * sizeof(uint4), hipMemcpyDeviceToHost, db->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
        if (e == hipSuccess) note_zone_words(db, 0, z.data(), z.size());
    }
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) return fail(set_error(SMAFA_ERR_DEVICE, "loading the packed store failed: %s", hipGetErrorString(e)));
    db->n = pk.h.n;
    for (uint64_t r = 0; r < pk.h.n_runs; r++) db->runs.push_back({pk.runs[2 * r], pk.runs[2 * r + 1] != 0});
    db->rows_since_sort = pk.h.n_runs > 1 ? pk.h.n : 0;  // a file saved from a patchwork store: sorted at the first scan
    db->generation++;
    return SMAFA_OK;
}

}  // namespace smafa

// ------------------------------------------------------------------------------------- C ABI
extern "C" {

int smafa_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} catch (...) {
    return smafa::exception_code("smafa_device_count");
}

int smafa_db_create(smafa_db **out, int device, int alphabet, uint32_t seq_len) try {
    if (!out) return set_error(SMAFA_ERR_INVALID, "smafa_db_create: out is NULL");
    *out = nullptr;
    if (alphabet != SMAFA_ALPHABET_NT && alphabet != SMAFA_ALPHABET_AA)
        return set_error(SMAFA_ERR_INVALID, "unknown alphabet %d", alphabet);
    if (seq_len == 0) return set_error(SMAFA_ERR_PANIC, "Cannot add empty sequence to WindowSet");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return set_error(SMAFA_ERR_DEVICE, "no HIP device visible: the smafa scan engine has no CPU fallback");
    if (device < 0 || device >= ndev) return set_error(SMAFA_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    smafa_db *db = new smafa_db();
    db->device = device;
    db->alphabet = alphabet;
    db->L = seq_len;
    db->PQ = (uint32_t)query_planes_for(alphabet);
    // nucleotide stores start in the 2-bit form (A C G T only) and gain the N plane when an N is appended
    db->P = alphabet == SMAFA_ALPHABET_NT ? 2u : db->PQ;
    if (const char *pv = getenv("SMAFA_NT_PLANES")) {  // testing: force the 3-plane store
        if (alphabet == SMAFA_ALPHABET_NT && atoi(pv) == 3) db->P = 3;
    }
    db->W = (seq_len + 31) / 32;
    db->QS = (uint32_t)qrec_stride((int)db->PQ, (int)db->W);
    if (const char *fv = getenv("SMAFA_FILTER")) db->knobs.use_filter = atoi(fv) != 0;
    if (const char *tv = getenv("SMAFA_TILES")) {
        const int t = atoi(tv);
        db->knobs.tiles_override = (t == 1 || t == 2 || t == 4) ? (uint32_t)t : 0u;
    }
    if (const char *lv = getenv("SMAFA_LAZY")) db->knobs.lazy = atoi(lv) != 0;
    if (const char *pv2 = getenv("SMAFA_TWO_PHASE")) db->two_phase = atoi(pv2) != 0;
    if (const char *f3 = getenv("SMAFA_FOLD3")) db->knobs.fold3 = atoi(f3) != 0;
    if (const char *sn = getenv("SMAFA_STREAM_NT")) db->stream_nt = atoi(sn) != 0;
    if (const char *cv = getenv("SMAFA_COUNT_FIRST_K")) db->count_first_k = (uint32_t)std::max(2, atoi(cv));
    if (const char *lp = getenv("SMAFA_LADDER_PROBE")) db->ladder_probe = atoi(lp) != 0;
    if (const char *zd = getenv("SMAFA_ZONE_DIRECT")) db->knobs.zone_direct = atoi(zd) != 0;
    if (const char *kg = getenv("SMAFA_ZONE_KEY_GATE")) db->zone_key_gate = std::min(65, std::max(0, atoi(kg)));
    if (const char *lf = getenv("SMAFA_LAZY_FOLD")) db->knobs.lazy_fold = atoi(lf) != 0;
    if (const char *ks = getenv("SMAFA_KTH_HIST_SEED")) db->kth_hist_seed = atoi(ks) != 0;
    if (const char *ks = getenv("SMAFA_KTH_SAMPLE")) db->kth_sample_div = (uint32_t)std::max(0, atoi(ks));
    if (const char *ks = getenv("SMAFA_KTH_SAMPLE_MIN_TILES")) db->kth_sample_min_tiles = (uint32_t)std::max(1, atoi(ks));
    if (const char *ks = getenv("SMAFA_KTH_GROUPS")) db->kth_groups = (uint32_t)std::max(0, atoi(ks));
    if (const char *ov = getenv("SMAFA_WIDE_ONE")) db->knobs.wide_one = atoi(ov) != 0;
    if (const char *wv = getenv("SMAFA_WIDE_FROM")) db->knobs.wide_from = (uint32_t)std::max(3, atoi(wv));
    if (const char *zv = getenv("SMAFA_ZONE")) db->knobs.zone = std::min(2, std::max(0, atoi(zv)));
    if (const char *sv = getenv("SMAFA_SORT")) db->sort_rows = atoi(sv) != 0;
    if (const char *sv = getenv("SMAFA_RESORT")) db->resort = atoi(sv) != 0;
    if (const char *sv = getenv("SMAFA_PRUNE_P")) db->knobs.prune_p = atof(sv);
    if (const char *sv = getenv("SMAFA_RESORT_MIN")) db->resort_min = std::max<uint64_t>(2, strtoull(sv, nullptr, 10));
    if (const char *zl = getenv("SMAFA_ZONE_LOOSE")) db->knobs.zone_loose = atof(zl);
    if (const char *iv = getenv("SMAFA_INDEX")) db->index_mode = std::min(3, std::max(0, atoi(iv)));
    if (const char *iv = getenv("SMAFA_INDEX_MAX_RUN")) db->index_max_run = std::max<uint64_t>(1, strtoull(iv, nullptr, 10));
    if (const char *iv = getenv("SMAFA_INDEX_CAND")) db->index_cand_per_subject = atof(iv);
    if (const char *iv = getenv("SMAFA_INDEX_MIN_ROWS")) db->index_min_rows = std::max<uint64_t>(1, strtoull(iv, nullptr, 10));
    if (const char *iv = getenv("SMAFA_INDEX_FAIL_BUILDS")) db->index_fail_builds = (uint32_t)std::max(0, atoi(iv));
    if (const char *jv = getenv("SMAFA_JOIN_BLOCK")) db->join_block = std::max<uint64_t>(64, strtoull(jv, nullptr, 10) / 64 * 64);
    if (const char *jv = getenv("SMAFA_JOIN_STRIDE")) db->join_stride = std::min<uint64_t>(4096, std::max<uint64_t>(1, strtoull(jv, nullptr, 10)));
    if (const char *jv = getenv("SMAFA_JOIN_SCRATCH_MAX")) db->join_scratch_max = std::max<uint64_t>(4096, strtoull(jv, nullptr, 10));
    if (const char *jv = getenv("SMAFA_CONSENSUS_CHUNK"))
        db->consensus_chunk = std::min<uint64_t>(1u << 20, std::max<uint64_t>(64, strtoull(jv, nullptr, 10) / 64 * 64));
    if (const char *jv = getenv("SMAFA_NEIGHBOUR_SORT")) db->neighbour_two_sorts = atoi(jv) == 2;
    if (const char *jv = getenv("SMAFA_ASSIGN_SPAN")) db->assign_span = std::min<uint64_t>(1u << 24, std::max<uint64_t>(64, strtoull(jv, nullptr, 10) / 64 * 64));
    db->assign_rows_max = db->join_scratch_max;
    if (const char *jv = getenv("SMAFA_ASSIGN_ROWS_MAX")) db->assign_rows_max = std::max<uint64_t>(64, strtoull(jv, nullptr, 10));
    db->density_keep_max = db->join_scratch_max;
    if (const char *jv = getenv("SMAFA_DENSITY_KEEP_MAX")) {  // any number of rows, 0 included (two joins); not a number: ignored, aloud
        char *end = nullptr;
        const unsigned long long rows = strtoull(jv, &end, 10);
        if (end != jv && *end == 0 && *jv != '-') db->density_keep_max = rows;
        else log_line(0, "SMAFA_DENSITY_KEEP_MAX=\"%s\" is not a number of rows: ignored, the kept pair list may hold %llu rows", jv,
                      (unsigned long long)db->density_keep_max);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) db->n_cu = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&db->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&db->ev0);
    if (e == hipSuccess) e = hipEventCreate(&db->ev1);
    if (e == hipSuccess && db->ctrs.ensure(kCtrBytes) != SMAFA_OK) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemset(db->ctrs.p, 0, kCtrBytes);  // the scan kernels leave their counters at zero
    if (e != hipSuccess) {
        smafa_db_destroy(db);
        return set_error(SMAFA_ERR_DEVICE, "stream/event/counter creation failed: %s", hipGetErrorString(e));
    }
    db->stream = db->own_stream;
    *out = db;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_create");
}

int smafa_db_append(smafa_db *db, const uint8_t *codes, uint64_t n) try {
    if (!db || (!codes && n)) return set_error(SMAFA_ERR_INVALID, "smafa_db_append: NULL argument");
    if (n == 0) return SMAFA_OK;
    if (db->n + n > 0xffffff00ull) return set_error(SMAFA_ERR_INVALID, "subject store limited to 2^32 rows");
    int rc = use_device(db);
    if (rc) return rc;
    uint8_t max_code = 0;
    rc = validate_codes(db, codes, n, &max_code);
    if (rc) return rc;
    if (db->alphabet == SMAFA_ALPHABET_NT && max_code >= 4 && db->P < 3) {  // first N: leave the 2-bit form
        rc = upgrade_planes(db, 3);
        if (rc) return rc;
    }
    rc = reserve_tiles(db, (db->n + n + kWaveTile - 1) / kWaveTile);
    if (rc) return rc;
    rc = pack_rows(db, codes, db->n, n, db->d_planes, 0);
    if (rc) return rc;
    db->n += n;
    db->rows_since_sort += n;
    // a store that is still ONE sorted run (the bulk load itself) has nothing to gain from a re-sort: the quarter rule
    // counts growth since the store was last in one sorted run
    if (db->runs.size() == 1 && db->runs[0].sorted) db->rows_since_sort = 0;
    db->generation++;
    if (n > (1u << 20)) {  // a bulk load's staging and sort buffers are not worth keeping
        for (DevBuf *b : {&db->upload, &db->keys_a, &db->keys_b, &db->idx_a, &db->idx_b, &db->sort_tmp}) b->release();
    }
    log_line(2, "append of %llu rows: %llu in the store, %zu runs, %.2f shared filter bits per tile", (unsigned long long)n,
             (unsigned long long)db->n, db->runs.size(), zone_bits_mean(db));
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_append");
}

int smafa_db_save(smafa_db *db, const char *path) try {
    if (!db || !path) return set_error(SMAFA_ERR_INVALID, "smafa_db_save: NULL argument");
    int rc = use_device(db);
    if (rc) return rc;
    if (!db->layout_set) {  // an empty store has no layout yet: give it the default one
        rc = choose_layout(db, nullptr, 0);
        if (rc) return rc;
    }
    rc = maybe_resort(db);  // a patchwork of appends is saved as one sorted run
    if (rc) return rc;
    PackedHeader h{};
    h.alphabet = (uint32_t)db->alphabet;
    h.seq_len = db->L;
    h.planes = db->P;
    h.words = db->W;
    h.n = db->n;
    h.n_tiles = (db->n + kWaveTile - 1) / kWaveTile;
    h.n_runs = db->runs.size();
    std::vector<uint32_t> planes(h.n_tiles * db->tile_words()), order(h.n_tiles * kWaveTile);
    std::vector<uint4> zone(h.n_tiles);
    if (h.n_tiles) {
        HIP_TRY(hipMemcpyAsync(planes.data(), db->d_planes, planes.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipMemcpyAsync(order.data(), db->d_order, order.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipMemcpyAsync(zone.data(), db->d_zone, zone.size() * sizeof(uint4), hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
    }
    std::vector<uint64_t> runs;
    for (const smafa_db::Run &r : db->runs) {
        runs.push_back(r.rows);
        runs.push_back(r.sorted ? 1u : 0u);
    }
    return write_packed_file(path, h, db->perm.data(), db->tab.data(), runs.data(), order.data(), zone.data(), planes.data());
} catch (...) {
    return smafa::exception_code("smafa_db_save");
}

int smafa_db_load(smafa_db **out, int device, const char *path) try {
    if (!out || !path) return set_error(SMAFA_ERR_INVALID, "smafa_db_load: NULL argument");
    *out = nullptr;
    PackedStore pk;
    int rc = pk.open(path);
    if (rc) return rc;
    return db_load_packed(out, device, pk);
} catch (...) {
    return smafa::exception_code("smafa_db_load");
}

int smafa_db_info(const smafa_db *db, smafa_db_info_t *info) try {
    if (!db || !info) return set_error(SMAFA_ERR_INVALID, "smafa_db_info: NULL argument");
    info->n_subjects = db->n;
    info->seq_len = db->L;
    info->alphabet = db->alphabet;
    info->device = db->device;
    info->planes = db->P;
    info->words_per_plane = db->W;
    info->bytes_per_subject = (uint64_t)db->P * db->W * 4;
    info->hbm_bytes = (db->n + kWaveTile - 1) / kWaveTile * db->tile_words() * sizeof(uint32_t);
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_info");
}

int smafa_db_set_stream(smafa_db *db, void *hip_stream) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_db_set_stream: NULL handle");
    db->stream = hip_stream ? (hipStream_t)hip_stream : db->own_stream;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_set_stream");
}

void smafa_db_destroy(smafa_db *db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->d_planes) (void)hipFree(db->d_planes);
    if (db->d_order) (void)hipFree(db->d_order);
    if (db->d_zone) (void)hipFree(db->d_zone);
    for (DevBuf *b : {&db->upload, &db->hits, &db->count, &db->scratch, &db->ctrs, &db->keys_a, &db->keys_b, &db->sort_tmp,
                      &db->idx_a, &db->idx_b, &db->d_perm, &db->d_tab, &db->d_inv, &db->scratch_q.qrec,
                      &db->scratch_q.thr, &db->scratch_q.cnt, &db->scratch_q2.qrec, &db->scratch_q2.thr, &db->scratch_q2.cnt,
                      &db->scratch_q3.qrec, &db->scratch_q3.thr, &db->scratch_q3.cnt, &db->index.kp, &db->index.dir,
                      &db->index.stats, &db->index.rows, &db->join.pos_of, &db->join.out, &db->join.cnt, &db->join.parent,
                      &db->join.kept, &db->join.hist, &db->join.stable, &db->join.cons, &db->join.ctl, &db->join.entries, &db->join_q.qrec, &db->join_q.thr, &db->join_q.cnt})
        b->release();
    for (hipEvent_t e : db->join.ev)
        if (e) (void)hipEventDestroy(e);
    if (db->each_graph) (void)hipGraphExecDestroy(db->each_graph);
    if (db->ev0) (void)hipEventDestroy(db->ev0);
    if (db->ev1) (void)hipEventDestroy(db->ev1);
    if (db->own_stream) (void)hipStreamDestroy(db->own_stream);
    delete db;
}

int smafa_set_query_block(smafa_db *db, uint32_t queries_per_block) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_set_query_block: NULL handle");
    db->qb_override = queries_per_block;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_set_query_block");
}

int smafa_last_scan_plan(smafa_db *db, uint32_t *filter_plane_resident, uint32_t *tiles_per_wave, uint32_t *query_blocks) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_last_scan_plan: NULL handle");
    if (filter_plane_resident) *filter_plane_resident = db->plan_lazy;
    if (tiles_per_wave) *tiles_per_wave = db->plan_tiles;
    if (query_blocks) *query_blocks = db->plan_qblocks;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_last_scan_plan");
}

int smafa_last_scan_kernel(smafa_db *db, char *name, uint64_t cap) try {
    if (!db || !name || cap == 0) return set_error(SMAFA_ERR_INVALID, "smafa_last_scan_kernel: NULL argument");
    snprintf(name, (size_t)cap, "%s", db->plan_kernel);
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_last_scan_kernel");
}

int smafa_last_call_kernels(smafa_db *db, char *names, uint64_t cap) try {
    if (!db || !names || cap == 0) return set_error(SMAFA_ERR_INVALID, "smafa_last_call_kernels: NULL argument");
    std::string all;
    for (const std::string &k : db->call_kernels) all += (all.empty() ? "" : "\n") + k;
    if (all.size() + 1 > cap) {
        names[0] = '\0';
        return set_error(SMAFA_ERR_CAPACITY, "kernel list too long: %zu bytes needed, capacity %llu", all.size() + 1,
                         (unsigned long long)cap);
    }
    memcpy(names, all.c_str(), all.size() + 1);
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_last_call_kernels");
}

int smafa_hbm_read_probe(int device, uint64_t bytes, double *gb_per_s) try {
    if (!gb_per_s) return set_error(SMAFA_ERR_INVALID, "smafa_hbm_read_probe: NULL argument");
    *gb_per_s = 0.0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return set_error(SMAFA_ERR_DEVICE, "no HIP device visible: the smafa scan engine has no CPU fallback");
    if (device < 0 || device >= ndev) return set_error(SMAFA_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);
    bytes = std::max<uint64_t>(bytes, 1ull << 20) / 16 * 16;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    uint4 *d = nullptr;
    uint32_t *out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess) e = hipMalloc(&out, 4);
    if (e == hipSuccess) e = hipMemset(d, 1, bytes);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best = 0.f;
    for (int shape = 0; shape < 4; shape++) {  // grid-stride at 8 and 32 workgroups per CU, then contiguous spans + nt at 8 and 16
        const int grid = prop.multiProcessorCount * (shape == 0 ? 8 : shape == 1 ? 32 : shape == 2 ? 8 : 16);
        for (int rep = 0; rep < 4 && e == hipSuccess; rep++) {  // the first repetition of each shape warms up
            e = hipEventRecord(e0, nullptr);
            if (shape < 2)
                hipLaunchKernelGGL(hbm_read_probe_kernel, dim3(grid), dim3(256), 0, nullptr, d, (size_t)(bytes / 16), out);
            else
                hipLaunchKernelGGL(hbm_read_probe_span_kernel, dim3(grid), dim3(256), 0, nullptr, d, (size_t)(bytes / 16), out);
            if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e == hipSuccess && rep > 0 && ms > 0.f && (best == 0.f || ms < best)) best = ms;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (out) (void)hipFree(out);
    if (e != hipSuccess) return set_error(SMAFA_ERR_DEVICE, "HBM read probe failed: %s", hipGetErrorString(e));
    if (best > 0.f) *gb_per_s = (double)bytes / ((double)best * 1e-3) / 1e9;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_hbm_read_probe");
}

const char *smafa_build_id(void) {
#ifdef SMAFA_BUILD_ID
    return SMAFA_BUILD_ID;
#else
    return "unknown";
#endif
}

int smafa_set_zone_level(smafa_db *db, int mode) try {
    if (!db || mode < 0 || mode > 2) return set_error(SMAFA_ERR_INVALID, "smafa_set_zone_level: bad argument");
    db->knobs.zone = mode;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_set_zone_level");
}

int smafa_db_build_index(smafa_db *db, uint32_t max_div) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_db_build_index: NULL handle");
    if (max_div >= (uint32_t)kIndexMaxBlocks) return set_error(SMAFA_ERR_INVALID, "smafa_db_build_index: bounds up to %d", kIndexMaxBlocks - 1);
    return index_build(db, max_div + 1u);
} catch (...) {
    return smafa::exception_code("smafa_db_build_index");
}

int smafa_db_drop_index(smafa_db *db) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_db_drop_index: NULL handle");
    int rc = use_device(db);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(db->stream));
    index_drop(db);
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_db_drop_index");
}

int smafa_set_index(smafa_db *db, int mode) try {
    if (!db || mode < 0 || mode > 3) return set_error(SMAFA_ERR_INVALID, "smafa_set_index: bad argument");
    db->index_mode = mode;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_set_index");
}

int smafa_index_info(const smafa_db *db, smafa_index_info_t *info) try {
    if (!db || !info) return set_error(SMAFA_ERR_INVALID, "smafa_index_info: NULL argument");
    memset(info, 0, sizeof *info);
    const auto &ix = db->index;
    info->mode = db->index_mode;
    info->probe_launches = db->index_probes;
    if (!index_current(db)) return SMAFA_OK;
    info->current = 1;
    info->blocks = ix.B;
    info->bytes = ix.kp.cap + ix.dir.cap + ix.rows.cap;
    info->build_ms = ix.build_ms;
    std::vector<double> runs;
    for (uint32_t b = 0; b < ix.B; b++) {
        if (ix.max_run[b] > info->longest_run) info->longest_run = ix.max_run[b];
        if (ix.max_run[b] <= db->index_max_run) runs.push_back(ix.mean_run[b]);
    }
    std::sort(runs.begin(), runs.end());
    info->usable_blocks = (uint32_t)runs.size();
    // the largest bound the index would answer for a big batch, and the candidates per query expected at it
    // (not every bound below it need be: the limit on candidates is wider where the scan kernels are in a slower form)
    double sum = 0.0;
    info->max_div_served = SMAFA_NONE;
    for (size_t j = 0; j < runs.size(); j++) {
        sum += runs[j];
        if (sum > index_cand_limit(db, (uint32_t)j)) continue;
        info->max_div_served = (uint32_t)j;
        info->candidates_per_query = sum;
    }
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_index_info");
}

int smafa_set_prefilter(smafa_db *db, int enabled) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_set_prefilter: NULL handle");
    db->knobs.use_filter = enabled != 0;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_set_prefilter");
}

int smafa_qset_create(smafa_qset **out, smafa_db *db, const uint8_t *query_codes, uint64_t n_queries) try {
    if (!out || !db || (!query_codes && n_queries)) return set_error(SMAFA_ERR_INVALID, "smafa_qset_create: NULL argument");
    *out = nullptr;
    if (n_queries > 0xfffffff0ull) return set_error(SMAFA_ERR_INVALID, "too many queries in one set");
    int rc = use_device(db);
    if (rc) return rc;
    rc = validate_codes(db, query_codes, n_queries);
    if (rc) return rc;
    smafa_qset *qs = new smafa_qset();
    rc = qset_fill(qs, db, query_codes, n_queries);
    if (rc) {
        smafa_qset_destroy(qs);
        return rc;
    }
    *out = qs;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_qset_create");
}

void smafa_qset_destroy(smafa_qset *qs) {
    if (!qs) return;
    if (qs->db) (void)hipSetDevice(qs->db->device);
    if (qs->db && qs->db->each_graph && qs->db->each_key.qs == qs) {  // the captured passes read this set's records
        (void)hipGraphExecDestroy(qs->db->each_graph);
        qs->db->each_graph = nullptr;
    }
    qs->qrec.release();
    qs->thr.release();
    qs->cnt.release();
    delete qs;
}

int smafa_scan_launch(smafa_db *db, smafa_qset *qs, uint32_t max_div, uint32_t max_num_hits, void *d_hits,
                      uint64_t cap, void *d_count) try {
    if (!db || !qs || !d_count || (!d_hits && cap)) return set_error(SMAFA_ERR_INVALID, "smafa_scan_launch: NULL argument");
    db->call_kernels.clear();
    if (qs->db != db) return set_error(SMAFA_ERR_INVALID, "query set was packed for a different store");
    if (max_num_hits == 0) max_num_hits = SMAFA_NONE;
    int rc = use_device(db);
    if (rc) return rc;
    // cap = 0 with no buffer: the caller only wants the count — the kernels still need a non-NULL list to know that rows
    // are wanted (nothing is ever written to it at capacity 0)
    if (!d_hits) d_hits = db->ctrs.p;
    return scan_range(db, qs, 0, (uint32_t)qs->nq, max_div, max_num_hits == SMAFA_NONE ? 0u : max_num_hits,
                      (smafa_hit *)d_hits, cap, (unsigned long long *)d_count);
} catch (...) {
    return smafa::exception_code("smafa_scan_launch");
}

// One pass over the store PER QUERY (north_star's literal "each query is broadcast against all subjects"), the passes
// enqueued back to back by this one call: query i's rows go to d_hits + i * cap_per_query, its exact count to d_counts[i].
// Each pass is the complete one-launch fixed-bound scan of smafa_scan_launch for a one-query set (same kernel choice: a
// sorted store takes scan_zone_few_kernel unless the zone level is off, then the pass streams the prefilter's plane).
// use_graph: the passes are captured once as a HIP graph and replayed while the arguments stay the same — no launch
// gap on the host side at all.
int smafa_scan_each(smafa_db *db, smafa_qset *qs, uint32_t max_div, void *d_hits, uint64_t cap_per_query, void *d_counts,
                    int use_graph) try {
    if (!db || !qs || !d_counts || (!d_hits && cap_per_query)) return set_error(SMAFA_ERR_INVALID, "smafa_scan_each: NULL argument");
    db->call_kernels.clear();
    if (qs->db != db) return set_error(SMAFA_ERR_INVALID, "query set was packed for a different store");
    int rc = use_device(db);
    if (rc) return rc;
    db->last_launches = 0;
    db->timed = false;
    db->call_timed = false;
    const uint32_t nq = (uint32_t)qs->nq;
    if (nq == 0) return SMAFA_OK;
    if (db->n == 0) {
        HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nq * sizeof(unsigned long long), db->stream));
        return SMAFA_OK;
    }
    rc = maybe_resort(db);
    if (rc) return rc;
    if (!d_hits) d_hits = db->ctrs.p;  // count-only: see smafa_scan_launch
    const uint32_t thr0 = std::min<uint32_t>(max_div, db->L);
    const uint32_t n_tiles = (uint32_t)((db->n + kWaveTile - 1) / kWaveTile);
    auto enqueue = [&]() -> int {
        // every pass reserves its rows from its own counter, d_counts[q], zeroed here once for all of them: the count a pass
        // leaves there is its result, and no workgroup has to find out whether it was the last one
        // (a kernel, not hipMemsetAsync: the memset node of a captured graph left garbage in the counters when the graph was
        // replayed — ROCm 7.2; kernel nodes replay as captured)
        hipLaunchKernelGGL(fill_u32_kernel, dim3((2 * nq + 255) / 256), dim3(256), 0, db->stream, (uint32_t *)d_counts, 0u,
                           (uint64_t)2 * nq);
        for (uint32_t q = 0; q < nq; q++) {
            int r = launch_tiles(db, qs, q, q + 1, 0, n_tiles, 0, thr0, (smafa_hit *)d_hits + (size_t)q * cap_per_query,
                                 cap_per_query, nullptr, false, (unsigned long long *)d_counts + q);
            if (r) return r;
        }
        return SMAFA_OK;
    };
    if (!use_graph) {
        HIP_TRY(hipEventRecord(db->ev0, db->stream));
        rc = enqueue();
        if (rc) return rc;
        HIP_TRY(hipEventRecord(db->ev1, db->stream));
        db->timed = true;
        return SMAFA_OK;
    }
    smafa_db::EachKey key;
    memset(&key, 0, sizeof key);  // (padding bytes take part in the comparison below)
    key.qs = qs, key.qrec = qs->qrec.p, key.qs_serial = qs->serial;
    key.hits = d_hits, key.counts = d_counts, key.cap = cap_per_query, key.nq = qs->nq, key.generation = db->generation;
    key.max_div = max_div, key.qb = db->qb_override, key.zone = db->knobs.zone, key.filter = db->knobs.use_filter;
    if (!db->each_graph || memcmp(&key, &db->each_key, sizeof key) != 0) {
        if (db->each_graph) (void)hipGraphExecDestroy(db->each_graph);
        db->each_graph = nullptr;
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(db->stream, hipStreamCaptureModeThreadLocal));
        rc = enqueue();
        hipError_t e = hipStreamEndCapture(db->stream, &graph);
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        if (e != hipSuccess) return set_error(SMAFA_ERR_DEVICE, "graph capture failed: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&db->each_graph, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) {
            db->each_graph = nullptr;
            return set_error(SMAFA_ERR_DEVICE, "graph instantiation failed: %s", hipGetErrorString(e));
        }
        memcpy(&db->each_key, &key, sizeof key);
        db->each_kernels = db->call_kernels;
    }
    db->call_kernels = db->each_kernels;
    db->last_launches = nq;
    HIP_TRY(hipEventRecord(db->ev0, db->stream));
    HIP_TRY(hipGraphLaunch(db->each_graph, db->stream));
    HIP_TRY(hipEventRecord(db->ev1, db->stream));
    db->timed = true;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_scan_each");
}

int smafa_last_call_stats(smafa_db *db, float *kernel_ms, uint32_t *n_launches, uint32_t *n_scans) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_last_call_stats: NULL handle");
    if (kernel_ms) *kernel_ms = db->call_ms;
    if (n_launches) *n_launches = db->call_launches;
    if (n_scans) *n_scans = db->call_scans;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_last_call_stats");
}

int smafa_launch_device(smafa_db *db, int *device_at_last_launch, uint64_t *launches_off_device) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_launch_device: NULL handle");
    if (device_at_last_launch) *device_at_last_launch = db->launch_device;
    if (launches_off_device) *launches_off_device = db->launches_off_device;
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_launch_device");
}

int smafa_sync(smafa_db *db) try {
    if (!db) return set_error(SMAFA_ERR_INVALID, "smafa_sync: NULL handle");
    HIP_TRY(hipStreamSynchronize(db->stream));
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_sync");
}

int smafa_last_scan_ms(smafa_db *db, float *ms, uint32_t *n_launches) try {
    if (!db || !ms) return set_error(SMAFA_ERR_INVALID, "smafa_last_scan_ms: NULL argument");
    *ms = 0.f;
    if (n_launches) *n_launches = db->call_timed ? db->call_launches : db->last_launches;
    if (db->call_timed) {  // a self-join: the totals over its blocks (each block was timed and waited for as it ran)
        *ms = db->call_ms;
        return SMAFA_OK;
    }
    if (!db->timed) return SMAFA_OK;
    HIP_TRY(hipEventSynchronize(db->ev1));
    HIP_TRY(hipEventElapsedTime(ms, db->ev0, db->ev1));
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_last_scan_ms");
}

int smafa_scan_hits(smafa_db *db, const uint8_t *query_codes, uint64_t n_queries, uint32_t max_div,
                    uint32_t max_num_hits, smafa_hit *out, uint64_t cap, uint64_t *n_out) try {
    if (!db || !n_out || (!query_codes && n_queries) || (!out && cap))
        return set_error(SMAFA_ERR_INVALID, "smafa_scan_hits: NULL argument");
    db->call_kernels.clear();
    if (max_num_hits == 0) max_num_hits = SMAFA_NONE;
    // fingerprint of the request: the query bytes, their count, the bounds and the state of the store
    uint64_t key = 0x9e3779b97f4a7c15ull ^ db->generation;
    {
        const size_t bytes = (size_t)n_queries * db->L;
        size_t i = 0;
        for (; i + 8 <= bytes; i += 8) {
            uint64_t v;
            memcpy(&v, query_codes + i, 8);
            key = (key ^ v) * 0xff51afd7ed558ccdull;
            key ^= key >> 32;
        }
        for (; i < bytes; i++) key = (key ^ query_codes[i]) * 0x100000001b3ull;
    }
    std::vector<smafa_hit> rows;
    if (db->retry_valid && db->retry_key == key && db->retry_nq == n_queries && db->retry_div == max_div &&
        db->retry_k == max_num_hits && db->retry_codes.size() == (size_t)n_queries * db->L &&
        memcmp(db->retry_codes.data(), query_codes, db->retry_codes.size()) == 0) {
        rows.swap(db->retry_rows);  // the retry after SMAFA_ERR_CAPACITY: same request, same store
    } else {
        int rc = scan_to_host(db, query_codes, n_queries, max_div, max_num_hits, rows);
        if (rc) return rc;
    }
    db->retry_valid = false;
    std::vector<smafa_hit>().swap(db->retry_rows);
    *n_out = rows.size();
    if (rows.size() <= cap) std::vector<uint8_t>().swap(db->retry_codes);
    if (rows.size() > cap) {
        const size_t need = rows.size();
        db->retry_rows.swap(rows);
        db->retry_codes.assign(query_codes, query_codes + (size_t)n_queries * db->L);
        db->retry_key = key;
        db->retry_nq = n_queries;
        db->retry_div = max_div;
        db->retry_k = max_num_hits;
        db->retry_valid = true;
        return set_error(SMAFA_ERR_CAPACITY, "hit buffer too small: %zu rows needed, capacity %llu", need,
                         (unsigned long long)cap);
    }
    if (!rows.empty()) memcpy(out, rows.data(), rows.size() * sizeof(smafa_hit));
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_scan_hits");
}

#include "self_join_abi.hip.h"  // the smafa_db_self_* entry points: argument checks, the device-pointer forms, the host forms
#include "read_table.hip.h"     // the frame of a call that scans a caller's query set and tabulates it: opening, span loop, table, host form
#include "assign_abi.hip.h"     // the abundance table: its call (assign_reads) and the two smafa_db_assign entry points
#include "classify_abi.hip.h"   // the LCA classification: its call (classify_reads) and the two smafa_db_classify entry points
#include "subset_abi.hip.h"     // rows out of a store: a subset of it as a new store, its sequences back as code bytes
#undef RC_TRY

int smafa_distances(smafa_db *db, const uint8_t *query_codes, uint32_t *distances) try {
    if (!db || !query_codes || (!distances && db->n)) return set_error(SMAFA_ERR_INVALID, "smafa_distances: NULL argument");
    db->call_kernels.clear();
    if (db->n == 0) return SMAFA_OK;
    int rc = use_device(db);
    if (rc) return rc;
    rc = validate_codes(db, query_codes, 1);
    if (rc) return rc;
    rc = qset_fill(&db->scratch_q, db, query_codes, 1);
    if (rc) return rc;
    const uint32_t n_tiles = (uint32_t)((db->n + kWaveTile - 1) / kWaveTile);
    rc = db->keys_a.ensure((size_t)n_tiles * kWaveTile * sizeof(uint32_t));  // any scratch buffer will do
    if (rc) return rc;
    hipLaunchKernelGGL(distances_kernel, dim3((n_tiles + kWgWaves - 1) / kWgWaves), dim3(256), 0, db->stream,
                       reinterpret_cast<const uint4 *>(db->d_planes), n_tiles, (uint32_t)db->n, db->P, db->PQ, db->W,
                       db->scratch_q.qrec.as<uint32_t>(), db->d_order, db->keys_a.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(distances, db->keys_a.p, db->n * sizeof(uint32_t), hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    return SMAFA_OK;
} catch (...) {
    return smafa::exception_code("smafa_distances");
}

}  // extern "C"

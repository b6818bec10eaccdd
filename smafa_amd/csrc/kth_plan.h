// kth_plan.h — what the k-nearest path decides, in ONE place: the near-hit ladder of a host-buffer call and what a block index
// replaces of it, when the automatic index modes buy an index (rent or buy), whether the ladder's first step is worth asking of
// the whole batch and which later steps pay, and the order of work of one tightening scan (kth_schedule).  scan_host.hip.h runs
// these decisions and takes none itself.  Every function is pure: values in, a small struct or a fixed array out.
// Plain C++17, no HIP types: tests/test_kth_plan_model.py compiles this header alone with g++ and checks every rule on the CPU.
#pragma once

#include <cassert>
#include <cmath>
#include <cstdint>

#include "scan_plan.h"

namespace smafa {

// ---- the near-hit ladder ----------------------------------------------------------------------------------------------------
// k-th-distance modes whose bound is loose or absent (`smafa query` without --max-divergence — the reference's
// default): the scan would run the all-planes kernel until each query's running bound has tightened.  Most queries
// of real inputs have their k nearest subjects within a few mismatches, so first ask the cheap questions: a LADDER of
// scans whose bound starts at a value the prefilters still handle well (5 of the first 32 columns: level 1 prunes,
// zone kernel; then 12, and 30 (two planes: 16) at two words per plane: the folded bounds of the all-planes kernel still reject
// nearly every pair there), each over the queries the step before left open.  A query with at least k rows within a step's bound is
// finished: its k-th smallest distance is <= that bound, so every row it may print is among them.  Whoever is
// left takes the tightening path, as a compacted batch.  Exact at every step.  A step that finishes fewer than an
// eighth of its queries is the last one (data without near neighbours pays for one cheap step only).
// Measured, 10 000 queries x 10M aa subjects, best hit, per step (tools/bound_probe.py, profiles/
// r02_bound_probe.txt): bound 5 2.1 ms, 8 8.1 ms, 12 9.2 ms, 14 14.3 ms, no bound 28 ms; nucleotides 1.8, 6.6, 7.7,
// 10.4, 16.7.
constexpr uint32_t kLadderMax = 4;             // steps a ladder can have
constexpr uint32_t kLadderMinQueries = 16;     // smaller batches (and smaller open batches) go straight to the loose path
constexpr uint32_t kPlannerMinQueries = 2048;  // open queries from which the later steps are planned from a sample
constexpr uint32_t kProbeSample = 256;         // queries the first step is asked of before the whole batch pays for it

struct LadderBounds {
    uint32_t n = 0;
    uint32_t bound[kLadderMax] = {0, 0, 0, 0};
    uint32_t operator[](size_t i) const { return bound[i]; }
    void push(uint32_t b) {
        assert(n < kLadderMax);
        bound[n++] = b;
    }
};

// the columns level 1 of the prefilter looks at
inline uint32_t ladder_cols(uint32_t L) { return L < 32u ? L : 32u; }

inline LadderBounds ladder_bounds(uint32_t L, uint32_t W, uint32_t P, uint64_t n_queries) {
    const uint32_t cols = ladder_cols(L);
    LadderBounds ladder;
    // first step: level 1 looks at `cols` columns of one plane; at a bound of a sixth of them it still rejects all but
    // a few percent of the (wave, query) steps
    ladder.push((cols - 1u) / 6u);
    ladder.push(3u * cols / 8u);
    if (W == 2 && L >= 33) {  // two words: scan_kernel's FOLD 1 / FOLD 2 forms still reject at 13..17 / 18..32
        // (a step at 16 in front of the one at 30 costs nearly as much and is redundant: queries 0..30 substitutions away
        // from their subject, 10 000 x 10M aa: 35 ms with both, profiles/r02_besthit_ladder.txt)
        // (three planes and more: a step at 17, the top of FOLD 1's range — 12 ms where the step at 30 costs 15 — is there for
        // the planner below to choose when most open queries lie within it)
        // — only where the planner will run (choose_later_steps needs 2048 open queries): a small batch would otherwise run the
        // steps at 17 AND 30 back to back, which the measurement above found redundant
        if (P >= 3 && n_queries >= kPlannerMinQueries) ladder.push(17u);
        ladder.push(P >= 3 ? 30u : 16u);
    }
    return ladder;
}

// does a call walk the ladder at all?
inline bool ladder_runs(uint32_t k_mode, const ScanKnobs &k, bool two_phase, uint64_t n_queries) {
    return k_mode >= 1 && k.use_filter && k.lazy && two_phase && n_queries >= kLadderMinQueries;
}

// A store with a current block index answers "every pair within d" for the largest bound d its blocks serve in a few
// microseconds per thousand queries: that fixed-bound scan goes first, in place of every tightening step at or below d
// (a query with k rows within d is finished exactly as after any other step).
// (only where it replaces the ladder's first step: a lower bound than that finishes too few queries to pay for the
// extra round of compaction — nucleotides, 10M x 100 000 queries, index served up to 2: 27 -> 45 ms; profiles/r04_index.txt)
// `served`: the largest bound the index answers for this batch.  Returns whether step 0 is now the index's.
inline bool ladder_with_index(LadderBounds &ladder, uint32_t served, uint32_t limit) {
    if (!(served < limit && served >= ladder[0])) return false;
    LadderBounds kept;
    kept.push(served);
    for (uint32_t i = 0; i < ladder.n; i++)
        if (ladder[i] > served) kept.push(ladder[i]);
    ladder = kept;
    return true;
}

// ---- rent or buy: when the automatic index modes build a block index ------------------------------------------------------------
// The scans that could have used an index are charged at the batched kernels' measured rate, in ms per pair and stored vector:
// a fixed-bound scan 1.7e-12 (profiles/r04_bench_full.json); the ladder and the loose path of a call WITHOUT a usable bound
// ~1.6e-11 (10 000 queries x 10M aa: 16-19 ms, profiles/r04_bench_full.json).  The build costs ~1 ms per block and 10M
// subjects (profiles/r04_index.txt); the index is built once the rent paid equals its price.
constexpr double kRentFixedBound = 1.7e-12;
constexpr double kRentLoose = 1.6e-11;

inline double index_rent_charge(uint64_t nq, uint64_t n, uint32_t vectors, double rate) {
    return (double)nq * (double)n * (double)vectors * rate;
}
inline bool index_rent_due(double debt_ms, uint32_t blocks, uint64_t n) { return debt_ms >= 0.3 + (double)blocks * (double)n * 1.0e-7; }

// what a rent site knows of the handle and of its index
struct IndexSite {
    int mode;                        // smafa_db::index_mode
    uint64_t n, min_rows;            // subjects stored, and the fewest an automatic build is worth (SMAFA_INDEX_MIN_ROWS)
    uint32_t W, L;
    uint32_t max_words, max_blocks;  // kIndexMaxWords, kIndexMaxBlocks (index.hip.h)
    bool current;                    // the store has an index that matches its state ...
    uint32_t B;                      // ... of this many blocks
    bool failed;                     // an automatic build failed since the store last changed: not tried again
};

// A fixed-bound scan of more than 64 queries (modes 2 and 3): would an index of bound + 1 blocks answer it, and is there none yet?
inline bool fixed_bound_wants_index(const IndexSite &s, const ScanKnobs &k, uint32_t nq, uint32_t thr0) {
    return s.mode >= 2 && k.use_filter && nq > 64u && s.W <= s.max_words && thr0 + 1u <= (s.max_blocks < s.L ? s.max_blocks : s.L) &&
           s.n >= s.min_rows && s.n < (1ull << 31) && (!s.current || s.B < thr0 + 1u);
}

// Blocks as narrow as the store's size leaves selective (~log2(n) - 2 bits of letters per block: 4 aa columns, 10 nucleotides at
// 10M subjects), so that the index serves the widest bounds it can (aa: up to 14).
inline uint32_t index_blocks_wanted(bool amino_acids, uint32_t P, uint64_t n, uint32_t L, uint32_t max_blocks) {
    const double letter_bits = amino_acids ? 4.3 : P == 2 ? 2.0 : 2.3;
    const double fit = std::floor((std::log2((double)n) - 2.0) / letter_bits);
    const uint32_t width = (uint32_t)(fit > 2.0 ? fit : 2.0);
    return max_blocks < L / width ? max_blocks : L / width;
}

// A k-nearest call WITHOUT a usable bound (mode 3 — what `smafa query` sets): may it be charged rent at all ...
inline bool loose_call_pays_rent(const IndexSite &s, const ScanKnobs &k, bool two_phase, uint32_t k_mode, uint64_t n_queries, uint32_t limit,
                                 uint32_t first_bound) {
    return s.mode == 3 && k_mode >= 1 && n_queries > 64 && k.use_filter && k.lazy && two_phase && limit > first_bound &&
           s.W <= s.max_words && s.n >= s.min_rows && s.n < (1ull << 31) && !s.failed;
}
// ... and is — only where that index would take at least the ladder's first step, and is not there yet
inline bool loose_call_wants_index(const IndexSite &s, uint32_t want, uint32_t first_bound) {
    return want >= first_bound + 1u && (!s.current || s.B < want);
}

// ---- the first step's probe, and the planner of the later steps --------------------------------------------------------------
// Does the FIRST step finish anybody?  On queries unrelated to the store (or a k that wants more neighbours than a family has)
// it costs a full zone-kernel pass and finishes nobody (2.2 ms per 10 000 queries at 10M subjects: 14 % of a batch of unrelated
// queries, 7 % of a k = 5 call).  Asked of every (n / 256)-th query first (0.1-0.2 ms): below a sixteenth of the sample finished,
// the step is skipped and the later steps are planned right away.  Exact either way (a skipped step only moves queries to a
// later, looser scan).
inline bool first_step_probed(bool laddered, bool ladder_probe, uint64_t n_queries, uint32_t limit, uint32_t first_bound, bool index_first) {
    return laddered && ladder_probe && n_queries >= kPlannerMinQueries && limit > first_bound && !index_first;
}
inline bool first_step_probe_skips(uint32_t finished, uint32_t ns) { return finished * 16u < ns; }

// "not planned yet, at least 2048 open, and a later step exists": the later steps are planned now
inline bool plans_later_now(bool planned, uint32_t open, size_t step, uint32_t n_steps) {
    return !planned && open >= kPlannerMinQueries && step + 1 < n_steps;
}
// the planner's sample of the open queries (a share estimated to +-3 %; ~0.7 ms at 10M subjects)
inline uint32_t planner_sample(uint32_t open) { return open / 8u < kProbeSample ? open / 8u : kProbeSample; }

// Which LATER steps pay is estimated once, on a sample of the queries the first step left open: every (cur_n / 256)-th
// open query is scanned in the k-th mode at the ladder's last bound, and the distribution of their k-th distances says
// what share of the open queries each later step would finish.  A step costs about 0.37 (bounds the OR-fold still
// rejects at), 0.5 (FOLD 1: the filter plane's per-word sums) or 0.53 (FOLD 2: two planes) of what the loose path costs
// per query (10M x 60 aa, 10 000 queries, best-hit launches: 9.1 / 12.5 / 13.2 ms against 25 ms for queries nothing is near to,
// profiles/r04_bound_probe.txt; round 3's 0.3 / 0.4 / 0.5 were taken against a 29 ms loose path: with half the queries
// unrelated the step at 12 then cost 7.4 ms to finish what the loose path does in 5.5, profiles/r04_kth.txt); the cheapest
// sequence of steps + loose path for the rest wins.
// (Round 2 stopped after any step that finished less than an eighth: queries 9-14 columns away from their nearest
// subject — novel members of a family — then paid the loose path in full: 33 ms per 10 000 instead of ~17.)
constexpr double kStepCostOrFold = 0.37, kStepCostFold1 = 0.5, kStepCostFold2 = 0.53;
inline double step_cost(uint32_t bound, uint32_t cols) { return bound <= 3u * cols / 8u ? kStepCostOrFold : bound <= 17u ? kStepCostFold1 : kStepCostFold2; }

// the steps from `from` on that lie below the call's own bound: the last of them, and whether there is any
struct LaterSteps {
    size_t last;
    bool any;
};
inline LaterSteps later_steps(const LadderBounds &ladder, size_t from, uint32_t limit) {
    size_t last = from;
    while (last + 1 < ladder.n && ladder[last + 1] < limit) last++;
    return {last, !(from >= ladder.n || ladder[from] >= limit)};
}

struct LaterChoice {
    uint32_t mask;  // bit t: the step at ladder[from + t] runs
    double cost;    // of the chosen steps and the loose path for the rest, in loose-path passes over the open queries
};
// kth[i]: the k-th smallest distance of sample query i within the last bound, UINT32_MAX where it has fewer than k rows there
inline LaterChoice choose_later_steps(const uint32_t *kth, uint32_t ns, const LadderBounds &ladder, size_t from, size_t last, uint32_t cols) {
    const size_t n_later = last - from + 1;  // at most two steps today: every subset is tried
    LaterChoice best = {0, 1.0};             // no further step: the loose path for everybody
    for (uint32_t mask = 1; mask < (1u << n_later); mask++) {
        double cost = 0.0, open_share = 1.0;
        for (size_t t = 0; t < n_later; t++) {
            if (!((mask >> t) & 1u)) continue;
            const uint32_t b = ladder[from + t];
            size_t fin = 0;
            for (uint32_t i = 0; i < ns; i++) fin += kth[i] <= b;
            cost += open_share * step_cost(b, cols);
            open_share = 1.0 - (double)fin / (double)ns;
        }
        cost += open_share;
        if (cost < best.cost) best = {mask, cost};
    }
    return best;
}

// a small batch: round 2's rule of thumb
// (the step at 30 costs half of what the loose path costs: it is taken only after a step that finished a quarter)
// next_bound: the bound of the ladder's next step, 0 where there is none
inline bool step_paid(uint64_t finished, uint32_t open_before, uint32_t next_bound) { return finished * (next_bound >= 30u ? 4u : 8u) >= open_before; }

// ---- one tightening scan (scan_kth) ---------------------------------------------------------------------------------------------
// (k >= 2 with a loose bound counts first and appends only the final rows, straight into the caller's list.)
inline bool kth_count_first(uint32_t k, uint32_t count_first_k, const ScanShape &s, const ScanKnobs &knobs, uint32_t thr0) {
    return k >= count_first_k && !prefilter_prunes(s, knobs, thr0);
}

// k >= 2: the k-th smallest distance within the first (up to) 1024 subjects, from an LDS histogram per query
// (kth_seed_kernel: no global atomics; the counting launch it replaces put every pair of its tile through them)
inline bool kth_hist_seed(uint32_t k, uint32_t L, uint32_t seed_bins, bool enabled) { return k >= 2 && L < seed_bins && enabled; }

// Counting first costs TWO passes over every pair (count, then append with the exact bounds).  On a big store the first
// one is cut to a SAMPLE — the first 1/32 of the tiles: the k-th smallest distance within any subset of the subjects is an
// upper bound of the k-th smallest over all of them — and the rest of the store is scanned ONCE, counting, tightening and
// appending to the scratch list from that bound on; the counts are then complete up to the k-th distance (the bound never
// dropped below it), so kth_from_counts_kernel gives the exact bounds, the sample's own tiles are scanned again with
// those fixed (appending), and filter_rows_kernel keeps what is within them: (1 + 1/32) passes instead of 2
// (10 000 queries x 10M aa, k = 5 / 50, sample 1/8: 34 / 39 ms, 1/16: 30 / 35, 1/32: 28 / 35; profiles/r04_kth.txt).
// Rows parked meanwhile: ~k x (segment / store seen before it) per segment, a few k per query (SMAFA_KTH_SAMPLE=0: two passes).
inline uint32_t kth_sample_tiles(bool count_first, uint32_t div, uint32_t min_tiles, uint32_t n_tiles, uint32_t k) {
    return (count_first && div && n_tiles >= min_tiles && n_tiles / div >= 1u && (uint64_t)k * 4u <= (uint64_t)(n_tiles / div) * kWaveTile)
               ? n_tiles / div : 0u;
}

// Tightening modes append every pair that is within its query's bound at that moment — 50-100 rows per query
// when the bound starts loose — of which the filter pass keeps the ones within the final bound: the scratch list
// is sized for the appended volume, the caller's buffer only has to hold what is kept.  0: the scan parks no rows.
inline uint64_t kth_scratch_rows(bool count_first, uint32_t sample_tiles, uint32_t nq, uint32_t k, uint64_t cap) {
    if (count_first && !sample_tiles) return 0;
    const uint64_t per_query = sample_tiles ? 16ull * k + 128u : 128u;
    const uint64_t appended = (uint64_t)nq * per_query < (1ull << 27) ? (uint64_t)nq * per_query : 1ull << 27;
    return 2 * cap > appended ? 2 * cap : appended;
}

// kth_seed_kernel's tile groups per query chunk, counting (a sample's pairs go to cnt[q][d]) or not (the seed bound alone: one):
// enough workgroups to fill the chip (8 per CU), never more tile groups than 4-tile steps
inline uint32_t kth_hist_groups(bool counting, uint32_t tiles, uint32_t n_chunks, uint32_t n_cu, uint32_t groups_override) {
    if (!counting) return 1u;
    const uint32_t steps = (tiles + kWgWaves - 1) / kWgWaves, fill = (n_cu * 8u + n_chunks - 1) / n_chunks;
    uint32_t n_groups = steps < fill ? steps : fill;
    if (n_groups < 1u) n_groups = 1u;
    if (groups_override && groups_override < n_groups) n_groups = groups_override;  // (1: one workgroup per chunk walks every step)
    return n_groups;
}

// The order of work of one tightening scan.  Workgroups of one launch run side by side and would all start from the loose
// initial bound, so the store is walked in segments that grow 8x per launch (bounds tighten between launches), after a seed
// that only lowers the bounds and appends nothing.  With a sample (kth_sample_tiles) only the sample is walked that way —
// or counted whole by the histogram kernel —, the rest in segments growing 4x from 3x the sample, so that the workgroups of
// one launch do not all start from the sample's bound.
enum class KthStep : uint8_t {
    ZeroCounts,          // cnt[q][*] = 0 for the scan's queries (k >= 2; k = 1 keeps no counts)
    SeedHist,            // kth_seed_kernel over the first tiles: lowers the bounds, counts nothing
    SeedScan,            // the scan kernel's seed form over the first tiles: lowers the bounds, appends nothing
    SampleHist,          // kth_seed_kernel counting every pair of the sample into cnt[q][d]
    Count,               // a tightening launch that counts and appends nothing (counting first)
    CountAppend,         // a tightening launch that appends to the scratch list
    BoundsFromCounts,    // kth_from_counts_kernel: bounds from the counts so far
    FixedAppendScratch,  // the sample's own tiles with the exact bounds fixed, appending to the scratch list
    FixedAppendCaller,   // every tile with the exact bounds fixed, straight into the caller's list; then the scan's end is recorded
    Filter,              // the scan's end is recorded; filter_rows_kernel keeps the scratch rows within the final bounds
};
struct KthScheduleStep {
    KthStep kind;
    uint32_t tile_begin, tile_end;  // (0, 0 where the step has no tile range)
};
// A store has at most 2^24 wave tiles (32-bit subject numbers).  Segments of 4 tiles growing 8x cover them in 9 launches
// (4 (8^9 - 1) / 7 > 2^24), segments growing 4x from 3 tiles and more in 13 (4^13 - 1 > 2^24); around them at most two
// ZeroCounts, a seed, two BoundsFromCounts, a fixed pass and the filter: 29 steps.
constexpr uint32_t kKthMaxTiles = 1u << 24;
constexpr uint32_t kKthScheduleMax = 32;
struct KthSchedule {
    uint32_t n = 0;
    KthScheduleStep step[kKthScheduleMax];
    void add(KthStep kind, uint32_t tile_begin = 0, uint32_t tile_end = 0) {
        assert(n < kKthScheduleMax);
        step[n++] = {kind, tile_begin, tile_end};
    }
};

inline KthSchedule kth_schedule(uint32_t n_tiles, uint32_t k, bool count_first, uint32_t sample_tiles, bool hist_seed) {
    assert(n_tiles >= 1 && n_tiles <= kKthMaxTiles && sample_tiles <= n_tiles);
    KthSchedule s;
    if (k >= 2) s.add(KthStep::ZeroCounts);
    // ... and where a sample is counted first (sample_tiles), the same kernel counts the WHOLE sample: every pair of it, in LDS
    // histograms that are added to cnt[q][d] — exactly what the counting launches would have counted, without their global
    // atomics per pair and their growing segments (k = 50, 10 000 queries: 12 ms -> ~2 ms for a 1/32 sample)
    const bool hist_sample = hist_seed && sample_tiles != 0;
    if (hist_sample) {
        s.add(KthStep::SampleHist, 0, sample_tiles);
    } else if (hist_seed) {
        s.add(KthStep::SeedHist, 0, n_tiles < (uint32_t)kWgWaves ? n_tiles : (uint32_t)kWgWaves);
    } else {
        // seed: k = 1 reduces each wave's minimum before its single atomicMin, so a whole workgroup tile is
        // cheap; the k >= 2 seed counts every pair in its histogram, so keep it to one wave tile
        const uint32_t seed_tiles = k == 1 ? (uint32_t)kWgWaves : 1u;
        s.add(KthStep::SeedScan, 0, seed_tiles < n_tiles ? seed_tiles : n_tiles);
        if (k >= 2) s.add(KthStep::ZeroCounts);  // the seed's subjects are counted again below
    }
    uint32_t len = hist_seed ? 8u * kWgWaves : kWgWaves;  // (the histogram seed already stands for the first 4 tiles)
    const uint32_t count_end = sample_tiles ? sample_tiles : n_tiles;  // the tiles that are only counted
    uint32_t begin = hist_sample ? count_end : 0u;                     // (counted already, every pair of them)
    while (begin < count_end) {
        const uint32_t end = count_end - begin > len ? begin + len : count_end;
        s.add(count_first ? KthStep::Count : KthStep::CountAppend, begin, end);
        begin = end;
        len = len > (1u << 28) ? len : len * 8;
    }
    if (sample_tiles) {
        // bounds from the sample's counts (a query with fewer than k subjects in range so far keeps its bound)
        s.add(KthStep::BoundsFromCounts);
        // the rest of the store, once: count, tighten, append to the scratch list — in segments growing 4x, so that the
        // workgroups of one launch do not all start from the sample's bound
        len = 3u * sample_tiles;
        while (begin < n_tiles) {
            const uint32_t end = n_tiles - begin > len ? begin + len : n_tiles;
            s.add(KthStep::CountAppend, begin, end);
            begin = end;
            len = len > (1u << 28) ? len : len * 4;
        }
        // every pair within the k-th distance has been counted once: the exact bounds; then the sample's own tiles with
        // those bounds fixed, appending to the same list
        s.add(KthStep::BoundsFromCounts);
        s.add(KthStep::FixedAppendScratch, 0, sample_tiles);
        s.add(KthStep::Filter);  // rows within the exact bounds go to the caller's list
    } else if (count_first) {
        s.add(KthStep::BoundsFromCounts);
        s.add(KthStep::FixedAppendCaller, 0, n_tiles);
    } else {
        s.add(KthStep::Filter);
    }
    return s;
}

}  // namespace smafa

// scan_plan.h — which kernel one scan launch runs, decided in ONE place: plan_scan() maps the store's shape, the handle's
// switches and the launch's inputs to the instantiation, its tiles per wave and workgroup size, and scan_kernel_name() spells
// that instantiation the way rocprofv3 lists it.  engine.hip launches from the plan and derives nothing itself; kernels.hip.h
// takes its compile-time geometry from the constants below, so host and device share one definition.
// Plain C++17, no HIP types: tests/test_scan_plan_model.py compiles this header alone with g++ and checks the choice on the CPU.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>

namespace smafa {

constexpr int kWaveTile = 256;  // subjects per wave tile
constexpr int kWgWaves = 4;     // waves per workgroup
constexpr int kChunk = 64;      // queries staged in LDS at a time
#ifndef SMAFA_SUM_FOLD
#define SMAFA_SUM_FOLD 1  // scan_kernel<.., FOLD = 1 | 2 | 3> for two-word launches with a bound of 13..17 | 18..32 | above (plan_scan)
#endif

constexpr int round_up4(int x) { return (x + 3) & ~3; }
// query record stride in u32 words: the plane words plus the bound slot, rounded up to whole uint4s
constexpr int qrec_stride(int planes, int words) { return round_up4(planes * words + 1); }

// ---- scan_zone_kernel / scan_zone_few_kernel: tiles per wave and waves per workgroup
#ifndef SMAFA_ZONE_TILES
#define SMAFA_ZONE_TILES 4
#endif
// ... per shape and form.  The UNSTAGED five-plane two-word kernel (60-column amino acids, fixed bound) takes 2 tiles per wave at
// 7 waves per SIMD (72 VGPRs): without LDS staging and barriers there is little per-chunk work left to amortise over more tiles,
// and every resident wave more hides more of the survivor loop's dependent slow-class chain.  Same box, ms per launch, 10M x 10k /
// 50M x 125k (profiles/r04_zone_variants.txt): 5 waves x 4 tiles 1.795 / 53.5, 5 x 6 1.77 / 52.0, 6 x 3 1.71 / 50.6, 6 x 2 1.72 /
// 51.5, **7 x 2 1.68 / 49.3**, 7 x 3 1.76 / 64.6 (spills), 8 x 2 1.78 / 78.4 (spills), 4 x 6 1.95, 6 x 4 2.01.  Nucleotides keep 4
// tiles (3: 2.80, 6: 3.12 vs 2.70 ms).  SMAFA_ZONE_TILES != 4 overrides for every shape.
#ifndef SMAFA_ZONE_TILES_DIRECT_AA
#define SMAFA_ZONE_TILES_DIRECT_AA 2  // tiles per wave of the unstaged five-plane two-word kernel alone (nucleotide shapes keep theirs)
#endif
constexpr int zone_tiles(int ps, int w, bool direct) {
    return SMAFA_ZONE_TILES != 4 ? SMAFA_ZONE_TILES : (direct && ps == 5 && w == 2 ? SMAFA_ZONE_TILES_DIRECT_AA : 4);
}
#ifndef SMAFA_ZONE_WG_WAVES
#define SMAFA_ZONE_WG_WAVES 2
#endif
constexpr int kZoneWgWaves = SMAFA_ZONE_WG_WAVES;
#ifndef SMAFA_FEW_TILES
#define SMAFA_FEW_TILES 4
#endif
constexpr int kFewTiles = SMAFA_FEW_TILES;  // wave tiles per wave in scan_zone_few_kernel

// ---- scan_wide_kernel and scan_generic_kernel
constexpr int kWideTiles = 4;
constexpr int kWideStage = 768;  // uint4 per LDS buffer
constexpr bool wide_fits(int planes, int words) { return qrec_stride(planes, words) / 4 <= kWideStage; }
constexpr int kGenericTiles = 4;

// The switches the choice reads: a member of the handle (smafa_db::knobs), set when it is created and by smafa_set_prefilter /
// smafa_set_zone_level.
struct ScanKnobs {
    bool lazy = true;             // filter-plane-resident kernel where it applies (SMAFA_LAZY=0 disables)
    bool use_filter = true;       // exact lower-bound prefilter in the scan kernel (SMAFA_FILTER=0 disables)
    bool wide_one = true;         // one-word stores (L <= 32) through scan_wide_kernel's two-plane level 2 (SMAFA_WIDE_ONE=0: lazy kernel)
    uint32_t wide_from = 5;       // words per plane from which scan_wide_kernel replaces the per-length kernels (SMAFA_WIDE_FROM)
    uint32_t tiles_override = 0;  // SMAFA_TILES
    int zone = 1;                 // zone level of the filter-plane-resident kernel: 1 = where it prunes (zone_pays), 0 = never
                                  // (SMAFA_ZONE=0), 2 = whenever that kernel runs (SMAFA_ZONE=2, tests)
    double zone_loose = 0.3;      // pass share below which the zone kernel also takes bounds level 1 cannot prune at (SMAFA_ZONE_LOOSE)
    bool zone_direct = true;      // fixed-bound zone launches without LDS staging and barriers (SMAFA_ZONE_DIRECT=0: the staged form)
    double prune_p = 2e-3;        // prefilter_prunes: largest level-1 pass probability per subject (SMAFA_PRUNE_P)
    bool lazy_fold = true;        // the filter-plane-resident kernel also at the bounds only its level 2 rejects at (SMAFA_LAZY_FOLD=0)
    bool fold3 = true;            // scan_kernel's all-planes-but-the-last bound for launches whose bound starts above 32 (SMAFA_FOLD3=0)
};

struct ScanShape {
    uint32_t P, PQ, W, L;  // planes per subject and per query record, words per plane, columns
};

// P(Binomial(bits, 1/2) <= bound): how often `bits` filter bits in which unrelated sequences differ half the time let a pair through
inline double binom_tail(uint32_t bits, uint32_t bound) {
    if (bound >= bits) return 1.0;
    double term = 1.0, tail = 0.0;  // C(bits, i), summed for i = 0..bound
    for (uint32_t i = 0; i <= bound; i++) {
        tail += term;
        term = term * (double)(bits - i) / (double)(i + 1);
    }
    for (uint32_t i = 0; i < bits; i++) tail *= 0.5;
    return tail;
}

// The filter-plane-resident kernel wins where the prefilter prunes (sparse hits: +18 % aa, 5x less HBM traffic)
// and loses 10-100 % where it cannot (profiles/r01_lazy_vs_resident.txt, r01_length_probe.txt).  Chosen per launch
// from the initial bound, so best-hit scans without --max-divergence (bound = L) and short sequences with a loose
// bound keep the all-planes kernel.
// Level 1 looks at cols = min(32, L) columns of one plane, where unrelated sequences differ in about half: a subject
// passes it with probability P(Binomial(cols, 1/2) <= bound).  The filter-plane-resident kernels pay off while a
// wave's 1024 subjects rarely produce a pass, i.e. while that tail stays below ~2e-3 — for cols = 32 this is
// bound <= 7, the measured crossover (profiles/r01_lazy_vs_resident.txt); short sequences need a tighter bound
// (cols = 20: bound <= 3; cols = 12: bound 0 — L = 12 with bound 2 ran 3x slower through these kernels).
inline bool prefilter_prunes(const ScanShape &s, const ScanKnobs &k, uint32_t bound) {
    const uint32_t cols = s.L < 32u ? s.L : 32u;
    return bound < cols && binom_tail(cols, bound) <= k.prune_p;
}

// Two words per plane: beyond the bounds level 1 prunes at, level 2 still rejects nearly every pair while the bound is well
// below what unrelated sequences score on it — the OR of the two words' mismatch bits has ~3/4 of the second word's columns
// set (+ half of the first word's columns that have no partner): bound <= half of that (L = 60: 12); then the per-word sums up
// to 14 (SUMFOLD).  There the filter-plane-resident kernel — 16 subjects per lane, one plane streamed — beats the all-planes
// one, which only ever uses its other planes for the pairs that pass: 10 000 queries x 10M aa, bound 8 / 9 / 10 / 12:
// 8.7 / 9.5 / 8.9 / 9.6 -> 7.8 / 8.3 / 8.4 / 9.1 ms, bound 14: 12.2 -> 11.3 (tools/bound_probe.py, profiles/r04_bound_probe.txt).
// SMAFA_LAZY_FOLD=0: off.
inline bool fold_rejects(const ScanShape &s, const ScanKnobs &k, uint32_t bound) {
    if (!k.lazy_fold || s.W != 2 || s.L < 56) return false;  // (measured at 60 columns; shorter second words: not claimed)
    const uint32_t second = s.L - 32u;                                    // columns that have a partner in the other word
    const uint32_t unrelated = (3u * second + 2u * (32u - second)) / 4u;  // expected popcount of the OR-fold (L = 60: 23)
    // OR-fold up to 12, the per-word sums (SUMFOLD) at 13 and 14; from 15 on too many wave steps pass level 2 and fetch their
    // tiles from L2 (bound 16: 18.1 ms against 13.8 for the all-planes kernel, whose tiles are resident)
    return bound * 2u <= unrelated + 1u || bound <= 14u;
}

// Does the zone level pay?  A tile that shares b filter bits lets a query unrelated to it through with probability
// P(Binomial(b, 1/2) <= bound); the expected share of (query, tile) pairs that pass follows from the store's measured
// shared-bit histogram (hist[b] = tiles sharing b bits, b = 0..64).  Measured (tools/zone_threshold.sh,
// profiles/r02_zone_threshold.txt): the zone kernel wins while that share stays below ~0.6 — 1M rows at bound 5 (~12 bits,
// 0.39): 0.51 vs 0.64 ms; 250k rows at bound 5 (~10 bits, 0.62): 0.225 vs 0.208 ms; 10M rows at bound 7 (~15 bits, 0.50): 5.8
// vs 6.5 ms.
inline double zone_pass_share(const uint64_t *hist, uint32_t thr0) {
    double tiles = 0.0, pass = 0.0;
    for (uint32_t b = 0; b <= 64; b++) {
        if (!hist[b]) continue;
        tiles += (double)hist[b];
        pass += (double)hist[b] * binom_tail(b, thr0);
    }
    return tiles > 0.0 ? pass / tiles : 1.0;
}

// The pass share a launch is planned with: the store's 65-entry histogram, looked at only where the choice needs the share
// (never with the zone level off or forced), or a value the caller computed once.
struct ZoneShare {
    const uint64_t *hist = nullptr;
    double value = 1.0;
    double at(uint32_t thr0) const { return hist ? zone_pass_share(hist, thr0) : value; }
};

// `prunes`: does level 1 (word 0 of the filter plane) prune at this bound (prefilter_prunes)?  Where it does not — short
// sequences, loose bounds: every (query, tile) pair that passes the zone level goes on to the exact comparison — the
// zone level has to exclude more on its own to beat the all-planes kernel: SMAFA_ZONE_LOOSE (default 0.3).
// Up to 128 columns (W <= 4) the zone level is scan_zone_kernel; longer: the zone level inside scan_wide_kernel (ScanArgs::zone_on).
inline bool zone_pays(const ScanShape &s, const ScanKnobs &k, uint32_t thr0, bool prunes, const ZoneShare &share) {
    if (!k.lazy || !k.use_filter) return false;
    if (k.zone != 1) return k.zone == 2;
    // (five planes of four words: the survivors' levels 2-3 fetch 20 vectors per tile from L2 — the crossover comes
    // earlier: aa 128 columns at bound 7, share 0.5: 11.7 ms vs 9.5 ms without the zone level; 80 columns: 6.6 vs 7.8)
    const double pays = s.W <= 4 && s.P * s.W >= 20 ? 0.4 : 0.6;  // (scan_wide_kernel's own zone level: 0.6)
    return share.at(thr0) < (prunes ? pays : k.zone_loose);
}

// What one launch brings to the choice.
struct ScanLaunch {
    uint32_t thr0;    // the bound the launch starts from, min(max_div, L)
    uint32_t nq;      // queries of the launch
    bool seed;        // no row list and k_tight == 1: the seed pass of the running-minimum mode (lowers bounds, appends nothing)
    bool has_rows;    // the launch appends to a row list
    bool per_query;   // bounds are read per query (k_tight, or fixed per-query bounds): no scalar bound
    ZoneShare share;  // the zone level's pass share
};

enum class ScanFamily { scan, lazy, zone, zone_few, wide, generic };

struct ScanPlan {
    ScanFamily family;
    uint32_t T;         // wave tiles per wave: the kernel's constexpr T, and what the grid is sized by
    uint32_t wg_waves;  // waves per workgroup: kZoneWgWaves only for scan_zone_kernel (more than 64 queries)
    bool seed;          // scan / lazy / wide: the SEED instantiation
    int fold;           // scan_kernel's FOLD, 0..3
    bool sumfold;       // scan_lazy_kernel's SUMFOLD
    bool fixed;         // scan_zone_kernel: one bound for every query (LDS-DMA staging, scalar bound) ...
    bool direct;        // ... or no staging at all (SMAFA_ZONE_DIRECT)
    uint32_t fw, wc;    // scan_wide_kernel: resident filter words, compile-time word count (0: run time)
    bool zone_on;       // scan_wide_kernel: apply its own zone level (ScanArgs::zone_on)
    bool whole_chunks;  // the kernel walks its query block in chunks of kChunk queries: blocks are whole chunks
    bool reported_lazy;  // a filter-plane-resident kernel (wide, lazy or zone): smafa_last_scan_plan, and what a query block reads
};

// More than four words per plane (L > 128): scan_wide_kernel under the lazy kernel's rule — its levels 1 and 2 are the lazy
// kernel's, with 16 subjects per lane whatever the length.  One-word stores (L <= 32) take it too: its level 2
// folds a second plane, which a single filter word needs (up to 1.8x on sparse hits, equal elsewhere).  At W = 3, 4
// it is 8-25 % faster than the per-length kernels on sparse hits but 1.3-2x slower on dense or closely related
// stores (tools/dense_check.py: their level 2 folds every filter word and their full comparison keeps the tile in
// registers), so those lengths keep them; SMAFA_WIDE_FROM=3 switches them over (profiles/r01_wide_vs_lazy.txt).
// Bound too loose, or prefilter off: scan_kernel (W <= 4) / scan_generic_kernel.
inline ScanPlan plan_scan(const ScanShape &s, const ScanKnobs &k, const ScanLaunch &l) {
    ScanPlan p{};
    const bool specialised = s.W <= 4;  // else scan_wide_kernel / scan_generic_kernel
    const bool resident = k.lazy && k.use_filter;
    const bool prunes = resident && prefilter_prunes(s, k, l.thr0);
    const bool wide_shape = s.W >= k.wide_from || (s.W == 1 && k.wide_one);
    const bool wide = prunes && wide_shape && wide_fits((int)s.PQ, (int)s.W);
    const bool lazy = resident && specialised && !wide_shape && (prunes || fold_rejects(s, k, l.thr0));
    // a sorted store whose tiles share enough bits takes the zone kernel at any length up to 128 columns — also where
    // scan_wide_kernel would otherwise run (one-word stores); the seed pass covers a few tiles: no zone level
    const bool zone = specialised && !l.seed && zone_pays(s, k, l.thr0, prunes, l.share);
    p.seed = l.seed;
    p.fixed = !l.per_query;
    p.wg_waves = (uint32_t)kWgWaves;
    p.reported_lazy = wide || lazy || zone;
    if (zone && l.nq <= 64u) {  // up to 64 queries per launch: scan_zone_few_kernel
        p.family = ScanFamily::zone_few;
        p.T = (uint32_t)kFewTiles;
    } else if (zone) {
        p.family = ScanFamily::zone;
        p.direct = p.fixed && k.zone_direct && l.has_rows;
        p.T = (uint32_t)zone_tiles((int)s.P, (int)s.W, p.direct);  // (the unstaged form has its own tile count per shape)
        p.wg_waves = (uint32_t)kZoneWgWaves;
        p.whole_chunks = true;
    } else if (wide) {
        p.family = ScanFamily::wide;
        p.T = (uint32_t)kWideTiles;
        // resident filter words per subject: 1 = one-word store (plus word 0 of a second plane), else 3 (a fourth
        // pushes the kernel past 128 VGPRs: measured spills, and one wave per SIMD less)
        p.fw = s.W == 1 ? 1u : 3u;
        p.wc = (s.W == 3 || s.W == 4) ? s.W : 0u;  // compile-time word count: register-resident dense walk
        p.zone_on = !l.seed && s.W > 4 && zone_pays(s, k, l.thr0, true, l.share);
    } else if (lazy) {
        p.family = ScanFamily::lazy;
        p.T = s.W >= 3 ? 2u : 4u;  // every filter word resident: 8 subjects per lane from 3 words on
        // two words per plane, bound 13..17: level 2 sums the filter plane's per-word popcounts (the OR-fold rejects nothing there)
        p.sumfold = s.W == 2 && !l.seed && l.thr0 > 12u && l.thr0 <= 17u;  // (fold_rejects sends bounds up to 14 here)
    } else if (specialised) {
        p.family = ScanFamily::scan;
        // wave tiles per wave (4*T subjects per lane).  With the cheap first-level bound the per-query work that does
        // not depend on the subject count (LDS read, OR tree, compare, branches, loop bookkeeping) is what T amortises:
        // measured 2 beats 1 for every store with W <= 2 even where it costs occupancy (profiles/r01_variant_tiles*.txt).
        // SMAFA_TILES=1|2|4 overrides (4: 2-plane store only).
        // Two tiles per wave share the per-query work of the bound levels between 8 subjects per lane — which pays while those
        // levels reject most pairs.  Where (nearly) every pair gets the full comparison — prefilter off, or a bound above 16 with
        // four and more planes (FOLD 2 / 3) — one tile per wave is faster: 80 registers less, more waves resident, and for a one-query
        // pass shorter waves that keep the memory pipeline full.  10 000 x 10M aa: prefilter off 30.5 -> 25.4 ms, bound 24
        // 15.0 -> 14.4 ms, best hit without a bound 23.1 -> 21.8 ms, bound 8 the other way (8.3 -> 9.6 ms: stays at two); one query
        // streaming every plane of the 10M store: 70.3 -> 58.4 us = 0.72 -> 0.86 of HBM peak (profiles/r03_stream_nt.txt).
        // (nucleotide stores the same way, less to gain: best hit without a bound, half the queries unrelated, 13.6 -> 12.8 ms)
        p.T = s.W > 2                                               ? 1u
              : k.tiles_override == 4                               ? (s.P == 2 ? 4u : 2u)
              : k.tiles_override == 1 || k.tiles_override == 2      ? k.tiles_override
              : !k.use_filter || l.thr0 > 16u                       ? 1u
                                                                    : 2u;
        // Two words per plane: level 2 by the bound of the launch.  Up to 12 the OR-fold of the filter plane's words (one
        // popcount per subject); 13..17 the filter plane's per-word popcounts summed (FOLD 1: the OR-fold rejects nothing
        // there); 18..32, stores of 3 planes and more, the same over two planes (FOLD 2: flat 14.7 ms from 18 to 28 where the full
        // comparison costs 31, 10 000 queries x 10M aa); beyond that nothing rejects.
        if (SMAFA_SUM_FOLD && s.W == 2 && !l.seed && k.use_filter) {
            if (l.thr0 > 12u && l.thr0 <= 17u) p.fold = 1;
            else if (s.P >= 3 && l.thr0 >= 18u && l.thr0 <= 32u) p.fold = 2;
            else if (s.P >= 4 && l.thr0 > 32u && k.fold3) p.fold = 3;  // all planes but the last (the k-th modes without a bound)
            else if (s.P == 3 && l.thr0 > 32u && k.fold3) p.fold = 2;  // three planes: "all but the last" IS the two-plane form
        }
    } else {
        p.family = ScanFamily::generic;
        p.T = (uint32_t)kGenericTiles;
    }
    return p;
}

// the template-id of the plan's instantiation, as rocprofv3 lists it (the wide kernel's "zone level on" marker is the caller's)
inline std::string scan_kernel_name(const ScanPlan &p, const ScanShape &s) {
    char b[96] = "smafa::scan_generic_kernel";
    const char *yes[2] = {"false", "true"}, *seed = yes[p.seed];
    if (p.family == ScanFamily::scan) snprintf(b, sizeof b, "smafa::scan_kernel<%u, %u, %u, %u, %s, %d>", s.P, s.PQ, s.W, p.T, seed, p.fold);
    if (p.family == ScanFamily::lazy) snprintf(b, sizeof b, "smafa::scan_lazy_kernel<%u, %u, %u, %u, %s, %s>", s.P, s.PQ, s.W, p.T, seed, yes[p.sumfold]);
    if (p.family == ScanFamily::zone) snprintf(b, sizeof b, "smafa::scan_zone_kernel<%u, %u, %u, %s, %s>", s.P, s.PQ, s.W, yes[p.fixed], yes[p.direct]);
    if (p.family == ScanFamily::zone_few) snprintf(b, sizeof b, "smafa::scan_zone_few_kernel<%u, %u, %u>", s.P, s.PQ, s.W);
    if (p.family == ScanFamily::wide) snprintf(b, sizeof b, "smafa::scan_wide_kernel<%u, %u, %s, %u, %u>", s.P, s.PQ, seed, p.fw, p.wc);
    return b;
}

}  // namespace smafa
